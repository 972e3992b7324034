// AA 12-mer window scan shared by the read path (k_extract_aa12, mtb_group.hip) and the common-k-mer
// DB builder's genome path (k_extract_genome_aa12, mtb_common.hip): KmerScanner_dna2aa(12) and
// SyncmerScanner_dna2aa(12, s) restated per window.
#pragma once
#include <cstdint>

#include "mtb_device.h"

namespace mtb {

constexpr uint32_t kGroupChunk = 32;   // windows per extraction unit
constexpr int kGroupK = 12;            // AA k-mer length
constexpr uint64_t kAA12Mask = (1ull << 60) - 1;

struct GroupTables {
    uint8_t base[256];
    int8_t aa[64];
};

// Windows [pFirst, pFirst + nWin) of one frame whose codons span seq[s0 .. e0], after 11 warm-up codons
// (a window depends on its own 12 codons only). Codons are read left to right from s0 on a forward
// frame and from e0 downwards on the complement for a reverse frame. A window is kept iff its 12
// codons translate and, with syncmers, the earliest minimum of its 12 - s + 1 s-mers sits at either
// end (the deque of SyncmerScanner_dna2aa pops strictly greater values only, so its front is the
// earliest minimum). emit(p, kept, value) is called once per window, p = 0 .. nWin - 1 in order.
template <typename Emit>
__device__ __forceinline__ void scan_aa12_chunk(const uint8_t* __restrict__ seq, bool fwd, int s0, int e0, int pFirst,
                                                int nWin, int syncmer, int smerLen, const uint8_t* sBase,
                                                const int8_t* sAA, Emit emit) {
    const int nSm = kGroupK - smerLen + 1;
    const uint64_t smMask = (1ull << (5 * smerLen)) - 1;
    uint64_t aaAcc = 0, smAcc = 0;
    uint64_t sm[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // sm[k]: the s-mer ending k codons back
    int run = 0;
    for (int j = pFirst; j < pFirst + nWin + kGroupK - 1; j++) {
        const int d = fwd ? 1 : -1;
        const int c0 = fwd ? s0 + 3 * j : e0 - 3 * j;
        const uint32_t x = sBase[seq[c0]], y = sBase[seq[c0 + d]], z = sBase[seq[c0 + 2 * d]];
        const uint32_t cm = fwd ? 0u : 2u;  // complement of a valid code (iRCT)
        const bool valid = (x | y | z) < 4u;
        const int aaT = sAA[(((x ^ cm) << 4) | ((y ^ cm) << 2) | (z ^ cm)) & 63u];
        const bool ok = valid && aaT >= 0;
        run = ok ? run + 1 : 0;
        aaAcc = ok ? (aaAcc << 5) | (uint64_t)aaT : aaAcc;
        smAcc = ok ? ((smAcc << 5) | (uint64_t)aaT) & smMask : smAcc;
#pragma unroll
        for (int k = 7; k > 0; k--) sm[k] = sm[k - 1];
        sm[0] = smAcc;
        const int p = j - pFirst - (kGroupK - 1);
        if (p < 0) continue;
        bool keep = run >= kGroupK;
        if (keep && syncmer) {
            int bestK = -1;
            uint64_t best = ~0ull;
#pragma unroll
            for (int k = 7; k >= 0; k--)  // from the oldest s-mer to the newest, strict <: the earliest minimum
                if (k <= nSm - 1 && sm[k] < best) { best = sm[k]; bestK = k; }
            keep = bestK == nSm - 1 || bestK == 0;
        }
        emit(p, keep, aaAcc & kAA12Mask);
    }
}

}  // namespace mtb
