// The common-k-mer DB of read grouping, built on the GPU: the reference's create_common_kmer_list
// (IndexCreator::createCommonKmerIndex, IndexCreator.cpp:231-314).
//   per batch of genomes: the AA 12-mers of all six frames (extractKmer_dna2aa, KmerExtractor.cpp:388-418;
//   payload = the genome's species) -> sort by (value, species) -> one pair per distinct (value, species)
//   (what a flush file of the reference holds once its taxIDs are read back as species)
//   -> folded into the pairs of the batches before it by the two-way merge of mtb_merge.hip and the same
//   dedupe (nothing is dropped before the end: a value under one species so far may meet a second later)
//   -> at the end, N pairs = numOfKmerBeforeMerge; a segmented reduction over each run of equal values
//   with the state (first species, LCA so far, a second species seen), packed in one 64-bit word, combine(a, b)
//   = (a.first, LCA(a.lca, b.lca), a.multi | b.multi | a.first != b.first) -> the runs with the multi bit are
//   the DB (mergeTargetFiles<COMMON_KMER>'s filter, IndexCreator.h:475-629: kept iff some member's species
//   differs from the leader's, info = LCA of the group's species) -> encode_sorted_kmers (mtb_build.hip).
// The COMMON_KMER rule is applied however many batches there were: the reference's one-flush return
// (IndexCreator.cpp:296-299) is not reproduced (DESIGN "Common-k-mer DB").
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mtb_aa12.h"
#include "mtb_host.h"
#include "mtb_launch.h"

namespace mtb {

// 12-mer windows of frame f of a genome of L bases under extractKmer_dna2aa's bounds: a forward frame
// spans [f, L - 1], a reverse frame [0, L - 1 - f % 3] read from its end. (The read path trims every
// frame to getMaxCoveredLength instead: read_windows12, mtb_group.hip.)
__host__ __device__ inline int genome_frame_codons(int64_t L, int f) {
    const int64_t span = L - (f % 3);
    return span > 0 ? (int)(span / 3) : 0;
}
__host__ __device__ inline uint32_t genome_frame_chunks(int64_t L, int f) {
    const int w = genome_frame_codons(L, f) - (kGroupK - 1);
    return w > 0 ? ((uint32_t)w + kGroupChunk - 1) / kGroupChunk : 0u;
}
__host__ __device__ inline uint64_t genome_units(int64_t L) {
    uint64_t u = 0;
    for (int f = 0; f < 6; f++) u += genome_frame_chunks(L, f);
    return u;
}

// One thread per unit: a chunk of <= kGroupChunk windows of one (genome, frame). A unit finds its genome
// by a search over the batch's unit offsets (uOff, nG + 1 entries), so a genome of any length is just
// more units. off: the batch's nG + 1 sequence offsets, seq[off[g] - offBase] the genome's first base.
// Slot u * kGroupChunk + p: (value, the genome's dense species id), or two sentinels.
__global__ void __launch_bounds__(256) k_extract_genome_aa12(const uint8_t* __restrict__ seq, const uint64_t* __restrict__ off,
                                                             uint64_t offBase, const uint64_t* __restrict__ uOff,
                                                             const uint32_t* __restrict__ gSpecies, uint32_t nG,
                                                             uint64_t nUnits, GroupTables tabs, int syncmer, int smerLen,
                                                             uint64_t* __restrict__ keys, uint64_t* __restrict__ pay) {
    __shared__ uint8_t sBase[256];
    __shared__ int8_t sAA[64];
    sBase[threadIdx.x] = tabs.base[threadIdx.x];
    if (threadIdx.x < 64) sAA[threadIdx.x] = tabs.aa[threadIdx.x];
    __syncthreads();
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nUnits) return;
    uint32_t lo = 0, hi = nG;  // the last genome whose first unit is <= u (it has units: uOff[g + 1] > u)
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (uOff[mid] <= u) lo = mid; else hi = mid;
    }
    const uint32_t g = lo;
    const int64_t L = (int64_t)(off[g + 1] - off[g]);
    uint32_t local = (uint32_t)(u - uOff[g]);
    int frame = 0;
    for (; frame < 5; frame++) {
        const uint32_t c = genome_frame_chunks(L, frame);
        if (local < c) break;
        local -= c;
    }
    const int codons = genome_frame_codons(L, frame);
    const int W = codons - (kGroupK - 1);
    const int pFirst = (int)(local * kGroupChunk);
    const int nWin = min((int)kGroupChunk, W - pFirst);
    const bool fwd = frame < 3;
    const int s0 = fwd ? frame : 0, e0 = (int)L - 1 - (fwd ? 0 : frame % 3);
    uint64_t* kOut = keys + u * kGroupChunk;
    uint64_t* pOut = pay + u * kGroupChunk;
    const uint64_t sp = gSpecies[g];
    scan_aa12_chunk(seq + (off[g] - offBase), fwd, s0, e0, pFirst, nWin, syncmer, smerLen, sBase, sAA,
                    [&](int p, bool keep, uint64_t value) {
                        kOut[p] = keep ? value : kSentinel;
                        pOut[p] = keep ? sp : kSentinel;
                    });
    for (int p = max(nWin, 0); p < (int)kGroupChunk; p++) {
        kOut[p] = kSentinel;
        pOut[p] = kSentinel;
    }
}

// heads of the runs of equal (value, species) in (value, species) order, and their compaction
__global__ void k_pair_heads(const uint64_t* __restrict__ v, const uint64_t* __restrict__ p, uint64_t n,
                             uint32_t* __restrict__ head) {
    MTB_GRID_STRIDE(i, n) head[i] = (i == 0 || v[i] != v[i - 1] || p[i] != p[i - 1]) ? 1u : 0u;
}
__global__ void k_pair_compact(const uint64_t* __restrict__ v, const uint64_t* __restrict__ p, uint64_t n,
                               const uint32_t* __restrict__ head, const uint64_t* __restrict__ idx,
                               uint64_t* __restrict__ ov, uint64_t* __restrict__ op) {
    MTB_GRID_STRIDE(i, n)
        if (head[i]) { ov[idx[i]] = v[i]; op[idx[i]] = p[i]; }
}

// ---- the segmented reduction ---------------------------------------------------------------------
// State word: bit 63 a second species seen, bits 31..61 the first species (dense id), bits 0..30 the
// taxonomy node of the LCA so far. kNoState: no record (the identity of combine).
constexpr uint64_t kNoState = ~0ull;
constexpr uint64_t kStateMulti = 1ull << 63;
constexpr uint32_t kReduceBlock = 256;

struct LcaTab {
    const int32_t *parent, *depth;
    __device__ int lca(int i, int j) const {  // NcbiTaxonomy::LCA over nodes, node 0 the root
        if (i == 0 || j == 0) return 0;
        while (i != j) {
            const int di = depth[i], dj = depth[j];
            if (di >= dj) i = parent[i];
            if (dj >= di) j = parent[j];
        }
        return i;
    }
};

__device__ __forceinline__ uint64_t state_combine(uint64_t a, uint64_t b, const LcaTab& t) {
    if (a == kNoState) return b;
    if (b == kNoState) return a;
    const uint64_t firstA = (a >> 31) & 0x7FFFFFFFull, firstB = (b >> 31) & 0x7FFFFFFFull;
    const int la = (int)(a & 0x7FFFFFFFull), lb = (int)(b & 0x7FFFFFFFull);
    const uint64_t multi = ((a | b) & kStateMulti) | (firstA != firstB ? kStateMulti : 0ull);
    return multi | (firstA << 31) | (uint64_t)(la == lb ? la : t.lca(la, lb));
}

// One workgroup per kReduceBlock consecutive pairs, one pair per lane. Within a wave: an inclusive
// segmented scan by __shfl_up over the lanes since the run's head (the head lanes come from one
// ballot); across the four waves: each wave's last lane leaves its tail in LDS and the lanes of a run
// that began in an earlier wave fold the tails back to the wave that holds the head. A run's last lane
// writes the run's state to st (at its own index). A run that began before the block has only its part
// inside the block there; leadEnd[b] names that entry (or kNoState) and k_common_carry completes it
// from blockTail (the state of the block's trailing run part) and blockHead (the block holds a head).
__global__ void __launch_bounds__(kReduceBlock) k_common_reduce_tile(const uint64_t* __restrict__ v,
                                                                     const uint64_t* __restrict__ sp, uint64_t n,
                                                                     const int32_t* __restrict__ spNode, LcaTab tab,
                                                                     uint64_t* __restrict__ st,
                                                                     uint64_t* __restrict__ blockTail,
                                                                     uint32_t* __restrict__ blockHead,
                                                                     uint64_t* __restrict__ leadEnd) {
    constexpr int kWaves = kReduceBlock / 64;
    __shared__ uint64_t sTail[kWaves];
    __shared__ uint32_t sHas[kWaves];
    __shared__ uint64_t sLead;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * kReduceBlock + threadIdx.x;
    const bool in = i < n;
    const uint64_t mine = in ? v[i] : 0ull;
    const bool head = !in || i == 0 || v[i - 1] != mine;
    const bool end = in && (i + 1 == n || v[i + 1] != mine);
    uint64_t x = kNoState;
    if (in) {
        const uint64_t d = sp[i];
        x = (d << 31) | (uint64_t)(uint32_t)spNode[d];
    }
    const unsigned long long heads = __ballot(head);
    const unsigned long long upTo = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1));
    const int hs = upTo ? 63 - __clzll((long long)upTo) : -1;  // the run's head lane; -1: in an earlier wave
    const int from = hs < 0 ? 0 : hs;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(x, d);
        if ((int)lane - d >= from) x = state_combine(up, x, tab);
    }
    if (threadIdx.x == 0) sLead = kNoState;
    if (lane == 63u) {
        sTail[w] = x;
        sHas[w] = heads != 0ull;
    }
    __syncthreads();
    bool open = hs < 0;  // the run began before this wave ... and, after the loop, before this block
    if (open && (end || threadIdx.x == kReduceBlock - 1)) {
        for (int t = (int)w - 1; t >= 0; t--) {
            x = state_combine(sTail[t], x, tab);
            if (sHas[t]) { open = false; break; }
        }
    } else if (open) {
        for (int t = (int)w - 1; t >= 0; t--)
            if (sHas[t]) { open = false; break; }
    }
    if (end) {
        st[i] = x;
        if (open) sLead = i;  // at most one run reaches back past the block's first pair
    }
    if (threadIdx.x == kReduceBlock - 1) {
        blockTail[blockIdx.x] = x;
        blockHead[blockIdx.x] = (sHas[0] | sHas[1] | sHas[2] | sHas[3]) != 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) leadEnd[blockIdx.x] = sLead;
}
static_assert(kReduceBlock == 256, "k_common_reduce_tile folds four waves");

// One thread per block whose first pairs end a run begun earlier: the tails of the blocks before it,
// back to the one that holds the run's head (a run of R pairs is at most R / kReduceBlock + 1 steps).
__global__ void k_common_carry(uint64_t nBlocks, const uint64_t* __restrict__ blockTail,
                               const uint32_t* __restrict__ blockHead, const uint64_t* __restrict__ leadEnd, LcaTab tab,
                               uint64_t* __restrict__ st) {
    MTB_GRID_STRIDE(b, nBlocks) {
        const uint64_t at = leadEnd[b];
        if (at == kNoState || b == 0) continue;
        uint64_t x = st[at];
        for (uint64_t t = b; t-- > 0;) {
            x = state_combine(blockTail[t], x, tab);
            if (blockHead[t]) break;
        }
        st[at] = x;
    }
}

// the runs with a second species: value and the LCA's taxID (as the low word of a builder payload)
__global__ void k_common_flag(const uint64_t* __restrict__ v, const uint64_t* __restrict__ st, uint64_t n,
                              uint32_t* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) flag[i] = (i + 1 == n || v[i + 1] != v[i]) && (st[i] & kStateMulti) ? 1u : 0u;
}
__global__ void k_common_select(const uint64_t* __restrict__ v, const uint64_t* __restrict__ st, uint64_t n,
                                const uint32_t* __restrict__ flag, const uint64_t* __restrict__ idx,
                                const int32_t* __restrict__ nodeTax, uint64_t* __restrict__ ov,
                                uint64_t* __restrict__ op) {
    MTB_GRID_STRIDE(i, n)
        if (flag[i]) {
            ov[idx[i]] = v[i];
            op[idx[i]] = (uint64_t)(uint32_t)nodeTax[st[i] & 0x7FFFFFFFull];
        }
}

namespace {

struct DBuf {  // one device allocation, freed on every return
    void* p = nullptr;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { reset(); }
    void reset() {
        if (p) hipFree(p);
        p = nullptr;
    }
    void swap(DBuf& o) { std::swap(p, o.p); }
    hipError_t alloc(uint64_t bytes) {
        reset();
        return hipMalloc(&p, bytes ? bytes : 8);
    }
    template <typename T>
    T* as() const { return (T*)p; }
};

struct CommonRun {  // stream and events of one build, destroyed on every return
    hipStream_t s = nullptr;
    hipEvent_t a = nullptr, b = nullptr, t0 = nullptr, t1 = nullptr;
    ~CommonRun() {
        if (s) hipStreamSynchronize(s);
        for (hipEvent_t e : {a, b, t0, t1})
            if (e) hipEventDestroy(e);
        if (s) hipStreamDestroy(s);
    }
};

float g_commonMs[6] = {0, 0, 0, 0, 0, 0};
enum { kMsExtract = 0, kMsSort, kMsReduce, kMsFold, kMsEncode, kMsTotal };

#define HIP_C(x)                                                                                \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x);            \
            return e_ == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                        \
        }                                                                                       \
    } while (0)

// a phase's time: begin() before its launches, end(k) after them (waits for the stream)
struct Phase {
    CommonRun& r;
    float* ms;
    int begin() {
        HIP_C(hipEventRecord(r.a, r.s));
        return MTB_OK;
    }
    int end(int k) {
        float t = 0;
        HIP_C(hipEventRecord(r.b, r.s));
        HIP_C(hipEventSynchronize(r.b));
        HIP_C(hipGetLastError());
        HIP_C(hipEventElapsedTime(&t, r.a, r.b));
        ms[k] += t;
        return MTB_OK;
    }
};

// sorted (value, species) pairs with repeats -> the distinct pairs in (ov, op), *outN of them
int dedupe_pairs(const uint64_t* v, const uint64_t* p, uint64_t n, DBuf& ov, DBuf& op, uint64_t* outN, hipStream_t s) {
    DBuf head, idx, tmp;
    HIP_C(head.alloc(4 * (n + 1)));
    HIP_C(idx.alloc(8 * (n + 1)));
    HIP_C(tmp.alloc(8 * scan_tmp_elems(n + 1)));
    if (n) k_pair_heads<<<stride_grid(n), 256, 0, s>>>(v, p, n, head.as<uint32_t>());
    exclusive_scan_u32(head.as<uint32_t>(), n, idx.as<uint64_t>(), tmp.p, s);
    uint64_t U = 0;
    HIP_C(hipMemcpyAsync(&U, idx.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
    HIP_C(hipStreamSynchronize(s));
    HIP_C(ov.alloc(8 * U));
    HIP_C(op.alloc(8 * U));
    if (n)
        k_pair_compact<<<stride_grid(n), 256, 0, s>>>(v, p, n, head.as<uint32_t>(), idx.as<uint64_t>(), ov.as<uint64_t>(),
                                                      op.as<uint64_t>());
    HIP_C(hipGetLastError());
    HIP_C(hipStreamSynchronize(s));
    *outN = U;
    return MTB_OK;
}

// Device bytes of one batch of S slots while it is extracted and sorted: two (value, payload) buffers
// of S pairs, the radix sort's counts, offsets and scan scratch, and (while those are still held) the
// dedupe's flags, indices, scan scratch of its own and output.
uint64_t batch_device_bytes(uint64_t S) {
    const uint64_t rc = radix_counts_elems(S + 1);
    return 32 * (S + 1) + 12 * (rc + 1) + 8 * scan_tmp_elems(rc + S + 2) + 28 * (S + 1) + 8 * scan_tmp_elems(S + 1) +
           (16ull << 20);
}

int common_core(const mtb_build_input* in, const HostTaxonomy& T, const std::vector<uint32_t>& gDense,
                const std::vector<int32_t>& spNode, int syncmer, int smerLen, int device, mtb_db_built* out) {
    const uint32_t nG = in->n_genomes;
    const bool devIn = (in->flags & MTB_INPUT_DEVICE) != 0;
    HIP_C(hipSetDevice(device));
    CommonRun run;
    HIP_C(hipStreamCreateWithFlags(&run.s, hipStreamNonBlocking));
    for (hipEvent_t* e : {&run.a, &run.b, &run.t0, &run.t1}) HIP_C(hipEventCreate(e));
    hipStream_t s = run.s;
    float ms[6] = {0, 0, 0, 0, 0, 0};
    Phase ph{run, ms};
    HIP_C(hipEventRecord(run.t0, s));

    // the genomes' offsets on the host (units, batches) whichever side the sequence is on
    std::vector<uint64_t> off((size_t)nG + 1, 0);
    if (nG) {
        if (devIn) HIP_C(hipMemcpy(off.data(), in->off, 8 * ((size_t)nG + 1), hipMemcpyDeviceToHost));
        else memcpy(off.data(), in->off, 8 * ((size_t)nG + 1));
    }
    if (off[nG] > off[0] && !in->seq) { set_error("null genome sequence"); return MTB_ERR_ARG; }
    std::vector<uint64_t> units((size_t)nG);
    for (uint32_t g = 0; g < nG; g++) {
        if (off[g + 1] < off[g]) { set_error("genome offsets descend"); return MTB_ERR_ARG; }
        if (off[g + 1] - off[g] >= 0x7FFFFF00ull) { set_error("a genome sequence of 2^31 bases or more"); return MTB_ERR_UNSUPPORTED; }
        units[g] = genome_units((int64_t)(off[g + 1] - off[g]));
    }
    uint64_t maxGenomes = ~0ull;  // MTB_COMMON_BATCH_GENOMES: at most this many genomes per batch (tests)
    if (const char* e = getenv("MTB_COMMON_BATCH_GENOMES")) maxGenomes = std::max<uint64_t>(1, strtoull(e, nullptr, 10));

    GroupTables tabs;
    {
        const HostTables ht = make_tables();
        for (int i = 0; i < 256; i++) tabs.base[i] = ht.base[i];
        for (int i = 0; i < 64; i++) tabs.aa[i] = ht.aa[i];
    }
    int spBits = 8;
    while (spBits < 32 && (1ull << spBits) < spNode.size()) spBits += 8;

    DBuf dSpecies, dSpNode, dParent, dDepth, dNodeTax;
    HIP_C(dSpecies.alloc(4 * (uint64_t)nG));
    HIP_C(dSpNode.alloc(4 * spNode.size()));
    HIP_C(dParent.alloc(4 * T.parent.size()));
    HIP_C(dDepth.alloc(4 * T.depth.size()));
    HIP_C(dNodeTax.alloc(4 * T.nodeTax.size()));
    if (nG) {
        HIP_C(hipMemcpyAsync(dSpecies.p, gDense.data(), 4 * (uint64_t)nG, hipMemcpyHostToDevice, s));
        HIP_C(hipMemcpyAsync(dSpNode.p, spNode.data(), 4 * spNode.size(), hipMemcpyHostToDevice, s));
    }
    HIP_C(hipMemcpyAsync(dParent.p, T.parent.data(), 4 * T.parent.size(), hipMemcpyHostToDevice, s));
    HIP_C(hipMemcpyAsync(dDepth.p, T.depth.data(), 4 * T.depth.size(), hipMemcpyHostToDevice, s));
    HIP_C(hipMemcpyAsync(dNodeTax.p, T.nodeTax.data(), 4 * T.nodeTax.size(), hipMemcpyHostToDevice, s));
    HIP_C(hipStreamSynchronize(s));
    const LcaTab lca{dParent.as<int32_t>(), dDepth.as<int32_t>()};

    DBuf accK, accP;  // the distinct (value, species) pairs of the batches so far
    uint64_t accN = 0;
    uint32_t g0 = 0;
    while (g0 < nG) {
        // the batch: as many genomes as fit a quarter of the free memory (the rest is the fold's)
        size_t freeB = 0, totalB = 0;
        HIP_C(hipMemGetInfo(&freeB, &totalB));
        uint32_t g1 = g0;
        uint64_t nUnits = 0;
        while (g1 < nG && g1 - g0 < maxGenomes) {
            const uint64_t nu = nUnits + units[g1];
            const uint64_t seqB = devIn ? 0 : off[g1 + 1] - off[g0];
            if (g1 > g0 && batch_device_bytes(nu * kGroupChunk) + seqB > freeB / 4) break;
            nUnits = nu;
            g1++;
        }
        const uint64_t S = nUnits * kGroupChunk;
        const uint64_t seqBytes = devIn ? 0 : off[g1] - off[g0];
        if (const uint64_t need = batch_device_bytes(S) + seqBytes; need > freeB) {
            set_error("common-k-mer build: a batch of " + std::to_string(g1 - g0) + " genome(s) next to the " +
                      std::to_string(accN) + " k-mers so far needs " + std::to_string(need) +
                      " bytes of device memory, " + std::to_string(freeB) + " are free");
            return MTB_ERR_OOM;
        }
        if (S >= (1ull << 39)) { set_error("a batch of 2^39 slots or more"); return MTB_ERR_UNSUPPORTED; }
        const uint32_t nb = g1 - g0;
        DBuf dSeq, dOff, dUOff, kA, pA, kB, pB, counts, offs, scanTmp;
        const uint8_t* seqPtr;
        const uint64_t* offPtr;
        uint64_t offBase;
        if (devIn) {
            seqPtr = in->seq;
            offPtr = in->off + g0;
            offBase = 0;
        } else {
            HIP_C(dSeq.alloc(seqBytes + 1));
            HIP_C(dOff.alloc(8 * ((uint64_t)nb + 1)));
            if (seqBytes) HIP_C(hipMemcpyAsync(dSeq.p, in->seq + off[g0], seqBytes, hipMemcpyHostToDevice, s));
            HIP_C(hipMemcpyAsync(dOff.p, off.data() + g0, 8 * ((uint64_t)nb + 1), hipMemcpyHostToDevice, s));
            seqPtr = dSeq.as<uint8_t>();
            offPtr = dOff.as<uint64_t>();
            offBase = off[g0];
        }
        std::vector<uint64_t> uOff((size_t)nb + 1, 0);
        for (uint32_t g = 0; g < nb; g++) uOff[g + 1] = uOff[g] + units[g0 + g];
        HIP_C(dUOff.alloc(8 * ((uint64_t)nb + 1)));
        HIP_C(hipMemcpyAsync(dUOff.p, uOff.data(), 8 * ((uint64_t)nb + 1), hipMemcpyHostToDevice, s));
        HIP_C(kA.alloc(8 * (S + 1)));
        HIP_C(pA.alloc(8 * (S + 1)));
        HIP_C(kB.alloc(8 * (S + 1)));
        HIP_C(pB.alloc(8 * (S + 1)));
        const uint64_t rc = radix_counts_elems(S + 1);
        HIP_C(counts.alloc(4 * rc));
        HIP_C(offs.alloc(8 * (rc + 1)));
        HIP_C(scanTmp.alloc(8 * scan_tmp_elems(rc + S + 2)));
        if (int e = ph.begin()) return e;
        if (nUnits)
            k_extract_genome_aa12<<<(unsigned)((nUnits + 255) / 256), 256, 0, s>>>(
                seqPtr, offPtr, offBase, dUOff.as<uint64_t>(), dSpecies.as<uint32_t>() + g0, nb, nUnits, tabs, syncmer,
                smerLen, kA.as<uint64_t>(), pA.as<uint64_t>());
        if (int e = ph.end(kMsExtract)) return e;
        // sort by (value, species): the species digits first (dropping the blank slots), then the value
        if (int e = ph.begin()) return e;
        bool inB1 = false, inB2 = false;
        const uint64_t kept = radix_sort_pairs(pA.as<uint64_t>(), kA.as<uint64_t>(), pB.as<uint64_t>(), kB.as<uint64_t>(), S,
                                               0, spBits, true, false, counts.as<uint32_t>(), offs.as<uint64_t>(),
                                               scanTmp.p, &inB1, s);
        uint64_t* k1 = inB1 ? kB.as<uint64_t>() : kA.as<uint64_t>();
        uint64_t* p1 = inB1 ? pB.as<uint64_t>() : pA.as<uint64_t>();
        uint64_t* k2 = inB1 ? kA.as<uint64_t>() : kB.as<uint64_t>();
        uint64_t* p2 = inB1 ? pA.as<uint64_t>() : pB.as<uint64_t>();
        radix_sort_pairs(k1, p1, k2, p2, kept, 0, 5 * kGroupK, false, false, counts.as<uint32_t>(), offs.as<uint64_t>(),
                         scanTmp.p, &inB2, s);
        const uint64_t* sk = inB2 ? k2 : k1;
        const uint64_t* sp = inB2 ? p2 : p1;
        if (int e = ph.end(kMsSort)) return e;
        // the batch's distinct pairs
        if (int e = ph.begin()) return e;
        DBuf bK, bP;
        uint64_t bN = 0;
        if (int e = dedupe_pairs(sk, sp, kept, bK, bP, &bN, s)) return e;
        if (int e = ph.end(kMsReduce)) return e;
        for (DBuf* d : {&dSeq, &dOff, &dUOff, &kA, &pA, &kB, &pB, &counts, &offs, &scanTmp}) d->reset();
        // fold
        if (int e = ph.begin()) return e;
        if (accN == 0) {
            accK.swap(bK);
            accP.swap(bP);
            accN = bN;
        } else if (bN) {
            const uint64_t total = accN + bN;
            const uint64_t nTiles = (total + kMergeDbTile - 1) / kMergeDbTile;
            if (nTiles > 0x7FFFFFFFull) { set_error("merge of more than 2^31 tiles"); return MTB_ERR_UNSUPPORTED; }
            // the merged pairs next to both inputs, then (the inputs freed) the dedupe's flags, indices and output
            HIP_C(hipMemGetInfo(&freeB, &totalB));
            if (const uint64_t need = 28 * (total + 1) + 8 * (nTiles + 1) + 8 * scan_tmp_elems(total + 1) + (16ull << 20);
                need > freeB) {
                set_error("common-k-mer build: folding " + std::to_string(bN) + " k-mers into " + std::to_string(accN) +
                          " needs " + std::to_string(need) + " bytes of device memory, " + std::to_string(freeB) +
                          " are free");
                return MTB_ERR_OOM;
            }
            DBuf mK, mP, part, nK, nP;
            HIP_C(mK.alloc(8 * total));
            HIP_C(mP.alloc(8 * total));
            HIP_C(part.alloc(8 * (nTiles + 1)));
            launch_merge_pairs(accK.as<uint64_t>(), accP.as<uint64_t>(), accN, bK.as<uint64_t>(), bP.as<uint64_t>(), bN,
                               part.as<uint64_t>(), mK.as<uint64_t>(), mP.as<uint64_t>(), s);
            HIP_C(hipGetLastError());
            HIP_C(hipStreamSynchronize(s));
            accK.reset();
            accP.reset();
            bK.reset();
            bP.reset();
            uint64_t nN = 0;
            if (int e = dedupe_pairs(mK.as<uint64_t>(), mP.as<uint64_t>(), total, nK, nP, &nN, s)) return e;
            accK.swap(nK);
            accP.swap(nP);
            accN = nN;
        }
        if (int e = ph.end(kMsFold)) return e;
        g0 = g1;
    }

    // one record per value, the ones with a second species selected
    DBuf selK, selP;
    uint64_t U = 0;
    {
        if (int e = ph.begin()) return e;
        const uint64_t nBlocks = (accN + kReduceBlock - 1) / kReduceBlock;
        if (nBlocks > 0x7FFFFFFFull) { set_error("reduction of more than 2^31 blocks"); return MTB_ERR_UNSUPPORTED; }
        DBuf st, blockTail, blockHead, leadEnd, flag, idx, tmp;
        HIP_C(st.alloc(8 * accN));
        HIP_C(blockTail.alloc(8 * nBlocks));
        HIP_C(blockHead.alloc(4 * nBlocks));
        HIP_C(leadEnd.alloc(8 * nBlocks));
        HIP_C(flag.alloc(4 * (accN + 1)));
        HIP_C(idx.alloc(8 * (accN + 1)));
        HIP_C(tmp.alloc(8 * scan_tmp_elems(accN + 1)));
        if (accN) {
            k_common_reduce_tile<<<(unsigned)nBlocks, kReduceBlock, 0, s>>>(
                accK.as<uint64_t>(), accP.as<uint64_t>(), accN, dSpNode.as<int32_t>(), lca, st.as<uint64_t>(),
                blockTail.as<uint64_t>(), blockHead.as<uint32_t>(), leadEnd.as<uint64_t>());
            k_common_carry<<<stride_grid(nBlocks), 256, 0, s>>>(nBlocks, blockTail.as<uint64_t>(), blockHead.as<uint32_t>(),
                                                                leadEnd.as<uint64_t>(), lca, st.as<uint64_t>());
            k_common_flag<<<stride_grid(accN), 256, 0, s>>>(accK.as<uint64_t>(), st.as<uint64_t>(), accN, flag.as<uint32_t>());
        }
        exclusive_scan_u32(flag.as<uint32_t>(), accN, idx.as<uint64_t>(), tmp.p, s);
        HIP_C(hipMemcpyAsync(&U, idx.as<uint64_t>() + accN, 8, hipMemcpyDeviceToHost, s));
        HIP_C(hipStreamSynchronize(s));
        HIP_C(selK.alloc(8 * U));
        HIP_C(selP.alloc(8 * U));
        if (accN)
            k_common_select<<<stride_grid(accN), 256, 0, s>>>(accK.as<uint64_t>(), st.as<uint64_t>(), accN, flag.as<uint32_t>(),
                                                              idx.as<uint64_t>(), dNodeTax.as<int32_t>(), selK.as<uint64_t>(),
                                                              selP.as<uint64_t>());
        if (int e = ph.end(kMsReduce)) return e;
    }
    accK.reset();
    accP.reset();
    if (int e = ph.begin()) return e;
    // every value is one group of one taxID here: the builder's tail writes it as it stands, and sizes the
    // split by the pairs before the merge (IndexCreator.h:343)
    if (int rc = encode_sorted_kmers(selK.as<uint64_t>(), selP.as<uint64_t>(), U, T, in->split_num, accN, false,
                                     syncmer ? 5 : 3, nullptr, nullptr, s, out))
        return rc;
    if (int e = ph.end(kMsEncode)) return e;
    {
        std::vector<int32_t> ids(in->genome_taxid, in->genome_taxid + nG);
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        out->n_taxid_list = ids.size();
        out->taxid_list = (int32_t*)malloc(4 * ids.size() + 4);
        memcpy(out->taxid_list, ids.data(), 4 * ids.size());
    }
    HIP_C(hipEventRecord(run.t1, s));
    HIP_C(hipEventSynchronize(run.t1));
    HIP_C(hipEventElapsedTime(&ms[kMsTotal], run.t0, run.t1));
    memcpy(g_commonMs, ms, sizeof(ms));
    return MTB_OK;
}

}  // namespace
}  // namespace mtb

using namespace mtb;

extern "C" {

int mtb_build_common_db(const mtb_build_input* in, const mtb_db_host* taxo, int syncmer, int smer_len, int device,
                        mtb_db_built* out) {
    if (!in || !taxo || !out) { set_error("null argument"); return MTB_ERR_ARG; }
    memset(out, 0, sizeof(*out));
    if (in->n_blocks != 0) { set_error("a common-k-mer build takes whole genomes: n_blocks must be 0"); return MTB_ERR_ARG; }
    if (in->n_genomes && (!in->off || !in->genome_taxid)) { set_error("null genome arrays"); return MTB_ERR_ARG; }
    if (in->split_num < 2) { set_error("split_num must be at least 2"); return MTB_ERR_ARG; }
    if (in->flags & ~(uint32_t)MTB_INPUT_DEVICE) { set_error("a common-k-mer build takes MTB_INPUT_DEVICE only"); return MTB_ERR_ARG; }
    if (syncmer != 0 && syncmer != 1) { set_error("syncmer must be 0 or 1"); return MTB_ERR_ARG; }
    if (syncmer && (smer_len < 5 || smer_len > kGroupK)) {
        set_error("smer_len must be in [5, 12] (at most 8 s-mers per 12-mer)");
        return MTB_ERR_ARG;
    }
    if (!taxo->node_taxid || !taxo->node_parent || !taxo->rank_pool || !taxo->rank_off) {
        set_error("null taxonomy arrays");
        return MTB_ERR_ARG;
    }
    HostTaxonomy T;
    {
        std::vector<std::string> ranks(taxo->n_nodes), names(taxo->n_nodes);
        for (uint64_t i = 0; i < taxo->n_nodes; i++) {
            ranks[i] = taxo->rank_pool + taxo->rank_off[i];
            if (taxo->name_pool) names[i] = taxo->name_pool + taxo->name_off[i];
        }
        if (!build_taxonomy(taxo->node_taxid, taxo->node_parent, taxo->n_nodes, ranks, names, taxo->merged_old,
                            taxo->merged_new, taxo->n_merged, T))
            return MTB_ERR_DB;
    }
    // every genome's species from the taxonomy (as mtb_build_db); dense ids keep the sort's digits few
    std::vector<int32_t> gSp(in->n_genomes), species;
    for (uint32_t g = 0; g < in->n_genomes; g++) {
        const int32_t t = in->genome_taxid[g];
        const int32_t sp = T.exists(t) ? T.taxIdAtRank(t, "species") : 0;
        if (sp <= 0 || !T.exists(sp) || T.rank[T.nodeOf[sp]] != "species") {
            set_error("genome " + std::to_string(g) + ": taxID " + std::to_string(t) + " has no species in the taxonomy");
            return MTB_ERR_DB;
        }
        gSp[g] = sp;
    }
    species = gSp;
    std::sort(species.begin(), species.end());
    species.erase(std::unique(species.begin(), species.end()), species.end());
    std::vector<uint32_t> gDense(in->n_genomes);
    std::vector<int32_t> spNode(species.size());
    for (size_t k = 0; k < species.size(); k++) spNode[k] = T.nodeOf[species[k]];
    for (uint32_t g = 0; g < in->n_genomes; g++)
        gDense[g] = (uint32_t)(std::lower_bound(species.begin(), species.end(), gSp[g]) - species.begin());
    const int rc = common_core(in, T, gDense, spNode, syncmer, syncmer ? smer_len : kGroupK, device, out);
    if (rc != MTB_OK) mtb_free_built(out);
    return rc;
}

int mtb_common_last_ms(float* ms, int n) {
    if (!ms || n < 0) { set_error("null argument"); return MTB_ERR_ARG; }
    const int k = std::min(n, 6);
    for (int i = 0; i < k; i++) ms[i] = g_commonMs[i];
    return k;
}

uint32_t mtb_common_unit_windows(void) { return kGroupChunk; }

}  // extern "C"
