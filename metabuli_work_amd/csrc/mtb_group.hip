// Read grouping on the GPU (the reference fork's src/read-group/, workflow groupGeneration). First half:
// the three grouping phases over a resident edge list; second half: the shared-k-mer graph those edges
// come from (AA 12-mer extraction, the common-k-mer filter, sort, run pass, pair rounds) and the
// mtb_group_* entry points.
//   Phase 1   makeGroups        (GroupGenerator.cpp:1469-1552): union id1, id2 of every edge with
//             weight > coreThr; a read is grouped iff such an edge touches it; label = smallest read ID
//   Phase 1.5 mergeBySupport    (GroupGenerator.cpp:1577-1976, mergeSupportRatio = 0, mergeMaxUnitReads = 0):
//             weak edges (weakThr < w <= coreThr) counted per unordered pair of units (a read's Phase-1
//             group, or the read itself), pairs with >= 2 of them united onto Phase 1's components
//   Phase 2   makeGroupsPhase2  (GroupGenerator.cpp:1978-2053): Phase 1's rule with weight > weakThr
//             over the edges whose two ends are both still ungrouped
// The reference runs one DisjointSet per thread over relations_* files and merges them; the components
// and their smallest IDs do not depend on that order, so one lock-free union-find serves: every hook
// sets the larger root's parent to the smaller root (compare-and-swap, retried when it loses), hence a
// component's root is its smallest read ID by construction and no rootToMin pass is needed.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "mtb_aa12.h"
#include "mtb_host.h"
#include "mtb_launch.h"

namespace mtb {

// Parents are read and written by every workgroup of a launch: the per-CU L1 is not refreshed by other
// CUs' stores, so every access is an agent-scope atomic (a find that re-read a stale "x is a root" from
// L1 would retry its compare-and-swap forever).
__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A parent only ever moves to an ancestor, and every ancestor has a smaller ID: shortcuts are written
// with atomicMin, so a late shortcut (a grandparent read before another thread stored the root) never
// puts a farther ancestor back over a nearer one. After k_uf_flatten every parent is therefore the root.
__device__ __forceinline__ void uf_store(uint32_t* p, uint32_t v) { atomicMin(p, v); }

// Root of x with path halving.
__device__ __forceinline__ uint32_t uf_find(uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = uf_load(parent + x);
        if (p == x) return x;
        const uint32_t g = uf_load(parent + p);
        if (g != p) uf_store(parent + x, g);
        x = g;
    }
}

__device__ __forceinline__ void uf_unite(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        // only a root is hooked (expected value: itself), and only below itself
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
    }
}

__device__ __forceinline__ bool bit_at(const uint32_t* bits, uint32_t i) { return (bits[i >> 5] >> (i & 31u)) & 1u; }

__global__ void k_uf_init(uint32_t* __restrict__ parent, uint64_t n) {
    MTB_GRID_STRIDE(i, n) parent[i] = (uint32_t)i;
}

// Phases 1 and 2: edges with weight > thr whose ends are both outside `excluded` (null: none) are
// united, their ends marked in `grouped`. IDs outside 1 .. N are skipped as the reference skips them.
__global__ void __launch_bounds__(256) k_uf_hook(const mtb_relation* __restrict__ edges, uint64_t nE, int thr,
                                                 const uint32_t* __restrict__ excluded, uint32_t N,
                                                 uint32_t* parent, uint32_t* grouped) {
    MTB_GRID_STRIDE(i, nE) {
        const mtb_relation e = edges[i];
        if ((int)e.weight <= thr) continue;
        if (e.id1 == 0 || e.id2 == 0 || e.id1 > N || e.id2 > N) continue;
        if (excluded && (bit_at(excluded, e.id1) || bit_at(excluded, e.id2))) continue;
        atomicOr(grouped + (e.id1 >> 5), 1u << (e.id1 & 31u));
        atomicOr(grouped + (e.id2 >> 5), 1u << (e.id2 & 31u));
        uf_unite(parent, e.id1, e.id2);
    }
}

__global__ void k_uf_flatten(uint32_t* parent, uint64_t n) {
    MTB_GRID_STRIDE(i, n) {
        const uint32_t r = uf_find(parent, (uint32_t)i);
        uf_store(parent + i, r);
    }
}

// groupMap after a phase: the root of a grouped read, else the earlier map's entry (null: 0)
__global__ void k_uf_label(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ grouped,
                           const uint32_t* __restrict__ prev, uint64_t n, uint32_t* __restrict__ out) {
    MTB_GRID_STRIDE(i, n) out[i] = i && bit_at(grouped, (uint32_t)i) ? parent[i] : (prev && i ? prev[i] : 0u);
}

// Phase 1.5's key per edge: the unit pair (smaller << nb | larger, nb = bits of N) of a weak edge that
// counts, else the sentinel. parent is flattened Phase 1: a read's unit is its root (itself when ungrouped).
__global__ void __launch_bounds__(256) k_weak_keys(const mtb_relation* __restrict__ edges, uint64_t nE, int weakThr,
                                                   int coreThr, uint32_t N, int nb,
                                                   const uint32_t* __restrict__ parent,
                                                   const uint32_t* __restrict__ grouped, uint64_t* __restrict__ keys) {
    MTB_GRID_STRIDE(i, nE) {
        const mtb_relation e = edges[i];
        const int w = (int)e.weight;
        uint64_t key = kSentinel;
        if (e.id1 && e.id2 && e.id1 <= N && e.id2 <= N && w > weakThr && w <= coreThr &&
            (bit_at(grouped, e.id1) || bit_at(grouped, e.id2))) {
            const uint32_t u = parent[e.id1], v = parent[e.id2];
            if (u != v) key = (uint64_t)(u < v ? u : v) << nb | (u < v ? v : u);
        }
        keys[i] = key;
    }
}

// The sorted unit pairs: a pair seen at least twice (the head of a run of >= 2) is united, both units marked.
__global__ void __launch_bounds__(256) k_uf_hook_pairs(const uint64_t* __restrict__ keys, uint64_t n, int nb,
                                                       uint32_t* parent, uint32_t* grouped) {
    MTB_GRID_STRIDE(i, n) {
        if (i + 1 >= n) continue;
        const uint64_t k = keys[i];
        if (keys[i + 1] != k || (i && keys[i - 1] == k)) continue;
        const uint32_t u = (uint32_t)(k >> nb), v = (uint32_t)(k & ((1ull << nb) - 1));
        atomicOr(grouped + (u >> 5), 1u << (u & 31u));
        atomicOr(grouped + (v >> 5), 1u << (v & 31u));
        uf_unite(parent, u, v);
    }
}

namespace {

#define GRP_TRY(x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x);      \
            return e_ == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                 \
        }                                                                                 \
    } while (0)

struct Buf {  // device scratch of one entry point, freed on every return path
    void* p = nullptr;
    hipError_t alloc(size_t bytes) {
        if (p) hipFree(p);
        p = nullptr;
        return hipMalloc(&p, bytes ? bytes : 16);
    }
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { if (p) hipFree(p); }
    template <typename T>
    T* as() const { return (T*)p; }
};

int bits_of(uint64_t x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

int check_params(const mtb_group_params* par) {
    if (!par) { set_error("null parameters"); return MTB_ERR_ARG; }
    if (par->merge_support_ratio > 0.0f) {
        set_error("merge_support_ratio > 0: the outcome depends on merge order and per-thread caps");
        return MTB_ERR_UNSUPPORTED;
    }
    if (par->merge_max_unit_reads > 0) {
        set_error("merge_max_unit_reads > 0: the outcome depends on merge order");
        return MTB_ERR_UNSUPPORTED;
    }
    if (!(par->min_overlap_ratio > 0.0f)) { set_error("min_overlap_ratio must be > 0"); return MTB_ERR_ARG; }
    if (!(par->weak_band_ratio > 0.0f) || !(par->weak_band_ratio < 1.0f)) {
        set_error("weak_band_ratio must be in (0, 1)");
        return MTB_ERR_ARG;
    }
    return MTB_OK;
}

// GroupGenerator.cpp:171-192 in its own types: float x double for the core threshold, float x int for
// the weak band's lower bound.
int thresholds(const mtb_group_params& par, uint64_t totalKmers, uint64_t reads, int* core, int* weak) {
    const double kmersPerRead = reads > 0 ? static_cast<double>(totalKmers) / static_cast<double>(reads) : 0.0;
    const int coreThr = static_cast<int>(par.min_overlap_ratio * kmersPerRead + 0.5);
    if (coreThr < 2) {
        set_error("core threshold resolves to " + std::to_string(coreThr) + " (it must be at least 2)");
        return MTB_ERR_ARG;
    }
    int weakThr = static_cast<int>(par.weak_band_ratio * coreThr + 0.5f);
    if (weakThr < 1) weakThr = 1;
    if (weakThr >= coreThr) weakThr = coreThr - 1;
    *core = coreThr;
    *weak = weakThr;
    return MTB_OK;
}

// The three phases over nE device edges of reads 1 .. N; maps: 3 * (N + 1) device words, the groupMap
// after each phase. ms (nullable): 3 phase times.
int run_phases(const mtb_relation* edges, uint64_t nE, uint32_t N, int coreThr, int weakThr, uint32_t* maps, float* ms,
               hipStream_t s) {
    const uint64_t n1 = (uint64_t)N + 1, words = (n1 + 31) / 32;
    const int nb = bits_of(N);
    Buf parent, parent2, grouped, grouped2, ka, kb, va, vb, cnt, offs, tmp;
    GRP_TRY(parent.alloc(4 * n1));
    GRP_TRY(parent2.alloc(4 * n1));
    GRP_TRY(grouped.alloc(4 * words));
    GRP_TRY(grouped2.alloc(4 * words));
    hipEvent_t ev[4];
    for (auto& e : ev) GRP_TRY(hipEventCreate(&e));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 4; i++) hipEventDestroy(e[i]); } } guard{ev};
    uint32_t* map1 = maps, *map2 = maps + n1, *map3 = maps + 2 * n1;

    // Phase 1
    GRP_TRY(hipEventRecord(ev[0], s));
    GRP_TRY(hipMemsetAsync(grouped.p, 0, 4 * words, s));
    k_uf_init<<<stride_grid(n1), 256, 0, s>>>(parent.as<uint32_t>(), n1);
    if (nE) k_uf_hook<<<stride_grid(nE), 256, 0, s>>>(edges, nE, coreThr, nullptr, N, parent.as<uint32_t>(), grouped.as<uint32_t>());
    k_uf_flatten<<<stride_grid(n1), 256, 0, s>>>(parent.as<uint32_t>(), n1);
    k_uf_label<<<stride_grid(n1), 256, 0, s>>>(parent.as<uint32_t>(), grouped.as<uint32_t>(), nullptr, n1, map1);
    GRP_TRY(hipEventRecord(ev[1], s));

    // Phase 1.5
    if (nE) {
        const uint64_t rc = radix_counts_elems(nE + 1);
        GRP_TRY(ka.alloc(8 * (nE + 1)));
        GRP_TRY(kb.alloc(8 * (nE + 1)));
        GRP_TRY(va.alloc(4 * (nE + 1)));
        GRP_TRY(vb.alloc(4 * (nE + 1)));
        GRP_TRY(cnt.alloc(4 * rc));
        GRP_TRY(offs.alloc(8 * (rc + 1)));
        GRP_TRY(tmp.alloc(8 * scan_tmp_elems(rc + nE + 2)));
        k_weak_keys<<<stride_grid(nE), 256, 0, s>>>(edges, nE, weakThr, coreThr, N, nb, parent.as<uint32_t>(),
                                                    grouped.as<uint32_t>(), ka.as<uint64_t>());
        GRP_TRY(hipMemsetAsync(va.p, 0, 4 * nE, s));  // the sort carries values; the pairs need none
        bool inB = false;
        const uint64_t kept = radix_sort_pairs<uint32_t>(ka.as<uint64_t>(), va.as<uint32_t>(), kb.as<uint64_t>(),
                                                         vb.as<uint32_t>(), nE, 0, 2 * nb, true, false,
                                                         cnt.as<uint32_t>(), offs.as<uint64_t>(), tmp.p, &inB, s);
        GRP_TRY(hipGetLastError());
        if (kept > nE) { set_error("radix sort kept more pairs than it was given"); return MTB_ERR_INTERNAL; }
        if (kept > 1)
            k_uf_hook_pairs<<<stride_grid(kept), 256, 0, s>>>(inB ? kb.as<uint64_t>() : ka.as<uint64_t>(), kept, nb,
                                                              parent.as<uint32_t>(), grouped.as<uint32_t>());
        k_uf_flatten<<<stride_grid(n1), 256, 0, s>>>(parent.as<uint32_t>(), n1);
    }
    k_uf_label<<<stride_grid(n1), 256, 0, s>>>(parent.as<uint32_t>(), grouped.as<uint32_t>(), nullptr, n1, map2);
    GRP_TRY(hipEventRecord(ev[2], s));

    // Phase 2: a fresh union-find over the reads Phase 1.5 left ungrouped; its labels go over map2
    GRP_TRY(hipMemsetAsync(grouped2.p, 0, 4 * words, s));
    k_uf_init<<<stride_grid(n1), 256, 0, s>>>(parent2.as<uint32_t>(), n1);
    if (nE) k_uf_hook<<<stride_grid(nE), 256, 0, s>>>(edges, nE, weakThr, grouped.as<uint32_t>(), N, parent2.as<uint32_t>(), grouped2.as<uint32_t>());
    k_uf_flatten<<<stride_grid(n1), 256, 0, s>>>(parent2.as<uint32_t>(), n1);
    k_uf_label<<<stride_grid(n1), 256, 0, s>>>(parent2.as<uint32_t>(), grouped2.as<uint32_t>(), map2, n1, map3);
    GRP_TRY(hipEventRecord(ev[3], s));
    GRP_TRY(hipGetLastError());
    GRP_TRY(hipStreamSynchronize(s));
    if (ms)
        for (int i = 0; i < 3; i++) GRP_TRY(hipEventElapsedTime(ms + i, ev[i], ev[i + 1]));
    return MTB_OK;
}

// groups and grouped reads of a host map (N + 1 entries)
void count_groups(const uint32_t* map, uint32_t N, uint64_t* groups, uint64_t* groupedReads) {
    uint64_t g = 0, r = 0;
    for (uint64_t i = 1; i <= N; i++) {
        g += map[i] == i;
        r += map[i] != 0;
    }
    *groups = g;
    *groupedReads = r;
}

}  // namespace
}  // namespace mtb

using namespace mtb;

extern "C" void mtb_group_default_params(mtb_group_params* par) {
    if (!par) return;
    memset(par, 0, sizeof(*par));
    // setGroupGenerationDefaults (groupGeneration.cpp:9-58)
    par->seq_mode = 2;
    par->syncmer = 1;
    par->smer_len = 5;
    par->max_kmer_reads = 1000;
    par->max_kmer_quantile = 0.0f;
    par->min_overlap_ratio = 0.3f;
    par->weak_band_ratio = 0.3333f;
    par->merge_support_ratio = 0.0f;
    par->merge_max_unit_reads = 0;
}

extern "C" int mtb_group_make_groups(int device, const mtb_relation* edges, uint64_t n_edges, uint32_t n_reads,
                                     uint64_t total_kmers, const mtb_group_params* par, uint32_t* phase_maps,
                                     mtb_group_stats* stats) {
    if (const int rc = check_params(par)) return rc;
    if (!phase_maps || (n_edges && !edges)) { set_error("null argument"); return MTB_ERR_ARG; }
    if (n_reads >= 0xFFFFFFFFu) { set_error("2^32 - 1 reads or more"); return MTB_ERR_ARG; }
    int coreThr = 0, weakThr = 0;
    if (const int rc = thresholds(*par, total_kmers, n_reads, &coreThr, &weakThr)) return rc;
    GRP_TRY(hipSetDevice(device));
    const uint64_t n1 = (uint64_t)n_reads + 1;
    Buf dEdges, dMaps;
    GRP_TRY(dEdges.alloc(sizeof(mtb_relation) * n_edges));
    GRP_TRY(dMaps.alloc(4 * 3 * n1));
    if (n_edges) GRP_TRY(hipMemcpy(dEdges.p, edges, sizeof(mtb_relation) * n_edges, hipMemcpyHostToDevice));
    float ms[3] = {0, 0, 0};
    if (const int rc = run_phases(dEdges.as<mtb_relation>(), n_edges, n_reads, coreThr, weakThr, dMaps.as<uint32_t>(), ms, nullptr))
        return rc;
    GRP_TRY(hipMemcpy(phase_maps, dMaps.p, 4 * 3 * n1, hipMemcpyDeviceToHost));
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->reads = n_reads;
        stats->kmers = total_kmers;
        stats->edges = n_edges;
        stats->core_thr = coreThr;
        stats->weak_thr = weakThr;
        for (int p = 0; p < 3; p++) {
            count_groups(phase_maps + p * n1, n_reads, &stats->groups_after[p], &stats->grouped_after[p]);
            stats->ms[5 + p] = ms[p];
        }
    }
    return MTB_OK;
}

// ------------------------------------------------------------------------------------------------
// The shared-k-mer graph: AA 12-mers of every read (fillQueryKmerBuffer, KmerExtractor.cpp:355-386,
// with KmerScanner_dna2aa(12) — kmerFormat 3, KmerScanner.h:185-261 — or SyncmerScanner_dna2aa(12, s)
// — kmerFormat 5, SyncmerScanner.h:192-295), sorted by value; per distinct value its distinct reads
// (m of them); every kept value adds 1 to each pair of its reads (makeSubGraph / scanKmerRuns,
// GroupGenerator.cpp:649-701, GroupGenerator.h:756-808).
// ------------------------------------------------------------------------------------------------
namespace mtb {

// 12-mer windows per frame of each mate (0, 0 when the shared empty-read rule drops the read:
// KmerExtractor.cpp:451-494 with kmerLen 12) and the read's units: chunks of kGroupChunk windows per
// (mate, frame).
__device__ __forceinline__ int windows12(int len) {
    const int w = len >= 3 ? max_covered_length(len) / 3 - kGroupK + 1 : 0;
    return w > 0 ? w : 0;
}
__device__ __forceinline__ void read_windows12(const ReadMeta& m, int paired, int& w1, int& w2) {
    w1 = windows12(m.len1);
    w2 = paired ? windows12(m.len2) : 0;
    if (paired && (w1 < 1 || w2 < 1)) w1 = w2 = 0;
}
__global__ void k_group_units(const ReadMeta* __restrict__ meta, uint32_t n, int paired, uint32_t* __restrict__ units) {
    MTB_GRID_STRIDE(i, n) {
        int w1, w2;
        read_windows12(meta[i], paired, w1, w2);
        units[i] = 6u * (((uint32_t)w1 + kGroupChunk - 1) / kGroupChunk + ((uint32_t)w2 + kGroupChunk - 1) / kGroupChunk);
    }
}

// One thread per unit: a chunk of <= kGroupChunk consecutive windows of one (read, mate, frame),
// scanned by scan_aa12_chunk (mtb_aa12.h), frames as K1's format 2. Slot u * kGroupChunk + p holds window p of unit
// u: (key, global read ID), or the sentinel. Units are in read order, so slot order is ascending in
// read ID — the order the stable sort keeps within a key.
__global__ void __launch_bounds__(256) k_extract_aa12(const uint8_t* __restrict__ seq1, const uint64_t* __restrict__ off1,
                                                      const uint8_t* __restrict__ seq2, const uint64_t* __restrict__ off2,
                                                      const ReadMeta* __restrict__ meta, const uint64_t* __restrict__ uOff,
                                                      const uint32_t* __restrict__ unitRead, uint64_t nUnits, int paired,
                                                      GroupTables tabs, int syncmer, int smerLen, uint32_t idBase,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ ids,
                                                      uint32_t* __restrict__ pos) {
    __shared__ uint8_t sBase[256];
    __shared__ int8_t sAA[64];
    sBase[threadIdx.x] = tabs.base[threadIdx.x];
    if (threadIdx.x < 64) sAA[threadIdx.x] = tabs.aa[threadIdx.x];
    __syncthreads();
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nUnits) return;
    const uint32_t r = unitRead[u];
    const ReadMeta m = meta[r];
    int w1, w2;
    read_windows12(m, paired, w1, w2);
    const uint32_t c1 = ((uint32_t)w1 + kGroupChunk - 1) / kGroupChunk, c2 = ((uint32_t)w2 + kGroupChunk - 1) / kGroupChunk;
    uint32_t local = (uint32_t)(u - uOff[r]), cpf = c1;
    int mate = 0;
    if (local >= 6 * c1) { local -= 6 * c1; mate = 1; cpf = c2; }
    const int frame = (int)(local / cpf), chunk = (int)(local % cpf);
    const int W = mate ? w2 : w1;
    const int pFirst = chunk * (int)kGroupChunk;
    const int nWin = min((int)kGroupChunk, W - pFirst);
    const uint8_t* seq = mate ? seq2 + off2[r] : seq1 + off1[r];
    const int len = mate ? m.len2 : m.len1;
    const int used = max_covered_length(len);
    const bool fwd = frame < 3;
    int begin;
    if (fwd) begin = frame;
    else { begin = (len % 3) - (frame % 3); if (begin < 0) begin += 3; }
    const int s0 = begin, e0 = begin + used - 1;
    uint64_t* kOut = keys + u * kGroupChunk;
    uint32_t* iOut = ids + u * kGroupChunk;
    const uint32_t id = idBase + r + 1;
    // pos (null without a common-k-mer set): the scanners' nucleotide position of window P of the frame —
    // frame + 3 P forward, seqEnd - 3 (P + 12) + 1 on a reverse frame (KmerScanner.h:253-257,
    // SyncmerScanner.h:287-289), mate 2 after getMaxCoveredLength(len1) + 3 (KmerExtractor.cpp:341-345)
    uint32_t* pOut = pos ? pos + u * kGroupChunk : nullptr;
    const int posBase = (fwd ? s0 : e0 - 3 * kGroupK + 1) + (mate ? max_covered_length(m.len1) + 3 : 0);
    scan_aa12_chunk(seq, fwd, s0, e0, pFirst, nWin, syncmer, smerLen, sBase, sAA, [&](int p, bool keep, uint64_t value) {
        kOut[p] = keep ? value : kSentinel;
        iOut[p] = id;
        if (pOut) pOut[p] = (uint32_t)(fwd ? posBase + 3 * (pFirst + p) : posBase - 3 * (pFirst + p));
    });
    for (int p = max(nWin, 0); p < (int)kGroupChunk; p++) {
        kOut[p] = kSentinel;
        iOut[p] = id;
        if (pOut) pOut[p] = 0;
    }
}

__global__ void k_flag_kept(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) flag[i] = keys[i] != kSentinel;
}
// stable compaction of the kept slots to dst (at the scan's offsets)
__global__ void k_compact_kmers(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ids, uint64_t n,
                                const uint64_t* __restrict__ off, uint64_t* __restrict__ dKeys,
                                uint32_t* __restrict__ dIds) {
    MTB_GRID_STRIDE(i, n)
        if (keys[i] != kSentinel) { dKeys[off[i]] = keys[i]; dIds[off[i]] = ids[i]; }
}

// ------------------------------------------------------------------------------------------------
// The common-k-mer filter (filterCommonKmers, GroupGenerator.cpp:228-408): an instance is hit iff its
// value is in the set, removed iff a hit of its read lies within one nucleotide of it.
// The set: its distinct values ascending in HBM, cut into leaves of kSetLeaf values; mid holds every
// leaf's first value; top holds every T-th mid entry, at most kSetTop of them (T = 1 up to
// kSetLeaf * kSetTop values: top = mid). A block stages top in LDS once and answers its queries by
// three searches: top in LDS, at most T mid entries (one stretch of HBM, shared through L2 by every
// query between the same two top entries), one leaf (512 B).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kSetLeaf = 64;
constexpr uint32_t kSetTop = 4096;
constexpr uint32_t kNbrLdsBits = 4096;  // a read's position bitmap held on chip

struct SetIndex {
    const uint64_t *set, *mid, *top;
    uint64_t n, nMid, T;
    uint32_t nTop;
};

// flag the first of each run of equal values (prev: the value before vals[0], when hasPrev); a value
// below the one before it sets *desc
__global__ void k_set_flag(const uint64_t* __restrict__ vals, uint64_t n, int hasPrev, uint64_t prev,
                           uint32_t* __restrict__ flag, int* __restrict__ desc) {
    MTB_GRID_STRIDE(i, n) {
        const uint64_t v = vals[i];
        const bool first = i == 0 && !hasPrev;
        const uint64_t b = i ? vals[i - 1] : prev;
        if (!first && v < b) *desc = 1;
        flag[i] = first || v != b;
    }
}
__global__ void k_compact_u64(const uint64_t* __restrict__ in, const uint32_t* __restrict__ flag,
                              const uint64_t* __restrict__ off, uint64_t n, uint64_t* __restrict__ out) {
    MTB_GRID_STRIDE(i, n)
        if (flag[i]) out[off[i]] = in[i];
}
__global__ void k_compact_u32(const uint32_t* __restrict__ in, const uint32_t* __restrict__ flag,
                              const uint64_t* __restrict__ off, uint64_t n, uint32_t* __restrict__ out) {
    MTB_GRID_STRIDE(i, n)
        if (flag[i]) out[off[i]] = in[i];
}
__global__ void k_set_sample(const uint64_t* __restrict__ src, uint64_t stride, uint64_t nOut, uint64_t* __restrict__ out) {
    MTB_GRID_STRIDE(i, nOut) out[i] = src[i * stride];
}

// hit[i] = keys[i] is in the set (a sentinel slot never is)
__global__ void __launch_bounds__(256) k_set_member(SetIndex ix, const uint64_t* __restrict__ keys, uint64_t n,
                                                    int skipSentinel, uint8_t* __restrict__ hit) {
    __shared__ uint64_t sTop[kSetTop];
    for (uint32_t i = threadIdx.x; i < ix.nTop; i += blockDim.x) sTop[i] = ix.top[i];
    __syncthreads();
    MTB_GRID_STRIDE(i, n) {
        const uint64_t q = keys[i];
        uint8_t h = 0;
        if (!(skipSentinel && q == kSentinel) && q >= sTop[0]) {
            uint32_t lo = 0, hi = ix.nTop - 1;  // the last top entry <= q
            while (lo < hi) {
                const uint32_t m = (lo + hi + 1) >> 1;
                if (sTop[m] <= q) lo = m; else hi = m - 1;
            }
            uint64_t a = (uint64_t)lo * ix.T, b = a + ix.T < ix.nMid ? a + ix.T - 1 : ix.nMid - 1;  // the last leaf head <= q
            while (a < b) {
                const uint64_t m = a + (b - a + 1) / 2;
                if (ix.mid[m] <= q) a = m; else b = m - 1;
            }
            uint64_t l = a * kSetLeaf, r = l + kSetLeaf < ix.n ? l + kSetLeaf : ix.n;
            const uint64_t end = r;
            while (l < r) {
                const uint64_t m = l + ((r - l) >> 1);
                if (ix.set[m] < q) l = m + 1; else r = m;
            }
            h = l < end && ix.set[l] == q;
        }
        hit[i] = h;
    }
}

// flag the first instance of each read (read IDs non-descending; a descent sets *desc)
__global__ void k_flag_read_heads(const uint32_t* __restrict__ ids, uint64_t n, uint32_t* __restrict__ flag,
                                  int* __restrict__ desc) {
    MTB_GRID_STRIDE(i, n) {
        if (i && ids[i] < ids[i - 1]) *desc = 1;
        flag[i] = i == 0 || ids[i] != ids[i - 1];
    }
}
__global__ void k_pos_range(const uint32_t* __restrict__ pos, uint64_t n, int* __restrict__ bad) {
    MTB_GRID_STRIDE(i, n) if (pos[i] >> 31) *bad = 1;
}

// Segment g (a read) holds the instances [off[g] * mul, off[g + 1] * mul). One wave per segment: the
// words of the bitmap its hits need (bits 0 .. last hit + 1), 0 when the on-chip bitmap holds them.
__global__ void __launch_bounds__(64) k_seg_span(const uint64_t* __restrict__ off, uint32_t mul, uint64_t nSeg,
                                                 const uint32_t* __restrict__ pos, const uint8_t* __restrict__ hit,
                                                 uint32_t* __restrict__ bigWords) {
    for (uint64_t g = blockIdx.x; g < nSeg; g += gridDim.x) {
        const uint64_t a = off[g] * mul, b = off[g + 1] * mul;
        uint32_t mx = 0;
        for (uint64_t i = a + threadIdx.x; i < b; i += 64)
            if (hit[i]) mx = pos[i] > mx ? pos[i] : mx;
#pragma unroll
        for (int d = 32; d; d >>= 1) {
            const uint32_t o = __shfl_xor(mx, d, 64);
            mx = o > mx ? o : mx;
        }
        if (threadIdx.x == 0) {
            const uint64_t span = (uint64_t)mx + 2;
            bigWords[g] = span > kNbrLdsBits ? (uint32_t)((span + 31) / 32) : 0u;
        }
    }
}

// removed[i] = a hit of i's segment lies at pos[i] - 1, pos[i] or pos[i] + 1. A block per segment: hits
// set their bit in the segment's own bitmap, then every instance tests its three bits; bits outside the
// bitmap (below 0, past the last hit + 1) are clear, so neither end reaches another read. big = 0: the
// segments whose bitmap fits LDS; big = 1: the others, bitmaps in HBM (bigBits, zeroed, at bigOff words).
__global__ void __launch_bounds__(256) k_neighbours(const uint64_t* __restrict__ off, uint32_t mul, uint64_t nSeg,
                                                    const uint32_t* __restrict__ pos, const uint8_t* __restrict__ hit,
                                                    const uint32_t* __restrict__ bigWords,
                                                    const uint64_t* __restrict__ bigOff, uint32_t* bigBits, int big,
                                                    uint8_t* __restrict__ removed) {
    __shared__ uint32_t sBits[kNbrLdsBits / 32];
    for (uint64_t g = blockIdx.x; g < nSeg; g += gridDim.x) {
        const uint32_t bw = bigWords[g];
        if ((bw != 0) != (big != 0)) continue;  // uniform over the block
        const uint64_t a = off[g] * mul, b = off[g + 1] * mul;
        uint32_t* bits = big ? bigBits + bigOff[g] : sBits;
        const uint64_t nBits = big ? (uint64_t)bw * 32 : kNbrLdsBits;
        if (!big) {
            for (uint32_t w = threadIdx.x; w < kNbrLdsBits / 32; w += blockDim.x) sBits[w] = 0;
            __syncthreads();
        }
        for (uint64_t i = a + threadIdx.x; i < b; i += blockDim.x)
            if (hit[i]) atomicOr(bits + (pos[i] >> 5), 1u << (pos[i] & 31u));
        __syncthreads();
        for (uint64_t i = a + threadIdx.x; i < b; i += blockDim.x) {
            const uint64_t p = pos[i];
            bool r = false;
#pragma unroll
            for (int d = -1; d <= 1; d++) {
                const uint64_t x = p + (uint64_t)(int64_t)d;  // p = 0, d = -1 wraps past nBits: clear
                if (x < nBits) {
                    const uint32_t w = big ? __hip_atomic_load(bits + (x >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                           : bits[x >> 5];
                    r = r || ((w >> (x & 31u)) & 1u);
                }
            }
            removed[i] = r;
        }
        __syncthreads();  // the next segment clears the bitmap
    }
}

// out[0] non-sentinel slots, out[1] hits, out[2] removed non-sentinel slots (keys null: no sentinels)
__global__ void __launch_bounds__(256) k_filter_counts(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ hit,
                                                       const uint8_t* __restrict__ removed, uint64_t n,
                                                       unsigned long long* __restrict__ out) {
    unsigned long long c[3] = {0, 0, 0};
    MTB_GRID_STRIDE(i, n) {
        const bool real = !keys || keys[i] != kSentinel;
        c[0] += real;
        c[1] += real && hit[i];
        c[2] += real && removed[i];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int d = 32; d; d >>= 1) c[k] += __shfl_xor(c[k], d, 64);
        if ((threadIdx.x & 63) == 0 && c[k]) atomicAdd(out + k, c[k]);
    }
}
__global__ void k_flag_unfiltered(const uint64_t* __restrict__ keys, const uint8_t* __restrict__ removed, uint64_t n,
                                  uint32_t* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) flag[i] = keys[i] != kSentinel && !removed[i];
}

// the sorted instances: flag the first of each (value, read)
__global__ void k_flag_distinct(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ids, uint64_t n,
                                uint32_t* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) flag[i] = i == 0 || keys[i] != keys[i - 1] || ids[i] != ids[i - 1];
}
__global__ void k_compact_distinct(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ ids,
                                   const uint32_t* __restrict__ flag, const uint64_t* __restrict__ off, uint64_t n,
                                   uint64_t* __restrict__ dKeys, uint32_t* __restrict__ dIds) {
    MTB_GRID_STRIDE(i, n)
        if (flag[i]) { dKeys[off[i]] = keys[i]; dIds[off[i]] = ids[i]; }
}
__global__ void k_flag_heads(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) flag[i] = i == 0 || keys[i] != keys[i - 1];
}
// positions of the flagged items: pos[off[i]] = i, pos[total] = n
__global__ void k_head_pos(const uint32_t* __restrict__ flag, const uint64_t* __restrict__ off, uint64_t n,
                           uint64_t* __restrict__ pos) {
    MTB_GRID_STRIDE(i, n + 1) {
        if (i == n) pos[off[n]] = n;
        else if (flag[i]) pos[off[i]] = i;
    }
}

__device__ __forceinline__ uint32_t hist_bucket(uint64_t m) {  // mHistBucket: floor(log2 m)
    return m ? 63u - (uint32_t)__clzll((long long)m) : 0u;
}

// runs (distinct values): m = reads of the run. Histograms of the runs with m >= 2 by log2 bucket (k-mers
// and C(m, 2)): LDS counts per block, then one atomic per non-empty bucket per block.
__global__ void __launch_bounds__(256) k_run_hist(const uint64_t* __restrict__ runStart, uint64_t nRuns,
                                                  unsigned long long* __restrict__ histK,
                                                  unsigned long long* __restrict__ histP) {
    __shared__ unsigned long long sK[64], sP[64];
    if (threadIdx.x < 64) { sK[threadIdx.x] = 0; sP[threadIdx.x] = 0; }
    __syncthreads();
    MTB_GRID_STRIDE(r, nRuns) {
        const uint64_t m = runStart[r + 1] - runStart[r];
        if (m >= 2) {
            const uint32_t b = hist_bucket(m);
            atomicAdd(&sK[b], 1ull);
            atomicAdd(&sP[b], (unsigned long long)(m * (m - 1) / 2));
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        if (sK[threadIdx.x]) atomicAdd(&histK[threadIdx.x], sK[threadIdx.x]);
        if (sP[threadIdx.x]) atomicAdd(&histP[threadIdx.x], sP[threadIdx.x]);
    }
}

// pairs[r] = C(m, 2) of a kept run, 0 of a run with m < 2 or over the cap (skip[r] = 1); maxPairs: the
// largest kept clique
__global__ void __launch_bounds__(256) k_run_pairs(const uint64_t* __restrict__ runStart, uint64_t nRuns, uint64_t cap,
                                                   uint64_t* __restrict__ pairs, uint32_t* __restrict__ skip,
                                                   unsigned long long* __restrict__ maxPairs) {
    unsigned long long mx = 0;
    MTB_GRID_STRIDE(r, nRuns) {
        const uint64_t m = runStart[r + 1] - runStart[r];
        const bool sk = m >= 2 && cap > 0 && m > cap;
        const uint64_t p = (m >= 2 && !sk) ? m * (m - 1) / 2 : 0;
        pairs[r] = p;
        skip[r] = sk;
        mx = p > mx ? p : mx;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const unsigned long long o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(maxPairs, mx);
}

__global__ void k_compact_skipped(const uint64_t* __restrict__ runStart, const uint64_t* __restrict__ dKeys,
                                  const uint32_t* __restrict__ skip, const uint64_t* __restrict__ off, uint64_t nRuns,
                                  uint64_t* __restrict__ values, uint32_t* __restrict__ ms) {
    MTB_GRID_STRIDE(r, nRuns)
        if (skip[r]) {
            values[off[r]] = dKeys[runStart[r]];
            const uint64_t m = runStart[r + 1] - runStart[r];
            ms[off[r]] = (uint32_t)(m > 0xFFFFFFFFull ? 0xFFFFFFFFull : m);
        }
}

// the last run r1 >= r0 with pairOff[r1] - pairOff[r0] <= budget (one thread: a binary search)
__global__ void k_round_end(const uint64_t* __restrict__ pairOff, uint64_t nRuns, uint64_t r0, uint64_t budget,
                            uint64_t* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t lim = pairOff[r0] + budget;
    uint64_t lo = r0, hi = nRuns;  // pairOff[lo] <= lim always
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (pairOff[mid] <= lim) lo = mid; else hi = mid - 1;
    }
    out[0] = lo;
    out[1] = pairOff[lo] - pairOff[r0];
}

// One thread per output pair of the round's runs [r0, r1): its run by binary search over the scan, then
// (i, j), i < j, un-ranked in the run's triangle (pair k = j (j - 1) / 2 + i). A run of m = 1000 reads is
// 499,500 threads' worth of work, spread like any other. key = id1 << nb | id2 (nb = bits of N).
__global__ void __launch_bounds__(256) k_emit_pairs(const uint64_t* __restrict__ pairOff, uint64_t r0, uint64_t r1,
                                                    const uint64_t* __restrict__ runStart,
                                                    const uint32_t* __restrict__ dIds, uint64_t nPairs, int nb,
                                                    uint64_t* __restrict__ keys) {
    const uint64_t base = pairOff[r0];
    MTB_GRID_STRIDE(t, nPairs) {
        const uint64_t g = base + t;
        uint64_t lo = r0, hi = r1 - 1;  // the last run with pairOff[run] <= g
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (pairOff[mid] <= g) lo = mid; else hi = mid - 1;
        }
        const uint64_t k = g - pairOff[lo];
        uint64_t j = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
        while (j * (j - 1) / 2 > k) j--;
        while ((j + 1) * j / 2 <= k) j++;
        const uint64_t i = k - j * (j - 1) / 2;
        const uint64_t s = runStart[lo];
        keys[t] = (uint64_t)dIds[s + i] << nb | dIds[s + j];
    }
}

// (pair, count) per run of equal sorted keys; cnt (nullable): per-item counts to sum instead of 1 each
__global__ void k_reduce_runs(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cnt,
                              const uint64_t* __restrict__ pos, uint64_t nHeads, uint64_t* __restrict__ outKeys,
                              uint32_t* __restrict__ outCnt) {
    MTB_GRID_STRIDE(h, nHeads) {
        const uint64_t a = pos[h], b = pos[h + 1];
        uint64_t sum = b - a;
        if (cnt) {  // a pair has at most one partial per round
            sum = 0;
            for (uint64_t i = a; i < b; i++) sum += cnt[i];
        }
        outKeys[h] = keys[a];
        outCnt[h] = (uint32_t)(sum > 0xFFFFFFFFull ? 0xFFFFFFFFull : sum);
    }
}

// Relation records: weight clamped to 65535 once (every term is positive, so this equals addSat16 per addition)
__global__ void k_make_relations(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ cnt, uint64_t n, int nb,
                                 mtb_relation* __restrict__ out) {
    MTB_GRID_STRIDE(i, n) {
        mtb_relation r;
        r.id1 = (uint32_t)(keys[i] >> nb);
        r.id2 = (uint32_t)(keys[i] & ((1ull << nb) - 1));
        r.weight = (uint16_t)(cnt[i] > 65535u ? 65535u : cnt[i]);
        r.pad = 0;
        out[i] = r;
    }
}

}  // namespace mtb

namespace {

// A device array that grows by reallocation (the resident k-mers and partial edge lists)
struct DVec {
    void* p = nullptr;
    uint64_t cap = 0;  // elements
    size_t elem;
    explicit DVec(size_t e) : elem(e) {}
    DVec(const DVec&) = delete;
    DVec& operator=(const DVec&) = delete;
    ~DVec() { if (p) hipFree(p); }
    // room for `need` elements, keeping the first `keep`
    hipError_t reserve(uint64_t need, uint64_t keep) {
        if (need <= cap) return hipSuccess;
        const uint64_t c = std::max<uint64_t>(need, cap + cap / 2) + 64;
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, c * elem);
        if (e != hipSuccess) return e;
        if (keep) e = hipMemcpy(q, p, keep * elem, hipMemcpyDeviceToDevice);
        if (p) hipFree(p);
        p = q;
        cap = c;
        return e;
    }
    void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
    template <typename T>
    T* as() const { return (T*)p; }
};

// an allocation of the edge build: out of memory names the bytes it needed
#define GRP_ALLOC(buf, bytes)                                                                              \
    do {                                                                                                   \
        const size_t b_ = (bytes);                                                                         \
        hipError_t e_ = (buf).alloc(b_);                                                                   \
        if (e_ != hipSuccess) {                                                                            \
            (void)hipGetLastError();                                                                       \
            set_error("the edge build does not fit the device: " + std::to_string(b_) + " bytes needed for " #buf); \
            return e_ == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                                  \
        }                                                                                                  \
    } while (0)

// capFromQuantile (GroupGenerator.h:611-636), restated
uint64_t cap_from_quantile(const uint64_t* hist, float quantile) {
    if (!(quantile > 0.0f) || !(quantile < 1.0f)) return 0;
    uint64_t total = 0;
    for (int b = 0; b < 64; b++) total += hist[b];
    if (total == 0) return 0;
    const double target = static_cast<double>(total) * static_cast<double>(quantile);
    uint64_t cumulative = 0;
    for (int b = 0; b < 64; b++) {
        cumulative += hist[b];
        if (static_cast<double>(cumulative) >= target) return b + 1 >= 63 ? 0 : (1ull << (b + 1)) - 1;
    }
    return 0;
}

}  // namespace

struct mtb_grouper {
    mtb_group_params par;
    int device = 0;
    HostTables tables;
    uint64_t reads = 0, kmers = 0;
    DVec keys{8}, ids{4};          // the run's k-mer instances, in emission order until build_edges sorts them
    Buf keysB, idsB;               // the sort's other side (held during the sort only)
    bool built = false;
    Buf edges;                     // mtb_relation[nEdges], (id1, id2) ascending
    uint64_t nEdges = 0;
    std::vector<uint64_t> skipValues;
    std::vector<uint32_t> skipM;
    mtb_group_stats stats;
    // the common-k-mer set (hasSet) and the kept instances' positions, held until the edges are built
    bool hasSet = false, started = false;
    DVec setVals{8}, pos{4};
    Buf setMid, setTop;
    SetIndex setIx{};
    mtb_group_filter_stats fst;
    mtb_grouper() : tables(make_tables()) {
        memset(&stats, 0, sizeof(stats));
        memset(&fst, 0, sizeof(fst));
    }
    const uint64_t* sortedKeys() const { return keys.as<uint64_t>(); }
    const uint32_t* sortedIds() const { return ids.as<uint32_t>(); }
};

namespace {

struct EvPair {  // two events around a stage, destroyed on every return path
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t create() {
        hipError_t e = hipEventCreate(&a);
        return e == hipSuccess ? hipEventCreate(&b) : e;
    }
    ~EvPair() { if (a) hipEventDestroy(a); if (b) hipEventDestroy(b); }
};

#define GRP_SET_OOM(e_, bytes_)                                                                                 \
    do {                                                                                                        \
        (void)hipGetLastError();                                                                                \
        set_error("the common k-mer set does not fit the device: " + std::to_string(bytes_) + " bytes needed"); \
        return (e_) == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                                         \
    } while (0)

// The distinct values of n ascending device values (prev: the value before them, when hasPrev) appended
// to set at nSet. flag: n u32, off: n + 1 u64, tmp: scan_tmp_elems(n) u64, dDesc: a zeroed device word.
int append_distinct(DVec& set, uint64_t& nSet, const uint64_t* vals, uint64_t n, bool hasPrev, uint64_t prev,
                    uint32_t* flag, uint64_t* off, void* tmp, int* dDesc, bool* descending) {
    if (!n) return MTB_OK;
    k_set_flag<<<stride_grid(n), 256>>>(vals, n, hasPrev, prev, flag, dDesc);
    exclusive_scan_u32(flag, n, off, tmp, nullptr);
    uint64_t add = 0;
    int desc = 0;
    GRP_TRY(hipMemcpy(&add, off + n, 8, hipMemcpyDeviceToHost));
    GRP_TRY(hipMemcpy(&desc, dDesc, 4, hipMemcpyDeviceToHost));
    if (desc) { *descending = true; return MTB_OK; }
    const hipError_t e = set.reserve(nSet + add, nSet);
    if (e != hipSuccess) GRP_SET_OOM(e, (nSet + add) * 8);
    k_compact_u64<<<stride_grid(n), 256>>>(vals, flag, off, n, set.as<uint64_t>() + nSet);
    GRP_TRY(hipGetLastError());
    nSet += add;
    return MTB_OK;
}

// the two sampled levels over nSet distinct values
int build_set_index(SetIndex& ix, const uint64_t* set, uint64_t nSet, Buf& mid, Buf& top) {
    ix = SetIndex{};
    ix.set = set;
    ix.n = nSet;
    if (!nSet) return MTB_OK;
    ix.nMid = (nSet + kSetLeaf - 1) / kSetLeaf;
    ix.T = (ix.nMid + kSetTop - 1) / kSetTop;
    ix.nTop = (uint32_t)((ix.nMid + ix.T - 1) / ix.T);
    hipError_t e = mid.alloc(8 * ix.nMid);
    if (e == hipSuccess) e = top.alloc(8 * (uint64_t)ix.nTop);
    if (e != hipSuccess) GRP_SET_OOM(e, 8 * (ix.nMid + ix.nTop));
    k_set_sample<<<stride_grid(ix.nMid), 256>>>(set, kSetLeaf, ix.nMid, mid.as<uint64_t>());
    k_set_sample<<<stride_grid(ix.nTop), 256>>>(mid.as<uint64_t>(), ix.T, ix.nTop, top.as<uint64_t>());
    GRP_TRY(hipGetLastError());
    ix.mid = mid.as<uint64_t>();
    ix.top = top.as<uint64_t>();
    return MTB_OK;
}

// hit and removed (n bytes each) of n instances in nSeg segments (segment g: [off[g] * mul, off[g + 1] * mul));
// ms (nullable): [0] += membership, [1] += neighbourhood
int run_filter(const SetIndex& ix, const uint64_t* keys, int skipSentinel, const uint32_t* pos, const uint64_t* off,
               uint32_t mul, uint64_t nSeg, uint64_t n, uint8_t* hit, uint8_t* removed, float* ms) {
    if (!n) return MTB_OK;
    EvPair m, nb;
    GRP_TRY(m.create());
    GRP_TRY(nb.create());
    GRP_TRY(hipEventRecord(m.a, nullptr));
    if (ix.n) k_set_member<<<std::min(stride_grid(n), 2048u), 256>>>(ix, keys, n, skipSentinel, hit);
    else GRP_TRY(hipMemsetAsync(hit, 0, n, nullptr));
    GRP_TRY(hipEventRecord(m.b, nullptr));
    GRP_TRY(hipEventRecord(nb.a, nullptr));
    Buf bigWords, bigOff, tmp, bigBits;
    if (ix.n && nSeg) {
        GRP_TRY(bigWords.alloc(4 * nSeg));
        GRP_TRY(bigOff.alloc(8 * (nSeg + 1)));
        GRP_TRY(tmp.alloc(8 * scan_tmp_elems(nSeg)));
        const unsigned grid = (unsigned)std::min<uint64_t>(nSeg, 1u << 20);
        k_seg_span<<<grid, 64>>>(off, mul, nSeg, pos, hit, bigWords.as<uint32_t>());
        exclusive_scan_u32(bigWords.as<uint32_t>(), nSeg, bigOff.as<uint64_t>(), tmp.p, nullptr);
        uint64_t words = 0;
        GRP_TRY(hipMemcpy(&words, bigOff.as<uint64_t>() + nSeg, 8, hipMemcpyDeviceToHost));
        k_neighbours<<<grid, 64>>>(off, mul, nSeg, pos, hit, bigWords.as<uint32_t>(), bigOff.as<uint64_t>(), nullptr, 0,
                                   removed);
        if (words) {  // reads whose hits reach past the on-chip bitmap: theirs in HBM
            const hipError_t e = bigBits.alloc(4 * words);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_error("the filter's position bitmaps do not fit the device: " + std::to_string(4 * words) + " bytes needed");
                return e == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;
            }
            GRP_TRY(hipMemsetAsync(bigBits.p, 0, 4 * words, nullptr));
            k_neighbours<<<(unsigned)std::min<uint64_t>(nSeg, 4096), 256>>>(off, mul, nSeg, pos, hit, bigWords.as<uint32_t>(),
                                                                          bigOff.as<uint64_t>(), bigBits.as<uint32_t>(), 1,
                                                                          removed);
        }
    } else {
        GRP_TRY(hipMemsetAsync(removed, 0, n, nullptr));
    }
    GRP_TRY(hipGetLastError());
    GRP_TRY(hipEventRecord(nb.b, nullptr));
    GRP_TRY(hipDeviceSynchronize());
    if (ms) {
        float t = 0;
        GRP_TRY(hipEventElapsedTime(&t, m.a, m.b));
        ms[0] += t;
        GRP_TRY(hipEventElapsedTime(&t, nb.a, nb.b));
        ms[1] += t;
    }
    return MTB_OK;
}

int attachable(mtb_grouper* g) {
    if (!g) { set_error("null argument"); return MTB_ERR_ARG; }
    if (g->hasSet) { set_error("a common k-mer set is attached already"); return MTB_ERR_ARG; }
    if (g->started) { set_error("the common k-mer set must be attached before the first batch"); return MTB_ERR_ARG; }
    return MTB_OK;
}

// groupGeneration.cpp:101-130: all three keys compared, a key the file lacks reads as -1
int check_kmer_params(mtb_grouper* g, const std::string& dir, int* checked) {
    *checked = 0;
    FILE* f = fopen((dir + "/kmer_params").c_str(), "r");
    if (!f) return MTB_OK;
    int dbSyncmer = -1, dbSmerLen = -1, dbKmerFormat = -1, value = 0;
    char key[64];
    while (fscanf(f, "%63s %d", key, &value) == 2) {
        if (!strcmp(key, "syncmer")) dbSyncmer = value;
        else if (!strcmp(key, "smer_len")) dbSmerLen = value;
        else if (!strcmp(key, "kmer_format")) dbKmerFormat = value;
    }
    fclose(f);
    const int syncmer = g->par.syncmer, smerLen = g->par.smer_len, kmerFormat = g->par.syncmer ? 5 : 3;
    if (dbSyncmer != syncmer || dbSmerLen != smerLen || dbKmerFormat != kmerFormat) {
        set_error("k-mer settings do not match the common k-mer DB at " + dir + ": DB syncmer " + std::to_string(dbSyncmer) +
                  " smer_len " + std::to_string(dbSmerLen) + " kmer_format " + std::to_string(dbKmerFormat) +
                  ", request syncmer " + std::to_string(syncmer) + " smer_len " + std::to_string(smerLen) +
                  " kmer_format " + std::to_string(kmerFormat));
        return MTB_ERR_ARG;
    }
    *checked = 1;
    return MTB_OK;
}

// after the set's values are in g->setVals (n of them): index, flags, stats
int finish_set(mtb_grouper* g, uint64_t nSet, const EvPair& ev) {
    if (const int rc = build_set_index(g->setIx, g->setVals.as<uint64_t>(), nSet, g->setMid, g->setTop)) return rc;
    GRP_TRY(hipEventRecord(ev.b, nullptr));
    GRP_TRY(hipDeviceSynchronize());
    float t = 0;
    GRP_TRY(hipEventElapsedTime(&t, ev.a, ev.b));
    g->fst.ms[0] += t;
    g->fst.db_values = nSet;
    g->hasSet = true;
    return MTB_OK;
}

// sorted (key, count-or-nothing) items -> one (key, sum) per distinct key, appended to outK / outC at outN
int reduce_sorted(const uint64_t* keys, const uint32_t* cnt, uint64_t n, DVec& outK, DVec& outC, uint64_t& outN,
                  Buf& flag, Buf& off, Buf& pos, void* scanTmp) {
    if (!n) return MTB_OK;
    k_flag_heads<<<stride_grid(n), 256>>>(keys, n, flag.as<uint32_t>());
    exclusive_scan_u32(flag.as<uint32_t>(), n, off.as<uint64_t>(), scanTmp, nullptr);
    uint64_t heads = 0;
    GRP_TRY(hipMemcpy(&heads, off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
    k_head_pos<<<stride_grid(n + 1), 256>>>(flag.as<uint32_t>(), off.as<uint64_t>(), n, pos.as<uint64_t>());
    hipError_t e = outK.reserve(outN + heads, outN);
    if (e == hipSuccess) e = outC.reserve(outN + heads, outN);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("the edge list does not fit the device: " + std::to_string((outN + heads) * 12) + " bytes needed");
        return e == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;
    }
    k_reduce_runs<<<stride_grid(heads), 256>>>(keys, cnt, pos.as<uint64_t>(), heads, outK.as<uint64_t>() + outN,
                                               outC.as<uint32_t>() + outN);
    GRP_TRY(hipGetLastError());
    outN += heads;
    return MTB_OK;
}

int build_edges_impl(mtb_grouper* g, uint64_t pairBudget) {
    mtb_group_stats& st = g->stats;
    memset(&st, 0, sizeof(st));
    st.reads = g->reads;
    st.kmers = g->kmers;
    g->nEdges = 0;
    g->skipValues.clear();
    g->skipM.clear();
    const uint64_t n = g->kmers;
    const int nb = bits_of(g->reads);
    hipEvent_t ev[5];
    for (auto& e : ev) GRP_TRY(hipEventCreate(&e));
    struct EvGuard { hipEvent_t* e; ~EvGuard() { for (int i = 0; i < 5; i++) hipEventDestroy(e[i]); } } guard{ev};
    GRP_TRY(hipEventRecord(ev[0], nullptr));
    if (!n) { g->built = true; return MTB_OK; }

    // 1. sort the instances by value (60 bits), stable: IDs stay ascending within a value
    Buf cnt, offs, tmp;
    {
        const uint64_t rc = radix_counts_elems(n + 1);
        GRP_ALLOC(g->keysB, 8 * (n + 1));
        GRP_ALLOC(g->idsB, 4 * (n + 1));
        GRP_ALLOC(cnt, 4 * rc);
        GRP_ALLOC(offs, 8 * (rc + 1));
        GRP_ALLOC(tmp, 8 * scan_tmp_elems(rc + n + 2));
        bool inB = false;
        radix_sort_pairs<uint32_t>(g->keys.as<uint64_t>(), g->ids.as<uint32_t>(), g->keysB.as<uint64_t>(),
                                   g->idsB.as<uint32_t>(), n, 0, 60, false, false, cnt.as<uint32_t>(),
                                   offs.as<uint64_t>(), tmp.p, &inB, nullptr);
        GRP_TRY(hipGetLastError());
        // 8 passes end on the first side; were it ever the other, bring the result back, so that the
        // resident arrays stay the instances whatever happens next (an error below, a second build)
        if (inB) {
            GRP_TRY(hipMemcpy(g->keys.p, g->keysB.p, 8 * n, hipMemcpyDeviceToDevice));
            GRP_TRY(hipMemcpy(g->ids.p, g->idsB.p, 4 * n, hipMemcpyDeviceToDevice));
        }
        g->keysB.alloc(0);
        g->idsB.alloc(0);
    }
    GRP_TRY(hipEventRecord(ev[1], nullptr));

    // 2. run pass: distinct (value, read) instances, run heads, m per run, histograms, cap, C(m, 2) scan
    Buf flag, off, dKeys, dIds, runStart, pairs, pairOff, skip, small;
    GRP_ALLOC(flag, 4 * (n + 1));
    GRP_ALLOC(off, 8 * (n + 2));
    k_flag_distinct<<<stride_grid(n), 256>>>(g->sortedKeys(), g->sortedIds(), n, flag.as<uint32_t>());
    exclusive_scan_u32(flag.as<uint32_t>(), n, off.as<uint64_t>(), tmp.p, nullptr);
    uint64_t nd = 0;
    GRP_TRY(hipMemcpy(&nd, off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
    GRP_ALLOC(dKeys, 8 * nd);
    GRP_ALLOC(dIds, 4 * nd);
    k_compact_distinct<<<stride_grid(n), 256>>>(g->sortedKeys(), g->sortedIds(), flag.as<uint32_t>(), off.as<uint64_t>(), n,
                                                dKeys.as<uint64_t>(), dIds.as<uint32_t>());
    k_flag_heads<<<stride_grid(nd), 256>>>(dKeys.as<uint64_t>(), nd, flag.as<uint32_t>());
    exclusive_scan_u32(flag.as<uint32_t>(), nd, off.as<uint64_t>(), tmp.p, nullptr);
    uint64_t nRuns = 0;
    GRP_TRY(hipMemcpy(&nRuns, off.as<uint64_t>() + nd, 8, hipMemcpyDeviceToHost));
    GRP_ALLOC(runStart, 8 * (nRuns + 1));
    k_head_pos<<<stride_grid(nd + 1), 256>>>(flag.as<uint32_t>(), off.as<uint64_t>(), nd, runStart.as<uint64_t>());
    st.distinct_kmers = nRuns;
    GRP_ALLOC(small, 8 * (64 + 64 + 4));  // the two histograms, the largest kept clique, the round's end
    unsigned long long* histK = small.as<unsigned long long>();
    unsigned long long* histP = histK + 64;
    unsigned long long* maxPairs = histK + 128;
    uint64_t* roundOut = reinterpret_cast<uint64_t*>(histK + 130);
    GRP_TRY(hipMemset(small.p, 0, 8 * (64 + 64 + 4)));
    k_run_hist<<<std::min(stride_grid(nRuns), 1024u), 256>>>(runStart.as<uint64_t>(), nRuns, histK, histP);
    GRP_TRY(hipMemcpy(st.hist_kmers, histK, 8 * 64, hipMemcpyDeviceToHost));
    GRP_TRY(hipMemcpy(st.hist_pairs, histP, 8 * 64, hipMemcpyDeviceToHost));
    // absThr (GroupGenerator.cpp:649-701): the explicit cap wins, else the quantile's, else off
    const uint64_t cap = g->par.max_kmer_reads > 0 ? (uint64_t)g->par.max_kmer_reads
                                                   : cap_from_quantile(st.hist_kmers, g->par.max_kmer_quantile);
    st.cap = cap;
    GRP_ALLOC(pairs, 8 * (nRuns + 1));
    GRP_ALLOC(pairOff, 8 * (nRuns + 2));
    GRP_ALLOC(skip, 4 * (nRuns + 1));
    k_run_pairs<<<stride_grid(nRuns), 256>>>(runStart.as<uint64_t>(), nRuns, cap, pairs.as<uint64_t>(), skip.as<uint32_t>(),
                                             maxPairs);
    exclusive_scan_u64(pairs.as<uint64_t>(), nRuns, pairOff.as<uint64_t>(), tmp.p, nullptr);
    uint64_t totalPairs = 0, maxClique = 0;
    GRP_TRY(hipMemcpy(&totalPairs, pairOff.as<uint64_t>() + nRuns, 8, hipMemcpyDeviceToHost));
    GRP_TRY(hipMemcpy(&maxClique, maxPairs, 8, hipMemcpyDeviceToHost));
    st.kept_pair_occurrences = totalPairs;
    {  // the skipped runs (value, m), ascending value
        exclusive_scan_u32(skip.as<uint32_t>(), nRuns, off.as<uint64_t>(), tmp.p, nullptr);
        uint64_t ns = 0;
        GRP_TRY(hipMemcpy(&ns, off.as<uint64_t>() + nRuns, 8, hipMemcpyDeviceToHost));
        st.skipped_kmers = ns;
        if (ns) {
            Buf sv, sm;
            GRP_ALLOC(sv, 8 * ns);
            GRP_ALLOC(sm, 4 * ns);
            k_compact_skipped<<<stride_grid(nRuns), 256>>>(runStart.as<uint64_t>(), dKeys.as<uint64_t>(), skip.as<uint32_t>(),
                                                           off.as<uint64_t>(), nRuns, sv.as<uint64_t>(), sm.as<uint32_t>());
            g->skipValues.resize(ns);
            g->skipM.resize(ns);
            GRP_TRY(hipMemcpy(g->skipValues.data(), sv.p, 8 * ns, hipMemcpyDeviceToHost));
            GRP_TRY(hipMemcpy(g->skipM.data(), sm.p, 4 * ns, hipMemcpyDeviceToHost));
        }
    }
    GRP_TRY(hipGetLastError());
    GRP_TRY(hipEventRecord(ev[2], nullptr));
    // the sort's and the run pass's per-instance scratch is done with
    flag.alloc(0); off.alloc(0); skip.alloc(0); pairs.alloc(0);

    // 3. pair emission in rounds of at most `budget` pairs
    uint64_t budget = pairBudget;
    if (!budget) {  // from free HBM: a pair in flight costs its two key and value sides, flags, offsets and positions
        size_t freeB = 0, totalB = 0;
        GRP_TRY(hipMemGetInfo(&freeB, &totalB));
        budget = std::max<uint64_t>(freeB / 2 / 48, 1u << 20);
    }
    if (budget < maxClique) {
        set_error("pair_budget " + std::to_string(budget) + " is below the largest kept clique (" + std::to_string(maxClique) + " pairs)");
        return MTB_ERR_ARG;
    }
    const uint64_t roundCap = std::min(budget, totalPairs);
    DVec partK(8), partC(4);
    uint64_t nPart = 0, rounds = 0;
    if (totalPairs) {
        Buf pk, pv, pkB, pvB, pflag, poff, ppos, pcnt, poffs, ptmp;
        const uint64_t rc = radix_counts_elems(roundCap + 1);
        GRP_ALLOC(pk, 8 * (roundCap + 1));
        GRP_ALLOC(pv, 4 * (roundCap + 1));
        GRP_ALLOC(pkB, 8 * (roundCap + 1));
        GRP_ALLOC(pvB, 4 * (roundCap + 1));
        GRP_ALLOC(pflag, 4 * (roundCap + 1));
        GRP_ALLOC(poff, 8 * (roundCap + 2));
        GRP_ALLOC(ppos, 8 * (roundCap + 2));
        GRP_ALLOC(pcnt, 4 * rc);
        GRP_ALLOC(poffs, 8 * (rc + 1));
        GRP_ALLOC(ptmp, 8 * scan_tmp_elems(rc + roundCap + 2));
        GRP_TRY(hipMemset(pv.p, 0, 4 * (roundCap + 1)));  // the sort carries values; a round's pairs need none
        uint64_t r0 = 0;
        while (r0 < nRuns) {
            k_round_end<<<1, 64>>>(pairOff.as<uint64_t>(), nRuns, r0, budget, roundOut);
            uint64_t ro[2];
            GRP_TRY(hipMemcpy(ro, roundOut, 16, hipMemcpyDeviceToHost));
            const uint64_t r1 = ro[0], np = ro[1];
            if (r1 <= r0 || np > roundCap) { set_error("round search made no progress"); return MTB_ERR_INTERNAL; }
            if (np) {
                k_emit_pairs<<<stride_grid(np), 256>>>(pairOff.as<uint64_t>(), r0, r1, runStart.as<uint64_t>(), dIds.as<uint32_t>(),
                                                       np, nb, pk.as<uint64_t>());
                bool inB = false;
                radix_sort_pairs<uint32_t>(pk.as<uint64_t>(), pv.as<uint32_t>(), pkB.as<uint64_t>(), pvB.as<uint32_t>(), np, 0,
                                           2 * nb, false, false, pcnt.as<uint32_t>(), poffs.as<uint64_t>(), ptmp.p, &inB,
                                           nullptr);
                GRP_TRY(hipGetLastError());
                if (const int rcode = reduce_sorted(inB ? pkB.as<uint64_t>() : pk.as<uint64_t>(), nullptr, np, partK, partC,
                                                    nPart, pflag, poff, ppos, ptmp.p))
                    return rcode;
                rounds++;
            }
            r0 = r1;
        }
    }
    st.rounds = rounds;
    GRP_TRY(hipEventRecord(ev[3], nullptr));

    // 4. more than one round: a pair may have a partial count per round — sort the concatenation, sum per pair
    DVec finK(8), finC(4);
    uint64_t nFin = 0;
    const uint64_t* eK = partK.as<uint64_t>();
    const uint32_t* eC = partC.as<uint32_t>();
    uint64_t nE = nPart;
    if (rounds > 1) {
        Buf kB, cB, mflag, moff, mpos, mcnt, moffs, mtmp;
        const uint64_t rc = radix_counts_elems(nPart + 1);
        GRP_ALLOC(kB, 8 * (nPart + 1));
        GRP_ALLOC(cB, 4 * (nPart + 1));
        GRP_ALLOC(mflag, 4 * (nPart + 1));
        GRP_ALLOC(moff, 8 * (nPart + 2));
        GRP_ALLOC(mpos, 8 * (nPart + 2));
        GRP_ALLOC(mcnt, 4 * rc);
        GRP_ALLOC(moffs, 8 * (rc + 1));
        GRP_ALLOC(mtmp, 8 * scan_tmp_elems(rc + nPart + 2));
        bool inB = false;
        radix_sort_pairs<uint32_t>(partK.as<uint64_t>(), partC.as<uint32_t>(), kB.as<uint64_t>(), cB.as<uint32_t>(), nPart, 0,
                                   2 * nb, false, false, mcnt.as<uint32_t>(), moffs.as<uint64_t>(), mtmp.p, &inB, nullptr);
        GRP_TRY(hipGetLastError());
        if (const int rcode = reduce_sorted(inB ? kB.as<uint64_t>() : partK.as<uint64_t>(),
                                            inB ? cB.as<uint32_t>() : partC.as<uint32_t>(), nPart, finK, finC, nFin, mflag,
                                            moff, mpos, mtmp.p))
            return rcode;
        GRP_TRY(hipDeviceSynchronize());
        eK = finK.as<uint64_t>();
        eC = finC.as<uint32_t>();
        nE = nFin;
    }
    GRP_ALLOC(g->edges, sizeof(mtb_relation) * nE);
    if (nE) k_make_relations<<<stride_grid(nE), 256>>>(eK, eC, nE, nb, g->edges.as<mtb_relation>());
    GRP_TRY(hipGetLastError());
    GRP_TRY(hipEventRecord(ev[4], nullptr));
    GRP_TRY(hipDeviceSynchronize());
    g->nEdges = nE;
    st.edges = nE;
    for (int i = 0; i < 4; i++) GRP_TRY(hipEventElapsedTime(&st.ms[1 + i], ev[i], ev[i + 1]));
    g->built = true;
    return MTB_OK;
}

}  // namespace

extern "C" int mtb_group_open(const mtb_group_params* par, int device, mtb_grouper** out) {
    if (!out) { set_error("null argument"); return MTB_ERR_ARG; }
    *out = nullptr;
    if (const int rc = check_params(par)) return rc;
    if (par->seq_mode < 1 || par->seq_mode > 3) { set_error("seq_mode must be 1, 2 or 3"); return MTB_ERR_ARG; }
    if (par->syncmer && (par->smer_len < 5 || par->smer_len > kGroupK)) {
        set_error("smer_len must be in [5, 12] (at most 8 s-mers per 12-mer)");
        return MTB_ERR_ARG;
    }
    GRP_TRY(hipSetDevice(device));
    mtb_grouper* g = new mtb_grouper();
    g->par = *par;
    g->device = device;
    *out = g;
    return MTB_OK;
}

extern "C" void mtb_group_close(mtb_grouper* g) {
    if (!g) return;
    hipSetDevice(g->device);
    delete g;
}

extern "C" int mtb_group_add_batch(mtb_grouper* g, const char* seq, const uint64_t* off, const char* seq2,
                                   const uint64_t* off2, uint32_t n_reads, uint32_t flags) {
    if (!g || (n_reads && (!seq || !off))) { set_error("null argument"); return MTB_ERR_ARG; }
    const int paired = g->par.seq_mode == 2;
    if (paired && n_reads && (!seq2 || !off2)) { set_error("seq_mode 2 needs both mates"); return MTB_ERR_ARG; }
    if (g->built) { set_error("the edges are built: no more batches"); return MTB_ERR_ARG; }
    if (g->reads + n_reads >= 0xFFFFFFFFull) { set_error("2^32 - 1 reads or more"); return MTB_ERR_ARG; }
    if (!n_reads) return MTB_OK;
    g->started = true;
    GRP_TRY(hipSetDevice(g->device));
    Buf hSeq1, hOff1, hSeq2, hOff2;
    const uint8_t* dSeq1 = (const uint8_t*)seq;
    const uint64_t* dOff1 = off;
    const uint8_t* dSeq2 = (const uint8_t*)seq2;
    const uint64_t* dOff2 = off2;
    if (!(flags & MTB_INPUT_DEVICE)) {
        GRP_TRY(hOff1.alloc(8 * ((uint64_t)n_reads + 1)));
        GRP_TRY(hSeq1.alloc(off[n_reads] + 16));
        GRP_TRY(hipMemcpy(hOff1.p, off, 8 * ((uint64_t)n_reads + 1), hipMemcpyHostToDevice));
        GRP_TRY(hipMemcpy(hSeq1.p, seq, off[n_reads], hipMemcpyHostToDevice));
        dSeq1 = hSeq1.as<uint8_t>();
        dOff1 = hOff1.as<uint64_t>();
        if (paired) {
            GRP_TRY(hOff2.alloc(8 * ((uint64_t)n_reads + 1)));
            GRP_TRY(hSeq2.alloc(off2[n_reads] + 16));
            GRP_TRY(hipMemcpy(hOff2.p, off2, 8 * ((uint64_t)n_reads + 1), hipMemcpyHostToDevice));
            GRP_TRY(hipMemcpy(hSeq2.p, seq2, off2[n_reads], hipMemcpyHostToDevice));
            dSeq2 = hSeq2.as<uint8_t>();
            dOff2 = hOff2.as<uint64_t>();
        }
    }
    hipEvent_t e0, e1;
    GRP_TRY(hipEventCreate(&e0));
    GRP_TRY(hipEventCreate(&e1));
    struct EvGuard { hipEvent_t a, b; ~EvGuard() { hipEventDestroy(a); hipEventDestroy(b); } } guard{e0, e1};
    GRP_TRY(hipEventRecord(e0, nullptr));
    // K0 read meta (lengths), then this path's own 12-mer units
    Buf meta, qlen, maxW, readLens, units, uOff, unitRead, tmp;
    GRP_TRY(meta.alloc(sizeof(ReadMeta) * (uint64_t)n_reads));
    GRP_TRY(qlen.alloc(4 * (uint64_t)n_reads));
    GRP_TRY(maxW.alloc(16));
    GRP_TRY(readLens.alloc(4 * (uint64_t)n_reads));
    GRP_TRY(units.alloc(4 * (uint64_t)n_reads));
    GRP_TRY(uOff.alloc(8 * ((uint64_t)n_reads + 1)));
    GRP_TRY(tmp.alloc(8 * scan_tmp_elems(n_reads)));
    launch_read_meta(dOff1, paired ? dOff2 : nullptr, n_reads, paired, meta.as<ReadMeta>(), qlen.as<uint32_t>(),
                     maxW.as<uint32_t>(), readLens.as<uint32_t>(), nullptr);
    k_group_units<<<stride_grid(n_reads), 256>>>(meta.as<ReadMeta>(), n_reads, paired, units.as<uint32_t>());
    exclusive_scan_u32(units.as<uint32_t>(), n_reads, uOff.as<uint64_t>(), tmp.p, nullptr);
    uint64_t nUnits = 0;
    GRP_TRY(hipMemcpy(&nUnits, uOff.as<uint64_t>() + n_reads, 8, hipMemcpyDeviceToHost));
    uint64_t kept = 0;
    if (nUnits) {
        const uint64_t slots = nUnits * kGroupChunk;
        Buf sk, si, sp, hit, removed, counts, flag, off64, tmp2;
        const bool filter = g->hasSet;
        GRP_TRY(unitRead.alloc(4 * nUnits));
        GRP_TRY(sk.alloc(8 * slots));
        GRP_TRY(si.alloc(4 * slots));
        GRP_TRY(flag.alloc(4 * slots));
        GRP_TRY(off64.alloc(8 * (slots + 1)));
        GRP_TRY(tmp2.alloc(8 * scan_tmp_elems(slots)));
        if (filter) {
            GRP_TRY(sp.alloc(4 * slots));
            GRP_TRY(hit.alloc(slots));
            GRP_TRY(removed.alloc(slots));
            GRP_TRY(counts.alloc(8 * 3));
        }
        launch_unit_read(uOff.as<uint64_t>(), n_reads, unitRead.as<uint32_t>(), nullptr);
        GroupTables tabs;
        for (int i = 0; i < 256; i++) tabs.base[i] = g->tables.base[i];
        for (int i = 0; i < 64; i++) tabs.aa[i] = g->tables.aa[i];
        k_extract_aa12<<<(unsigned)((nUnits + 255) / 256), 256>>>(dSeq1, dOff1, dSeq2, dOff2, meta.as<ReadMeta>(),
                                                                  uOff.as<uint64_t>(), unitRead.as<uint32_t>(), nUnits, paired,
                                                                  tabs, g->par.syncmer != 0, g->par.syncmer ? g->par.smer_len : 5,
                                                                  (uint32_t)g->reads, sk.as<uint64_t>(), si.as<uint32_t>(),
                                                                  filter ? sp.as<uint32_t>() : nullptr);
        EvPair evC;
        if (filter) {
            // filterCommonKmers on the batch's slots (a read's slots are contiguous: its units), then the
            // usual flag, scan and compact over what is left
            GRP_TRY(evC.create());
            if (const int rc = run_filter(g->setIx, sk.as<uint64_t>(), 1, sp.as<uint32_t>(), uOff.as<uint64_t>(), kGroupChunk,
                                          n_reads, slots, hit.as<uint8_t>(), removed.as<uint8_t>(), g->fst.ms + 1))
                return rc;
            GRP_TRY(hipEventRecord(evC.a, nullptr));
            GRP_TRY(hipMemsetAsync(counts.p, 0, 8 * 3, nullptr));
            k_filter_counts<<<std::min(stride_grid(slots), 2048u), 256>>>(sk.as<uint64_t>(), hit.as<uint8_t>(),
                                                                           removed.as<uint8_t>(), slots,
                                                                           counts.as<unsigned long long>());
            k_flag_unfiltered<<<stride_grid(slots), 256>>>(sk.as<uint64_t>(), removed.as<uint8_t>(), slots, flag.as<uint32_t>());
        } else {
            k_flag_kept<<<stride_grid(slots), 256>>>(sk.as<uint64_t>(), slots, flag.as<uint32_t>());
        }
        exclusive_scan_u32(flag.as<uint32_t>(), slots, off64.as<uint64_t>(), tmp2.p, nullptr);
        GRP_TRY(hipMemcpy(&kept, off64.as<uint64_t>() + slots, 8, hipMemcpyDeviceToHost));
        hipError_t e = g->keys.reserve(g->kmers + kept, g->kmers);
        if (e == hipSuccess) e = g->ids.reserve(g->kmers + kept, g->kmers);
        if (e == hipSuccess && filter) e = g->pos.reserve(g->kmers + kept, g->kmers);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("the k-mers do not fit the device: " + std::to_string((g->kmers + kept) * (filter ? 16 : 12)) + " bytes needed");
            return e == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;
        }
        if (filter) {
            k_compact_distinct<<<stride_grid(slots), 256>>>(sk.as<uint64_t>(), si.as<uint32_t>(), flag.as<uint32_t>(),
                                                            off64.as<uint64_t>(), slots, g->keys.as<uint64_t>() + g->kmers,
                                                            g->ids.as<uint32_t>() + g->kmers);
            k_compact_u32<<<stride_grid(slots), 256>>>(sp.as<uint32_t>(), flag.as<uint32_t>(), off64.as<uint64_t>(), slots,
                                                       g->pos.as<uint32_t>() + g->kmers);
            GRP_TRY(hipEventRecord(evC.b, nullptr));
            unsigned long long c[3];
            GRP_TRY(hipMemcpy(c, counts.p, 8 * 3, hipMemcpyDeviceToHost));
            float t = 0;
            GRP_TRY(hipEventElapsedTime(&t, evC.a, evC.b));
            g->fst.ms[3] += t;
            if (c[0] - c[2] != kept) { set_error("the filter's counts disagree with its compaction"); return MTB_ERR_INTERNAL; }
            g->fst.extracted += c[0];
            g->fst.hit += c[1];
            g->fst.removed += c[2];
            g->fst.kept += kept;
        } else {
            k_compact_kmers<<<stride_grid(slots), 256>>>(sk.as<uint64_t>(), si.as<uint32_t>(), slots, off64.as<uint64_t>(),
                                                         g->keys.as<uint64_t>() + g->kmers, g->ids.as<uint32_t>() + g->kmers);
        }
        GRP_TRY(hipGetLastError());
    }
    GRP_TRY(hipEventRecord(e1, nullptr));
    GRP_TRY(hipDeviceSynchronize());
    float ms = 0;
    GRP_TRY(hipEventElapsedTime(&ms, e0, e1));
    g->stats.ms[0] += ms;
    g->kmers += kept;
    g->reads += n_reads;
    return MTB_OK;
}

extern "C" int mtb_group_get_kmers(mtb_grouper* g, uint64_t* values, uint32_t* read_ids, uint64_t cap, uint64_t* n) {
    if (!g || !n) { set_error("null argument"); return MTB_ERR_ARG; }
    *n = g->kmers;
    if (cap < g->kmers) return MTB_RETRY;
    if (!g->kmers) return MTB_OK;
    if (!values || !read_ids) { set_error("null argument"); return MTB_ERR_ARG; }
    GRP_TRY(hipSetDevice(g->device));
    GRP_TRY(hipMemcpy(values, g->built ? g->sortedKeys() : g->keys.as<uint64_t>(), 8 * g->kmers, hipMemcpyDeviceToHost));
    GRP_TRY(hipMemcpy(read_ids, g->built ? g->sortedIds() : g->ids.as<uint32_t>(), 4 * g->kmers, hipMemcpyDeviceToHost));
    return MTB_OK;
}

extern "C" int mtb_group_build_edges(mtb_grouper* g, uint64_t pair_budget, mtb_group_stats* stats) {
    if (!g) { set_error("null argument"); return MTB_ERR_ARG; }
    GRP_TRY(hipSetDevice(g->device));
    g->built = false;  // again, e.g. with another budget: from the sorted instances (sorting them again keeps them)
    g->pos.release();  // the sort does not carry the positions
    const float extractMs = g->stats.ms[0];
    const int rc = build_edges_impl(g, pair_budget);
    g->stats.ms[0] = extractMs;
    if (stats) *stats = g->stats;
    return rc;
}

extern "C" int mtb_group_get_edges(mtb_grouper* g, mtb_relation* out, uint64_t cap, uint64_t* n) {
    if (!g || !n) { set_error("null argument"); return MTB_ERR_ARG; }
    if (!g->built) { set_error("mtb_group_build_edges first"); return MTB_ERR_ARG; }
    *n = g->nEdges;
    if (cap < g->nEdges) return MTB_RETRY;
    if (!g->nEdges) return MTB_OK;
    if (!out) { set_error("null argument"); return MTB_ERR_ARG; }
    GRP_TRY(hipSetDevice(g->device));
    GRP_TRY(hipMemcpy(out, g->edges.p, sizeof(mtb_relation) * g->nEdges, hipMemcpyDeviceToHost));
    return MTB_OK;
}

extern "C" int mtb_group_get_skipped(mtb_grouper* g, uint64_t* values, uint32_t* m, uint64_t cap, uint64_t* n) {
    if (!g || !n) { set_error("null argument"); return MTB_ERR_ARG; }
    if (!g->built) { set_error("mtb_group_build_edges first"); return MTB_ERR_ARG; }
    *n = g->skipValues.size();
    if (cap < *n) return MTB_RETRY;
    if (*n && (!values || !m)) { set_error("null argument"); return MTB_ERR_ARG; }
    if (*n) {
        memcpy(values, g->skipValues.data(), 8 * *n);
        memcpy(m, g->skipM.data(), 4 * *n);
    }
    return MTB_OK;
}

extern "C" int mtb_group_finish(mtb_grouper* g, uint32_t* group_map, mtb_group_stats* stats) {
    if (!g || !group_map) { set_error("null argument"); return MTB_ERR_ARG; }
    if (!g->built) { set_error("mtb_group_build_edges first"); return MTB_ERR_ARG; }
    int coreThr = 0, weakThr = 0;
    if (const int rc = thresholds(g->par, g->kmers, g->reads, &coreThr, &weakThr)) return rc;
    GRP_TRY(hipSetDevice(g->device));
    const uint64_t n1 = g->reads + 1;
    Buf dMaps;
    GRP_TRY(dMaps.alloc(4 * 3 * n1));
    float ms[3] = {0, 0, 0};
    if (const int rc = run_phases(g->edges.as<mtb_relation>(), g->nEdges, (uint32_t)g->reads, coreThr, weakThr,
                                  dMaps.as<uint32_t>(), ms, nullptr))
        return rc;
    std::vector<uint32_t> maps(3 * n1);
    GRP_TRY(hipMemcpy(maps.data(), dMaps.p, 4 * 3 * n1, hipMemcpyDeviceToHost));
    memcpy(group_map, maps.data() + 2 * n1, 4 * n1);
    g->stats.core_thr = coreThr;
    g->stats.weak_thr = weakThr;
    for (int p = 0; p < 3; p++) {
        count_groups(maps.data() + p * n1, (uint32_t)g->reads, &g->stats.groups_after[p], &g->stats.grouped_after[p]);
        g->stats.ms[5 + p] = ms[p];
    }
    if (stats) *stats = g->stats;
    return MTB_OK;
}

// ---- the common-k-mer filter's entry points -------------------------------------------------------
extern "C" void mtb_group_filter_constants(uint32_t out[4]) {
    if (!out) return;
    out[0] = kSetLeaf;
    out[1] = kSetTop;
    out[2] = kNbrLdsBits;
    out[3] = 0;
}

extern "C" int mtb_group_set_common_kmers(mtb_grouper* g, const uint64_t* values, uint64_t n) {
    if (const int rc = attachable(g)) return rc;
    if (n && !values) { set_error("null argument"); return MTB_ERR_ARG; }
    GRP_TRY(hipSetDevice(g->device));
    EvPair ev;
    GRP_TRY(ev.create());
    GRP_TRY(hipEventRecord(ev.a, nullptr));
    uint64_t nSet = 0;
    if (n) {
        Buf dVal, flag, off, tmp, desc;
        hipError_t e = dVal.alloc(8 * n);
        if (e == hipSuccess) e = flag.alloc(4 * n);
        if (e == hipSuccess) e = off.alloc(8 * (n + 1));
        if (e == hipSuccess) e = tmp.alloc(8 * scan_tmp_elems(n));
        if (e == hipSuccess) e = desc.alloc(4);
        if (e != hipSuccess) GRP_SET_OOM(e, n * (8 + 4 + 8 + 8));
        GRP_TRY(hipMemcpy(dVal.p, values, 8 * n, hipMemcpyHostToDevice));
        GRP_TRY(hipMemset(desc.p, 0, 4));
        bool descending = false;
        if (const int rc = append_distinct(g->setVals, nSet, dVal.as<uint64_t>(), n, false, 0, flag.as<uint32_t>(),
                                           off.as<uint64_t>(), tmp.p, desc.as<int>(), &descending))
            return rc;
        if (descending) { set_error("the common k-mer values descend"); return MTB_ERR_ARG; }
    }
    return finish_set(g, nSet, ev);
}

extern "C" int mtb_group_set_common_db(mtb_grouper* g, const char* db_dir) {
    if (const int rc = attachable(g)) return rc;
    if (!db_dir) { set_error("null argument"); return MTB_ERR_ARG; }
    const std::string dir(db_dir);
    int checked = 0;
    if (const int rc = check_kmer_params(g, dir, &checked)) return rc;
    FILE* f = fopen((dir + "/diffIdx").c_str(), "rb");
    if (!f) { set_error("cannot open " + dir + "/diffIdx"); return MTB_ERR_IO; }
    struct Closer { FILE* f; ~Closer() { fclose(f); } } closer{f};
    if (fseeko(f, 0, SEEK_END) != 0) { set_error("cannot size " + dir + "/diffIdx"); return MTB_ERR_IO; }
    const uint64_t bytes = (uint64_t)ftello(f);
    if (bytes % 2) { set_error("diffIdx ends mid k-mer"); return MTB_ERR_DB; }
    const uint64_t nDiff = bytes / 2;
    GRP_TRY(hipSetDevice(g->device));
    EvPair ev;
    GRP_TRY(ev.create());
    GRP_TRY(hipEventRecord(ev.a, nullptr));
    uint64_t nSet = 0;
    if (nDiff) {
        uint64_t W = 1ull << 26;  // words per chunk, as decode_db_chunked cuts the reference DB's
        if (const char* e = getenv("MTB_DECODE_CHUNK_WORDS")) W = std::max<uint64_t>(8, strtoull(e, nullptr, 10));
        W = std::min(W, nDiff);
        Buf dDiff, dFlag, dIdx, dTmp, dVal, desc;
        hipError_t e = dDiff.alloc(2 * W);
        if (e == hipSuccess) e = dFlag.alloc(4 * W);
        if (e == hipSuccess) e = dIdx.alloc(8 * (W + 2));
        if (e == hipSuccess) e = dTmp.alloc(8 * scan_tmp_elems(W + 1));
        if (e == hipSuccess) e = dVal.alloc(8 * W);
        if (e == hipSuccess) e = desc.alloc(4);
        if (e != hipSuccess) GRP_SET_OOM(e, W * (2 + 4 + 8 + 8 + 8));
        GRP_TRY(hipMemset(desc.p, 0, 4));
        std::vector<uint16_t> host(W);
        uint64_t w0 = 0, carry = 0;
        bool first = true;
        while (w0 < nDiff) {
            const uint64_t n = std::min(W, nDiff - w0);
            if (fseeko(f, (off_t)(2 * w0), SEEK_SET) != 0 || fread(host.data(), 2, n, f) != n) {
                set_error("cannot read " + dir + "/diffIdx");
                return MTB_ERR_IO;
            }
            GRP_TRY(hipMemcpy(dDiff.p, host.data(), 2 * n, hipMemcpyHostToDevice));
            uint64_t lastTerm = 0, lastValue = 0;
            const uint64_t terms = decode_diff_chunk(dDiff.as<uint16_t>(), n, carry, dVal.as<uint64_t>(), dFlag.as<uint32_t>(),
                                                     dIdx.as<uint64_t>(), dTmp.p, &lastTerm, &lastValue, nullptr);
            GRP_TRY(hipGetLastError());
            // no terminator in a whole chunk (a k-mer of more words than a chunk, or a cut tail), or a last word that ends none
            if (terms == 0 || (w0 + n == nDiff && lastTerm != n - 1)) { set_error("diffIdx ends mid k-mer"); return MTB_ERR_DB; }
            bool descending = false;
            if (const int rc = append_distinct(g->setVals, nSet, dVal.as<uint64_t>(), terms, !first, carry, dFlag.as<uint32_t>(),
                                               dIdx.as<uint64_t>(), dTmp.p, desc.as<int>(), &descending))
                return rc;
            if (descending) { set_error("diffIdx values descend"); return MTB_ERR_DB; }
            first = false;
            carry = lastValue;
            w0 += lastTerm + 1;
        }
    }
    g->fst.params_checked = checked;
    return finish_set(g, nSet, ev);
}

extern "C" int mtb_group_get_filter_stats(mtb_grouper* g, mtb_group_filter_stats* out) {
    if (!g || !out) { set_error("null argument"); return MTB_ERR_ARG; }
    *out = g->fst;
    return MTB_OK;
}

extern "C" int mtb_group_get_kmer_pos(mtb_grouper* g, uint32_t* pos, uint64_t cap, uint64_t* n) {
    if (!g || !n) { set_error("null argument"); return MTB_ERR_ARG; }
    if (!g->hasSet) { set_error("positions are kept only with a common k-mer set attached"); return MTB_ERR_ARG; }
    if (g->built || (g->kmers && !g->pos.p)) { set_error("positions are released when the edges are built"); return MTB_ERR_ARG; }
    *n = g->kmers;
    if (cap < g->kmers) return MTB_RETRY;
    if (!g->kmers) return MTB_OK;
    if (!pos) { set_error("null argument"); return MTB_ERR_ARG; }
    GRP_TRY(hipSetDevice(g->device));
    GRP_TRY(hipMemcpy(pos, g->pos.p, 4 * g->kmers, hipMemcpyDeviceToHost));
    return MTB_OK;
}

extern "C" int mtb_group_filter_common(int device, const uint64_t* db_values, uint64_t n_db, const uint64_t* values,
                                       const uint32_t* read_ids, const uint32_t* pos, uint64_t n, uint8_t* hit,
                                       uint8_t* keep) {
    if ((n_db && !db_values) || (n && (!values || !read_ids || !pos || !hit || !keep))) {
        set_error("null argument");
        return MTB_ERR_ARG;
    }
    GRP_TRY(hipSetDevice(device));
    DVec set(8);
    Buf mid, top, desc;
    SetIndex ix{};
    uint64_t nSet = 0;
    GRP_TRY(desc.alloc(4));
    GRP_TRY(hipMemset(desc.p, 0, 4));
    if (n_db) {
        Buf dVal, flag, off, tmp;
        GRP_TRY(dVal.alloc(8 * n_db));
        GRP_TRY(flag.alloc(4 * n_db));
        GRP_TRY(off.alloc(8 * (n_db + 1)));
        GRP_TRY(tmp.alloc(8 * scan_tmp_elems(n_db)));
        GRP_TRY(hipMemcpy(dVal.p, db_values, 8 * n_db, hipMemcpyHostToDevice));
        bool descending = false;
        if (const int rc = append_distinct(set, nSet, dVal.as<uint64_t>(), n_db, false, 0, flag.as<uint32_t>(), off.as<uint64_t>(),
                                           tmp.p, desc.as<int>(), &descending))
            return rc;
        if (descending) { set_error("db_values descend"); return MTB_ERR_ARG; }
    }
    if (const int rc = build_set_index(ix, set.as<uint64_t>(), nSet, mid, top)) return rc;
    if (!n) return MTB_OK;
    Buf dKeys, dIds, dPos, flag, off, segStart, tmp, dHit, dRem;
    GRP_TRY(dKeys.alloc(8 * n));
    GRP_TRY(dIds.alloc(4 * n));
    GRP_TRY(dPos.alloc(4 * n));
    GRP_TRY(flag.alloc(4 * n));
    GRP_TRY(off.alloc(8 * (n + 1)));
    GRP_TRY(tmp.alloc(8 * scan_tmp_elems(n)));
    GRP_TRY(dHit.alloc(n));
    GRP_TRY(dRem.alloc(n));
    GRP_TRY(hipMemcpy(dKeys.p, values, 8 * n, hipMemcpyHostToDevice));
    GRP_TRY(hipMemcpy(dIds.p, read_ids, 4 * n, hipMemcpyHostToDevice));
    GRP_TRY(hipMemcpy(dPos.p, pos, 4 * n, hipMemcpyHostToDevice));
    // a segment per read: the heads of the runs of equal read IDs
    k_flag_read_heads<<<stride_grid(n), 256>>>(dIds.as<uint32_t>(), n, flag.as<uint32_t>(), desc.as<int>());
    int bad = 0;
    GRP_TRY(hipMemcpy(&bad, desc.p, 4, hipMemcpyDeviceToHost));
    if (bad) { set_error("read_ids descend"); return MTB_ERR_ARG; }
    k_pos_range<<<stride_grid(n), 256>>>(dPos.as<uint32_t>(), n, desc.as<int>());
    GRP_TRY(hipMemcpy(&bad, desc.p, 4, hipMemcpyDeviceToHost));
    if (bad) { set_error("a pos of 2^31 or more"); return MTB_ERR_ARG; }
    exclusive_scan_u32(flag.as<uint32_t>(), n, off.as<uint64_t>(), tmp.p, nullptr);
    uint64_t nSeg = 0;
    GRP_TRY(hipMemcpy(&nSeg, off.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost));
    GRP_TRY(segStart.alloc(8 * (nSeg + 1)));
    k_head_pos<<<stride_grid(n + 1), 256>>>(flag.as<uint32_t>(), off.as<uint64_t>(), n, segStart.as<uint64_t>());
    if (const int rc = run_filter(ix, dKeys.as<uint64_t>(), 0, dPos.as<uint32_t>(), segStart.as<uint64_t>(), 1, nSeg, n,
                                  dHit.as<uint8_t>(), dRem.as<uint8_t>(), nullptr))
        return rc;
    GRP_TRY(hipMemcpy(hit, dHit.p, n, hipMemcpyDeviceToHost));
    GRP_TRY(hipMemcpy(keep, dRem.p, n, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++) keep[i] = !keep[i];
    return MTB_OK;
}
