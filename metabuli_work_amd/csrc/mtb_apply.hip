// Group application on the GPU (the reference fork's src/read-group/GroupApplier.cpp, workflow
// groupApplication): every group of reads gets one representative taxon, the weighted-majority label of
// its members' classifications, and the reads the classifier left unclassified or scored low take it.
//   getRepLabel   (GroupApplier.cpp:134-192): a member votes with its internal label (not 0; in weight
//                 modes 1 and 2 only with score >= minVoteScr), weight 1 / score / score * score;
//                 the representative is weightedMajorityLCA(votes, 0.5), 0 or the root = none
//   applyRepLabel (GroupApplier.cpp:194-237): per read, the representative or its own label
// weightedMajorityLCA is MMseqs2's (absent from the reference tree: PARITY UNPINNED), restated from the
// published algorithm: a vote adds its weight to its node and every ancestor; a node is a candidate when
// it is some vote's label or got weight through two or more children; of the candidates holding at
// least half the total, the one of the smallest lineage rank wins, then the largest share, then the
// smallest taxID.
// Stages (all on the device; the host sees the counts allocation and the return need):
//   keys and sort   one key per grouped read, group << 32 | label (label 0: the read does not vote),
//                   stable radix sort: a run of equal keys is one label of one group, members in read order
//   per-label sums  W(g, v) in double: slices of kApplySlice consecutive members summed from 0.0, the
//                   slice sums added in slice order (a run of at most kApplySlice members: its plain sum)
//   per-group choice  a group's labels are contiguous, ascending by taxID. Its candidates are the labels
//                   and the LCAs among them; with the labels in pre-order every such LCA is the LCA of a
//                   label and its pre-order predecessor among the labels, so each label brings two
//                   candidates. C(g, c) = the sum of W(g, v) over the labels v in c's clade (a pre-order
//                   interval test), ascending taxID; T(g) the same over all labels; share = C / T.
//   apply           per read: the representative, or its own label
// The reference adds a group's weights in unordered_set order; the orders above are fixed instead.
#include <algorithm>
#include <charconv>
#include <climits>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "mtb_host.h"
#include "mtb_launch.h"

namespace mtb {

constexpr uint32_t kApplySlice = 1024;      // members per slice of a label's sum
constexpr uint32_t kApplyThreadLabels = 8;  // a thread chooses for a group of at most this many labels
constexpr uint32_t kApplyWaveLabels = 128;  // a wave, labels in LDS, up to this many; a workgroup beyond
constexpr int32_t kRootRank = INT32_MAX;    // lineage rank of a lineage without a ranked node (ROOT_RANK)

enum {  // device counters of one call
    kCtVoters = 0, kCtRuns, kCtGroups, kCtWithRep, kCtApplied, kCtLong, kCtWave, kCtBlock, kCtBadRead, kCtBadGroup,
    kCtLabels, kCtCount
};

struct ApplyTax {
    TaxDevice t;
    const int32_t* tin;   // node -> pre-order index
    const int32_t* tout;  // node -> pre-order index past its clade
};

// One key per read: group << 32 | label for a grouped read (label 0 unless it votes; a merged taxID
// votes as the node it was merged into), kSentinel for a read of no group. Counters: the first read
// whose non-zero label the taxonomy does not hold, the first read of group 2^32 - 1.
__global__ void __launch_bounds__(256) k_apply_keys(const uint32_t* __restrict__ gm, const int32_t* __restrict__ tax,
                                                    const float* __restrict__ score, uint64_t n, int mode, float thr,
                                                    ApplyTax T, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                    unsigned long long* ctr) {
    MTB_GRID_STRIDE(r, n) {
        const uint32_t g = gm[r + 1];
        const int32_t t = tax[r];
        const bool known = t == 0 || (t > 0 && t <= T.t.maxTax && T.t.nodeOf[t] >= 0);
        if (!known) atomicMin(ctr + kCtBadRead, (unsigned long long)r);
        uint64_t key = kSentinel;
        if (g == 0xFFFFFFFFu) {
            atomicMin(ctr + kCtBadGroup, (unsigned long long)r);
        } else if (g != 0) {
            uint32_t lab = 0;
            if (known && t != 0 && (mode == 0 || score[r] >= thr)) lab = (uint32_t)T.t.nodeTax[T.t.nodeOf[t]];
            if (lab) atomicAdd(ctr + kCtVoters, 1ull);
            key = (uint64_t)g << 32 | lab;
        }
        keys[r] = key;
        vals[r] = (uint32_t)r;
    }
}

__global__ void __launch_bounds__(256) k_apply_run_heads(const uint64_t* __restrict__ keys, uint64_t V,
                                                         uint32_t* __restrict__ head) {
    MTB_GRID_STRIDE(i, V) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// runIdx: the exclusive scan of head (V + 1 entries; runIdx[V] = the runs)
__global__ void __launch_bounds__(256) k_apply_run_starts(const uint32_t* __restrict__ head,
                                                          const uint32_t* __restrict__ runIdx, uint64_t V,
                                                          uint32_t* __restrict__ runStart, unsigned long long* ctr) {
    MTB_GRID_STRIDE(i, V) {
        if (head[i]) runStart[runIdx[i]] = (uint32_t)i;
        if (i == 0) {
            runStart[runIdx[V]] = (uint32_t)V;
            ctr[kCtRuns] = runIdx[V];
        }
    }
}

__device__ __forceinline__ double apply_weight(const float* score, uint32_t r, int mode) {
    if (mode == 0) return 1.0;
    const float s = score[r];
    return mode == 1 ? (double)s : (double)(s * s);  // the float product, as setTaxa.emplace_back(.., score * score, ..)
}

// Per run: its node and pre-order index, its group-head flag, and W when it has at most kApplySlice
// members; longer runs are queued for k_apply_sums_long.
__global__ void __launch_bounds__(256) k_apply_sums(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                    const float* __restrict__ score, const uint32_t* __restrict__ runStart,
                                                    uint64_t V, int mode, ApplyTax T, double* __restrict__ W,
                                                    int32_t* __restrict__ runNode, int32_t* __restrict__ runTin,
                                                    uint32_t* __restrict__ ghead, uint32_t* __restrict__ longList,
                                                    unsigned long long* ctr) {
    const uint64_t L = ctr[kCtRuns];
    MTB_GRID_STRIDE(r, V) {
        if (r >= L) continue;
        const uint32_t a = runStart[r], b = runStart[r + 1];
        const uint64_t k = keys[a];
        const uint32_t lab = (uint32_t)k;
        ghead[r] = (r == 0 || (keys[runStart[r - 1]] >> 32) != (k >> 32)) ? 1u : 0u;
        if (lab == 0) {  // the group's members without a vote
            W[r] = 0.0;
            runNode[r] = 0;
            runTin[r] = -1;
            continue;
        }
        atomicAdd(ctr + kCtLabels, 1ull);
        const int32_t node = T.t.nodeOf[lab];
        runNode[r] = node;
        runTin[r] = T.tin[node];
        if (b - a <= kApplySlice) {
            double s = 0.0;
            for (uint32_t i = a; i < b; i++) s += apply_weight(score, vals[i], mode);
            W[r] = s;
        } else {
            longList[atomicAdd(ctr + kCtLong, 1ull)] = (uint32_t)r;
        }
    }
}

// A workgroup per queued run: 256 slices at a time, a thread per slice (sequential from 0.0), then
// thread 0 adds the slice sums in slice order.
__global__ void __launch_bounds__(256) k_apply_sums_long(const uint32_t* __restrict__ vals, const float* __restrict__ score,
                                                         const uint32_t* __restrict__ runStart, int mode,
                                                         const uint32_t* __restrict__ longList, double* __restrict__ W,
                                                         const unsigned long long* ctr) {
    __shared__ double part[256];
    const uint64_t nLong = ctr[kCtLong];
    for (uint64_t e = blockIdx.x; e < nLong; e += gridDim.x) {
        const uint32_t r = longList[e];
        const uint32_t a = runStart[r], b = runStart[r + 1];
        const uint32_t slices = (b - a + kApplySlice - 1) / kApplySlice;
        double total = 0.0;
        for (uint32_t s0 = 0; s0 < slices; s0 += 256) {
            const uint32_t sl = s0 + threadIdx.x;
            double s = 0.0;
            if (sl < slices) {
                const uint32_t lo = a + sl * kApplySlice, hi = min(b, lo + kApplySlice);
                for (uint32_t i = lo; i < hi; i++) s += apply_weight(score, vals[i], mode);
            }
            part[threadIdx.x] = s;
            __syncthreads();
            if (threadIdx.x == 0) {
                const uint32_t cnt = min(256u, slices - s0);
                for (uint32_t j = 0; j < cnt; j++) total += part[j];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) W[r] = total;
    }
}

// grpIdx: the exclusive scan of ghead over V entries (zero past the runs; grpIdx[V] = the groups)
__global__ void __launch_bounds__(256) k_apply_group_starts(const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ runStart,
                                                            const uint32_t* __restrict__ ghead,
                                                            const uint32_t* __restrict__ grpIdx, uint64_t V,
                                                            uint32_t* __restrict__ gStart, uint32_t* __restrict__ repGroup,
                                                            unsigned long long* ctr) {
    const uint64_t L = ctr[kCtRuns];
    MTB_GRID_STRIDE(r, V) {
        if (r < L && ghead[r]) {
            gStart[grpIdx[r]] = (uint32_t)r;
            repGroup[grpIdx[r]] = (uint32_t)(keys[runStart[r]] >> 32);
        }
        if (r == 0) {
            gStart[grpIdx[V]] = (uint32_t)L;
            ctr[kCtGroups] = grpIdx[V];
        }
    }
}

// ---- the choice ------------------------------------------------------------------------------------
struct ApplyBest {  // the qualifying candidate so far; rank kNoBest: none
    int32_t rank;
    int32_t tax;
    double ratio;
};
constexpr int32_t kNoBest = -1;

__device__ __forceinline__ bool apply_better(int32_t rank, double ratio, int32_t tax, const ApplyBest& b) {
    if (b.rank == kNoBest) return true;
    if (rank != b.rank) return rank < b.rank;
    if (ratio != b.ratio) return ratio > b.ratio;
    return tax < b.tax;
}
__device__ __forceinline__ void apply_merge(ApplyBest& a, const ApplyBest& b) {
    if (b.rank != kNoBest && apply_better(b.rank, b.ratio, b.tax, a)) a = b;
}

__device__ __forceinline__ int apply_lca(const TaxDevice& t, int i, int j) {
    while (i != j) {
        const int di = t.depth[i], dj = t.depth[j];
        if (di >= dj) i = t.parent[i];
        if (dj >= di) j = t.parent[j];
    }
    return i;
}

// Labels of one group behind an accessor (tin(k), node(k), w(k), k ascending by taxID): the candidates
// of labels k0, k0 + step, ... weighed against the whole group.
template <class Labels>
__device__ __forceinline__ void apply_candidate(const Labels& lab, uint32_t m, double total, const ApplyTax& T, int c,
                                                ApplyBest& best) {
    const int32_t lo = T.tin[c], hi = T.tout[c];
    double C = 0.0;
    for (uint32_t j = 0; j < m; j++) {
        const int32_t tj = lab.tin(j);
        if (tj >= lo && tj < hi) C += lab.w(j);
    }
    const double ratio = C / total;
    if (ratio >= 0.5) {
        const int32_t rank = T.t.lineageRank[c], tax = T.t.nodeTax[c];
        if (apply_better(rank, ratio, tax, best)) best = ApplyBest{rank, tax, ratio};
    }
}

template <class Labels>
__device__ __forceinline__ void apply_choose(const Labels& lab, uint32_t m, double total, const ApplyTax& T, uint32_t k0,
                                             uint32_t step, ApplyBest& best) {
    for (uint32_t k = k0; k < m; k += step) {
        const int32_t tk = lab.tin(k);
        const int nk = lab.node(k);
        int32_t predTin = -1;
        int pred = -1;
        for (uint32_t j = 0; j < m; j++) {  // the label before it in pre-order
            const int32_t tj = lab.tin(j);
            if (tj < tk && tj > predTin) {
                predTin = tj;
                pred = lab.node(j);
            }
        }
        apply_candidate(lab, m, total, T, nk, best);
        if (pred >= 0) {
            const int c = apply_lca(T.t, nk, pred);
            if (c != nk) apply_candidate(lab, m, total, T, c, best);
        }
    }
}

__device__ __forceinline__ int32_t apply_rep(const ApplyBest& b) { return b.rank == kNoBest || b.tax == 1 ? 0 : b.tax; }

struct LabelsGlobal {
    const int32_t *tinP, *nodeP;
    const double* wP;
    __device__ int32_t tin(uint32_t k) const { return tinP[k]; }
    __device__ int node(uint32_t k) const { return nodeP[k]; }
    __device__ double w(uint32_t k) const { return wP[k]; }
};
struct LabelsLdsThread {  // [label][thread of the workgroup]
    const int32_t (*tinP)[256];
    const int32_t (*nodeP)[256];
    const double (*wP)[256];
    uint32_t t;
    __device__ int32_t tin(uint32_t k) const { return tinP[k][t]; }
    __device__ int node(uint32_t k) const { return nodeP[k][t]; }
    __device__ double w(uint32_t k) const { return wP[k][t]; }
};

// The runs of group j that carry a label: [*ra, *ra + m)
__device__ __forceinline__ uint32_t apply_group_labels(const uint32_t* gStart, const int32_t* runTin, uint32_t j,
                                                       uint32_t* ra) {
    uint32_t a = gStart[j];
    const uint32_t b = gStart[j + 1];
    if (a < b && runTin[a] < 0) a++;  // the members without a vote sort first (label 0)
    *ra = a;
    return b - a;
}

// A thread per group: up to kApplyThreadLabels labels are chosen here (staged in LDS), larger groups
// queued for the wave or the workgroup kernel.
__global__ void __launch_bounds__(256) k_apply_choose_thread(const uint32_t* __restrict__ gStart,
                                                             const int32_t* __restrict__ runTin,
                                                             const int32_t* __restrict__ runNode,
                                                             const double* __restrict__ W, uint64_t V, ApplyTax T,
                                                             int32_t* __restrict__ repTax, uint32_t* __restrict__ waveList,
                                                             uint32_t* __restrict__ blockList, unsigned long long* ctr) {
    __shared__ int32_t sTin[kApplyThreadLabels][256];
    __shared__ int32_t sNode[kApplyThreadLabels][256];
    __shared__ double sW[kApplyThreadLabels][256];
    const uint64_t G = ctr[kCtGroups];
    MTB_GRID_STRIDE(j, V) {
        if (j >= G) continue;
        uint32_t ra;
        const uint32_t m = apply_group_labels(gStart, runTin, (uint32_t)j, &ra);
        if (m > kApplyWaveLabels) {
            blockList[atomicAdd(ctr + kCtBlock, 1ull)] = (uint32_t)j;
            continue;
        }
        if (m > kApplyThreadLabels) {
            waveList[atomicAdd(ctr + kCtWave, 1ull)] = (uint32_t)j;
            continue;
        }
        double total = 0.0;
        for (uint32_t k = 0; k < m; k++) {
            sTin[k][threadIdx.x] = runTin[ra + k];
            sNode[k][threadIdx.x] = runNode[ra + k];
            const double w = W[ra + k];
            sW[k][threadIdx.x] = w;
            total += w;
        }
        ApplyBest best{kNoBest, 0, 0.0};
        if (m && total != 0.0) {
            const LabelsLdsThread lab{sTin, sNode, sW, threadIdx.x};
            apply_choose(lab, m, total, T, 0, 1, best);
        }
        const int32_t rep = apply_rep(best);
        repTax[j] = rep;
        if (rep) atomicAdd(ctr + kCtWithRep, 1ull);
    }
}

// A workgroup of kThreads per queued group. LDS: the labels are staged in LDS (one wave, up to
// kApplyWaveLabels labels); otherwise they are read where the per-label pass left them in HBM. Each
// thread takes the labels k = thread, thread + kThreads, ...; thread 0 folds the threads' choices.
template <int kThreads, bool LDS>
__global__ void __launch_bounds__(kThreads) k_apply_choose_group(const uint32_t* __restrict__ gStart,
                                                                 const int32_t* __restrict__ runTin,
                                                                 const int32_t* __restrict__ runNode,
                                                                 const double* __restrict__ W, ApplyTax T,
                                                                 const uint32_t* __restrict__ list, int ctrList,
                                                                 int32_t* __restrict__ repTax, unsigned long long* ctr) {
    constexpr uint32_t kStage = LDS ? kApplyWaveLabels : 1;
    __shared__ int32_t sTin[kStage];
    __shared__ int32_t sNode[kStage];
    __shared__ double sW[kStage];
    __shared__ ApplyBest sBest[kThreads];
    __shared__ double sTotal;
    const uint64_t nList = ctr[ctrList];
    for (uint64_t e = blockIdx.x; e < nList; e += gridDim.x) {
        const uint32_t j = list[e];
        uint32_t ra;
        const uint32_t m = apply_group_labels(gStart, runTin, j, &ra);
        if constexpr (LDS) {
            for (uint32_t k = threadIdx.x; k < m && k < kStage; k += kThreads) {
                sTin[k] = runTin[ra + k];
                sNode[k] = runNode[ra + k];
                sW[k] = W[ra + k];
            }
        }
        if (threadIdx.x == 0) {
            double total = 0.0;
            for (uint32_t k = 0; k < m; k++) total += W[ra + k];
            sTotal = total;
        }
        __syncthreads();
        const double total = sTotal;
        ApplyBest best{kNoBest, 0, 0.0};
        if (total != 0.0) {
            if constexpr (LDS) {
                const LabelsGlobal lab{sTin, sNode, sW};  // the same accessor over the staged copies
                apply_choose(lab, m, total, T, threadIdx.x, kThreads, best);
            } else {
                const LabelsGlobal lab{runTin + ra, runNode + ra, W + ra};
                apply_choose(lab, m, total, T, threadIdx.x, kThreads, best);
            }
        }
        sBest[threadIdx.x] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            ApplyBest b = sBest[0];
            for (int t = 1; t < kThreads; t++) apply_merge(b, sBest[t]);
            const int32_t rep = apply_rep(b);
            repTax[j] = rep;
            if (rep) atomicAdd(ctr + kCtWithRep, 1ull);
        }
        __syncthreads();
    }
}

// ---- apply -----------------------------------------------------------------------------------------
// Reads of no group keep their label.
__global__ void __launch_bounds__(256) k_apply_ungrouped(const uint32_t* __restrict__ gm, const int32_t* __restrict__ tax,
                                                         uint64_t n, int32_t* __restrict__ outTax,
                                                         uint8_t* __restrict__ outCls, uint8_t* __restrict__ outApplied) {
    MTB_GRID_STRIDE(r, n) {
        if (gm[r + 1] != 0) continue;
        const int32_t t = tax[r];
        outTax[r] = t;
        outCls[r] = t != 0;
        outApplied[r] = 0;
    }
}

// Grouped reads, through the sorted order (position -> run -> group -> representative).
__global__ void __launch_bounds__(256) k_apply_grouped(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ runIdx,
                                                       const uint32_t* __restrict__ grpIdx,
                                                       const int32_t* __restrict__ repTax, const int32_t* __restrict__ tax,
                                                       const float* __restrict__ score, uint64_t V, int mode, float thr,
                                                       int32_t* __restrict__ outTax, uint8_t* __restrict__ outCls,
                                                       uint8_t* __restrict__ outApplied, unsigned long long* ctr) {
    MTB_GRID_STRIDE(i, V) {
        const uint32_t r = vals[i];
        const uint32_t run = runIdx[i + 1] - 1;   // the inclusive scan at i
        const uint32_t grp = grpIdx[run + 1] - 1;
        const int32_t rep = repTax[grp];
        const int32_t t = tax[r];
        bool applied = false;
        if (rep != 0) applied = mode == 0 || t == 0 || score[r] < thr;
        outTax[r] = applied ? rep : t;
        outCls[r] = rep != 0 || t != 0;
        outApplied[r] = applied;
        if (applied) atomicAdd(ctr + kCtApplied, 1ull);
    }
}

__global__ void __launch_bounds__(256) k_apply_label_out(const uint64_t* __restrict__ keys,
                                                         const uint32_t* __restrict__ runStart, uint64_t V,
                                                         const unsigned long long* ctr, uint64_t* __restrict__ outKey) {
    const uint64_t L = ctr[kCtRuns];
    MTB_GRID_STRIDE(r, V)
        if (r < L) outKey[r] = keys[runStart[r]];
}

namespace {

#define APL_TRY(x)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x);      \
            return e_ == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                 \
        }                                                                                 \
    } while (0)

struct ApplyRun {  // device memory, stream and events of one call, released on every return
    void* arena = nullptr;
    void* tax = nullptr;
    void* io = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~ApplyRun() {
        if (s) hipStreamSynchronize(s);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (s) hipStreamDestroy(s);
        if (arena) hipFree(arena);
        if (tax) hipFree(tax);
        if (io) hipFree(io);
    }
};

struct Carve {  // 256-B aligned pieces of one allocation
    uint64_t bytes = 0;
    uint64_t take(uint64_t b) {
        const uint64_t at = bytes;
        bytes += (b + 255) / 256 * 256;
        return at;
    }
};

int bits_of(uint64_t x) {
    int b = 1;
    while (b < 64 && (x >> b)) b++;
    return b;
}

bool taxonomy_from_host(const mtb_db_host* taxo, HostTaxonomy& T) {
    std::vector<std::string> ranks(taxo->n_nodes), names(taxo->n_nodes);
    for (uint64_t i = 0; i < taxo->n_nodes; i++) {
        ranks[i] = taxo->rank_pool + taxo->rank_off[i];
        if (taxo->name_pool && taxo->name_off) names[i] = taxo->name_pool + taxo->name_off[i];
    }
    return build_taxonomy(taxo->node_taxid, taxo->node_parent, taxo->n_nodes, ranks, names, taxo->merged_old,
                          taxo->merged_new, taxo->n_merged, T);
}

// Pre-order intervals of every node's clade, O(nodes).
void preorder(const HostTaxonomy& T, std::vector<int32_t>& tin, std::vector<int32_t>& tout) {
    const size_t n = T.parent.size();
    const int root = T.nodeOf[1];
    std::vector<uint32_t> first(n + 1, 0), child(n);
    for (size_t i = 0; i < n; i++)
        if ((int)i != root) first[T.parent[i] + 1]++;
    for (size_t i = 0; i < n; i++) first[i + 1] += first[i];
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        for (size_t i = 0; i < n; i++)
            if ((int)i != root) child[at[T.parent[i]]++] = (uint32_t)i;
    }
    tin.assign(n, 0);
    tout.assign(n, 0);
    std::vector<std::pair<int, uint32_t>> stack;  // node, its next child
    int32_t clock = 0;
    tin[root] = clock++;
    stack.emplace_back(root, first[root]);
    while (!stack.empty()) {
        auto& top = stack.back();
        if (top.second < first[top.first + 1]) {
            const int c = (int)child[top.second++];
            tin[c] = clock++;
            stack.emplace_back(c, first[c]);
        } else {
            tout[top.first] = clock;
            stack.pop_back();
        }
    }
}

}  // namespace

// The lineage rank of every node, O(nodes): the rank index of the first node with an index > 0 from
// the node itself towards the root, the root never looked at; kRootRank when there is none.
std::vector<int32_t> lineage_ranks(const HostTaxonomy& T) {
    const size_t n = T.parent.size();
    const int root = T.nodeOf[1];
    std::vector<int32_t> lr(n, -1);
    lr[root] = kRootRank;
    std::vector<int> chain;
    for (size_t i = 0; i < n; i++) {
        int x = (int)i;
        chain.clear();
        while (lr[x] < 0) {
            const int ri = HostTaxonomy::rankIndex(T.rank[x]);
            if (ri > 0) {
                lr[x] = ri;
                break;
            }
            chain.push_back(x);
            x = T.parent[x];
        }
        for (int c : chain) lr[c] = lr[x];
    }
    return lr;
}

namespace {

struct ApplyIo {  // the per-read arrays of one call; host pointers unless devIn
    const uint32_t* groupMap;
    const int32_t* taxIds;
    const float* scores;
    uint64_t n;
    bool devIn;
    uint32_t* repGroup;
    int32_t* repTax;
    uint64_t repCap;
    uint64_t* nGroups;
    int32_t* outTax;
    uint8_t* outCls;
    uint8_t* outApplied;
    // staged (host arrays, nullable): the per-label sums, (group << 32 | label, W) ascending
    uint64_t* labelKeys = nullptr;
    double* labelW = nullptr;
    uint64_t labelCap = 0;
    uint64_t* nLabels = nullptr;
};

int apply_core(const HostTaxonomy& T, const mtb_group_apply_params& par, int device, const ApplyIo& io,
               mtb_group_apply_stats* stats) {
    const uint64_t n = io.n, n1 = n + 1;
    const int mode = par.weight_mode;
    const float thr = par.min_vote_score;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (io.nGroups) *io.nGroups = 0;
    if (io.nLabels) *io.nLabels = 0;

    // host arrays: the refusals before any device call
    if (!io.devIn) {
        for (uint64_t r = 0; r < n; r++) {
            const int32_t t = io.taxIds[r];
            if (t != 0 && !T.exists(t)) {
                set_error("read " + std::to_string(r + 1) + ": label " + std::to_string(t) + " is not in the taxonomy");
                return MTB_ERR_ARG;
            }
            if (io.groupMap[r + 1] == 0xFFFFFFFFu) {
                set_error("read " + std::to_string(r + 1) + ": group ID 2^32 - 1");
                return MTB_ERR_ARG;
            }
        }
    }

    APL_TRY(hipSetDevice(device));
    ApplyRun run;
    APL_TRY(hipStreamCreateWithFlags(&run.s, hipStreamNonBlocking));
    for (hipEvent_t& e : run.ev) APL_TRY(hipEventCreate(&e));
    hipStream_t s = run.s;

    // the taxonomy
    const std::vector<int32_t> lr = lineage_ranks(T);
    std::vector<int32_t> tin, tout;
    preorder(T, tin, tout);
    const uint64_t nNodes = T.parent.size(), nTax = (uint64_t)T.maxTax + 1;
    Carve ct;
    const uint64_t oNodeOf = ct.take(4 * nTax), oNodeTax = ct.take(4 * nNodes), oParent = ct.take(4 * nNodes),
                   oDepth = ct.take(4 * nNodes), oLr = ct.take(4 * nNodes), oTin = ct.take(4 * nNodes),
                   oTout = ct.take(4 * nNodes);
    // the per-read arrays on the device (host input) and the scratch, one allocation each
    Carve ci;
    uint64_t oGm = 0, oTaxIn = 0, oScore = 0, oOutTax = 0, oOutCls = 0, oOutApp = 0;
    if (!io.devIn) {
        oGm = ci.take(4 * n1); oTaxIn = ci.take(4 * n1); oScore = ci.take(4 * n1);
        oOutTax = ci.take(4 * n1); oOutCls = ci.take(n1); oOutApp = ci.take(n1);
    }
    Carve ca;
    const uint64_t rc = radix_counts_elems(n1);
    const uint64_t oKA = ca.take(8 * n1), oKB = ca.take(8 * n1), oVA = ca.take(4 * n1), oVB = ca.take(4 * n1),
                   oCnt = ca.take(4 * rc), oOffs = ca.take(8 * (rc + 1)), oTmp = ca.take(8 * scan_tmp_elems(rc + n + 2)),
                   oHead = ca.take(4 * n1), oRunIdx = ca.take(4 * (n1 + 1)), oRunStart = ca.take(4 * (n1 + 1)),
                   oW = ca.take(8 * n1), oRunNode = ca.take(4 * n1), oRunTin = ca.take(4 * n1),
                   oGhead = ca.take(4 * n1), oGrpIdx = ca.take(4 * (n1 + 1)), oGStart = ca.take(4 * (n1 + 1)),
                   oRepG = ca.take(4 * n1), oRepT = ca.take(4 * n1), oLong = ca.take(4 * (n / kApplySlice + 1)),
                   oWave = ca.take(4 * (n / (kApplyThreadLabels + 1) + 1)),
                   oBlock = ca.take(4 * (n / (kApplyWaveLabels + 1) + 1)), oCtr = ca.take(8 * kCtCount);
    const uint64_t need = ct.bytes + ci.bytes + ca.bytes;
    {
        hipError_t e = hipMalloc(&run.tax, ct.bytes ? ct.bytes : 256);
        if (e == hipSuccess) e = hipMalloc(&run.io, ci.bytes ? ci.bytes : 256);
        if (e == hipSuccess) e = hipMalloc(&run.arena, ca.bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("the group application does not fit the device: " + std::to_string(need) + " bytes needed");
            return e == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;
        }
    }
    char* tb = (char*)run.tax;
    APL_TRY(hipMemcpyAsync(tb + oNodeOf, T.nodeOf.data(), 4 * nTax, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oNodeTax, T.nodeTax.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oParent, T.parent.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oDepth, T.depth.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oLr, lr.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oTin, tin.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    APL_TRY(hipMemcpyAsync(tb + oTout, tout.data(), 4 * nNodes, hipMemcpyHostToDevice, s));
    ApplyTax D;
    D.t = TaxDevice{(const int32_t*)(tb + oNodeOf), (const int32_t*)(tb + oNodeTax), (const int32_t*)(tb + oParent),
                    (const int32_t*)(tb + oDepth), nullptr, nullptr, T.maxTax, (const int32_t*)(tb + oLr)};
    D.tin = (const int32_t*)(tb + oTin);
    D.tout = (const int32_t*)(tb + oTout);

    char* ib = (char*)run.io;
    const uint32_t* gm = io.groupMap;
    const int32_t* taxIn = io.taxIds;
    const float* score = io.scores;
    int32_t* outTax = io.outTax;
    uint8_t *outCls = io.outCls, *outApp = io.outApplied;
    if (!io.devIn) {
        APL_TRY(hipMemcpyAsync(ib + oGm, io.groupMap, 4 * n1, hipMemcpyHostToDevice, s));
        if (n) APL_TRY(hipMemcpyAsync(ib + oTaxIn, io.taxIds, 4 * n, hipMemcpyHostToDevice, s));
        if (n && mode != 0) APL_TRY(hipMemcpyAsync(ib + oScore, io.scores, 4 * n, hipMemcpyHostToDevice, s));
        gm = (const uint32_t*)(ib + oGm);
        taxIn = (const int32_t*)(ib + oTaxIn);
        score = (const float*)(ib + oScore);
        outTax = (int32_t*)(ib + oOutTax);
        outCls = (uint8_t*)(ib + oOutCls);
        outApp = (uint8_t*)(ib + oOutApp);
    }

    char* ab = (char*)run.arena;
    uint64_t *kA = (uint64_t*)(ab + oKA), *kB = (uint64_t*)(ab + oKB);
    uint32_t *vA = (uint32_t*)(ab + oVA), *vB = (uint32_t*)(ab + oVB);
    uint32_t* cnt = (uint32_t*)(ab + oCnt);
    uint64_t* offs = (uint64_t*)(ab + oOffs);
    void* tmp = ab + oTmp;
    uint32_t *head = (uint32_t*)(ab + oHead), *runIdx = (uint32_t*)(ab + oRunIdx), *runStart = (uint32_t*)(ab + oRunStart);
    double* W = (double*)(ab + oW);
    int32_t *runNode = (int32_t*)(ab + oRunNode), *runTin = (int32_t*)(ab + oRunTin);
    uint32_t *ghead = (uint32_t*)(ab + oGhead), *grpIdx = (uint32_t*)(ab + oGrpIdx), *gStart = (uint32_t*)(ab + oGStart);
    uint32_t* repG = (uint32_t*)(ab + oRepG);
    int32_t* repT = (int32_t*)(ab + oRepT);
    uint32_t *longList = (uint32_t*)(ab + oLong), *waveList = (uint32_t*)(ab + oWave), *blockList = (uint32_t*)(ab + oBlock);
    unsigned long long* ctr = (unsigned long long*)(ab + oCtr);

    unsigned long long h[kCtCount];
    memset(h, 0, sizeof h);
    h[kCtBadRead] = h[kCtBadGroup] = ~0ull;
    APL_TRY(hipMemcpyAsync(ctr, h, sizeof h, hipMemcpyHostToDevice, s));

    // keys and sort
    APL_TRY(hipEventRecord(run.ev[0], s));
    uint64_t V = 0;
    const uint64_t* K = kA;
    const uint32_t* R = vA;
    if (n) {
        k_apply_keys<<<stride_grid(n), 256, 0, s>>>(gm, taxIn, score, n, mode, thr, D, kA, vA, ctr);
        // least significant first: the label bits (sentinels dropped there), then the group bits
        bool inB = false;
        V = radix_sort_pairs<uint32_t>(kA, vA, kB, vB, n, 0, bits_of((uint64_t)T.maxTax), true, false, cnt, offs, tmp, &inB, s);
        APL_TRY(hipGetLastError());
        if (V > n) { set_error("radix sort kept more pairs than it was given"); return MTB_ERR_INTERNAL; }
        uint64_t *k0 = inB ? kB : kA, *k1 = inB ? kA : kB;
        uint32_t *v0 = inB ? vB : vA, *v1 = inB ? vA : vB;
        bool inB2 = false;
        if (V) radix_sort_pairs<uint32_t>(k0, v0, k1, v1, V, 32, 64, false, false, cnt, offs, tmp, &inB2, s);
        APL_TRY(hipGetLastError());
        K = inB2 ? k1 : k0;
        R = inB2 ? v1 : v0;
    }
    APL_TRY(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, s));
    APL_TRY(hipStreamSynchronize(s));
    if (h[kCtBadRead] != ~0ull) {
        set_error("read " + std::to_string(h[kCtBadRead] + 1) + ": its label is not in the taxonomy");
        return MTB_ERR_ARG;
    }
    if (h[kCtBadGroup] != ~0ull) {
        set_error("read " + std::to_string(h[kCtBadGroup] + 1) + ": group ID 2^32 - 1");
        return MTB_ERR_ARG;
    }
    APL_TRY(hipEventRecord(run.ev[1], s));

    // per-label sums
    if (V) {
        k_apply_run_heads<<<stride_grid(V), 256, 0, s>>>(K, V, head);
        exclusive_scan_u32_out32(head, V, runIdx, tmp, s);
        k_apply_run_starts<<<stride_grid(V), 256, 0, s>>>(head, runIdx, V, runStart, ctr);
        APL_TRY(hipMemsetAsync(ghead, 0, 4 * V, s));
        k_apply_sums<<<stride_grid(V), 256, 0, s>>>(K, R, score, runStart, V, mode, D, W, runNode, runTin, ghead, longList, ctr);
        const uint64_t longCap = V / kApplySlice + 1;
        k_apply_sums_long<<<(unsigned)std::min<uint64_t>(longCap, 4096), 256, 0, s>>>(R, score, runStart, mode, longList, W, ctr);
    }
    APL_TRY(hipEventRecord(run.ev[2], s));

    // per-group choice
    if (V) {
        exclusive_scan_u32_out32(ghead, V, grpIdx, tmp, s);
        k_apply_group_starts<<<stride_grid(V), 256, 0, s>>>(K, runStart, ghead, grpIdx, V, gStart, repG, ctr);
        k_apply_choose_thread<<<stride_grid(V), 256, 0, s>>>(gStart, runTin, runNode, W, V, D, repT, waveList, blockList, ctr);
        const uint64_t waveCap = V / (kApplyThreadLabels + 1) + 1, blockCap = V / (kApplyWaveLabels + 1) + 1;
        k_apply_choose_group<64, true><<<(unsigned)std::min<uint64_t>(waveCap, 8192), 64, 0, s>>>(
            gStart, runTin, runNode, W, D, waveList, kCtWave, repT, ctr);
        k_apply_choose_group<256, false><<<(unsigned)std::min<uint64_t>(blockCap, 2048), 256, 0, s>>>(
            gStart, runTin, runNode, W, D, blockList, kCtBlock, repT, ctr);
    }
    APL_TRY(hipEventRecord(run.ev[3], s));

    // apply
    if (n) k_apply_ungrouped<<<stride_grid(n), 256, 0, s>>>(gm, taxIn, n, outTax, outCls, outApp);
    if (V) k_apply_grouped<<<stride_grid(V), 256, 0, s>>>(R, runIdx, grpIdx, repT, taxIn, score, V, mode, thr, outTax, outCls, outApp, ctr);
    APL_TRY(hipEventRecord(run.ev[4], s));
    APL_TRY(hipGetLastError());
    APL_TRY(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, s));
    APL_TRY(hipStreamSynchronize(s));

    const uint64_t G = h[kCtGroups], L = h[kCtRuns];
    if (stats) {
        stats->reads = n;
        stats->voting_reads = h[kCtVoters];
        stats->labels = h[kCtLabels];
        stats->groups = G;
        stats->groups_with_rep = h[kCtWithRep];
        stats->applied = h[kCtApplied];
        for (int k = 0; k < 4; k++) APL_TRY(hipEventElapsedTime(&stats->ms[k], run.ev[k], run.ev[k + 1]));
    }
    if (G > V || L > V) { set_error("more groups or labels than grouped reads"); return MTB_ERR_INTERNAL; }
    if (!io.devIn && n) {
        APL_TRY(hipMemcpyAsync(io.outTax, outTax, 4 * n, hipMemcpyDeviceToHost, s));
        APL_TRY(hipMemcpyAsync(io.outCls, outCls, n, hipMemcpyDeviceToHost, s));
        APL_TRY(hipMemcpyAsync(io.outApplied, outApp, n, hipMemcpyDeviceToHost, s));
    }
    int rcode = MTB_OK;
    if (io.nGroups) *io.nGroups = G;
    if (G > io.repCap) {
        rcode = MTB_RETRY;
    } else if (G) {
        const hipMemcpyKind kind = io.devIn ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        APL_TRY(hipMemcpyAsync(io.repGroup, repG, 4 * G, kind, s));
        APL_TRY(hipMemcpyAsync(io.repTax, repT, 4 * G, kind, s));
    }
    if (io.nLabels) {
        *io.nLabels = L;
        if (L > io.labelCap) {
            rcode = MTB_RETRY;
        } else if (L) {  // the sort's other key buffer is free now
            uint64_t* ok = K == kA ? kB : kA;
            k_apply_label_out<<<stride_grid(V), 256, 0, s>>>(K, runStart, V, ctr, ok);
            APL_TRY(hipGetLastError());
            APL_TRY(hipMemcpyAsync(io.labelKeys, ok, 8 * L, hipMemcpyDeviceToHost, s));
            APL_TRY(hipMemcpyAsync(io.labelW, W, 8 * L, hipMemcpyDeviceToHost, s));
        }
    }
    APL_TRY(hipStreamSynchronize(s));
    return rcode;
}

}  // namespace
}  // namespace mtb

using namespace mtb;

namespace {

int check_apply_params(const mtb_group_apply_params* par) {
    if (!par) { set_error("null parameters"); return MTB_ERR_ARG; }
    if (par->weight_mode < 0 || par->weight_mode > 2) {
        set_error("weight_mode " + std::to_string(par->weight_mode) + " (0 uniform, 1 score, 2 score^2)");
        return MTB_ERR_ARG;
    }
    return MTB_OK;
}

int check_taxonomy_arg(const mtb_db_host* taxo) {
    if (!taxo) { set_error("null argument"); return MTB_ERR_ARG; }
    if (!taxo->node_taxid || !taxo->node_parent || !taxo->rank_pool || !taxo->rank_off) {
        set_error("null taxonomy arrays");
        return MTB_ERR_ARG;
    }
    return MTB_OK;
}

// TaxonomyWrapper::splitByDelimiter(line, "\t", 20)
std::vector<std::string> split_tabs(const std::string& s, int maxCol) {
    std::vector<std::string> out;
    size_t prev = 0, pos = 0;
    int i = 0;
    do {
        pos = s.find('\t', prev);
        if (pos == std::string::npos) pos = s.length();
        out.emplace_back(s.substr(prev, pos - prev));
        prev = pos + 1;
        i++;
    } while (pos < s.length() && prev < s.length() && i < maxCol);
    return out;
}

struct OrgRow {
    int32_t label;  // as the TSV names it
    float score;
    std::string name;
};

// GroupApplier::loadOrgResult (GroupApplier.cpp:55-90); columns 0-based here. stoi / stof on a field
// without a number throw there: refused here.
int load_org_result(const std::string& path, int taxCol, int scoreCol, int nameCol, bool uniform,
                    std::vector<OrgRow>& rows) {
    std::ifstream in(path);
    if (!in.is_open()) { set_error("cannot open " + path); return MTB_ERR_IO; }
    std::string line;
    uint64_t lineNo = 0;
    while (std::getline(in, line)) {
        lineNo++;
        if (line.empty() || line.front() == '#') continue;
        const std::vector<std::string> col = split_tabs(line, 20);
        const int need = std::max(taxCol, std::max(nameCol, uniform ? 0 : scoreCol));
        if (need >= (int)col.size()) {
            set_error(path + " line " + std::to_string(lineNo) + ": column " + std::to_string(need + 1) + " of a row of " +
                      std::to_string(col.size()));
            return MTB_ERR_ARG;
        }
        OrgRow r;
        char* end = nullptr;
        const long t = strtol(col[taxCol].c_str(), &end, 10);
        if (end == col[taxCol].c_str() || t < INT_MIN || t > INT_MAX) {
            set_error(path + " line " + std::to_string(lineNo) + ": no taxID in column " + std::to_string(taxCol + 1));
            return MTB_ERR_ARG;
        }
        r.label = (int32_t)t;
        r.score = 1.0f;
        if (!uniform) {
            r.score = strtof(col[scoreCol].c_str(), &end);
            if (end == col[scoreCol].c_str()) {
                set_error(path + " line " + std::to_string(lineNo) + ": no score in column " + std::to_string(scoreCol + 1));
                return MTB_ERR_ARG;
            }
        }
        r.name = col[nameCol];
        rows.push_back(std::move(r));
    }
    return MTB_OK;
}

// groupMap: "readId \t groupId" per read, in read order (loadGroupsFromFile, GroupApplier.cpp:117-131:
// the k-th pair is read k's, whatever its first field says; reading stops at the first pair that does not parse)
int load_group_map(const std::string& path, std::vector<uint32_t>& gm) {
    std::ifstream in(path);
    if (!in.is_open()) { set_error("cannot open " + path); return MTB_ERR_IO; }
    gm.assign(1, 0);
    std::string id;
    unsigned long long g;
    while (in >> id >> g) {
        if (g >= 0xFFFFFFFFull) {
            set_error(path + ": read " + std::to_string(gm.size()) + " has group ID " + std::to_string(g) + " (2^32 - 1 or more)");
            return MTB_ERR_ARG;
        }
        gm.push_back((uint32_t)g);
    }
    return MTB_OK;
}

// groups: "groupId member member ..." per group, members 1-based; must be groupMap's membership
int check_groups_file(const std::string& path, const std::vector<uint32_t>& gm) {
    std::ifstream in(path);
    if (!in.is_open()) { set_error("cannot open " + path); return MTB_ERR_IO; }
    std::vector<uint8_t> seen(gm.size(), 0);
    std::string line;
    while (std::getline(in, line)) {
        const char* p = line.c_str();
        char* end = nullptr;
        const unsigned long long g = strtoull(p, &end, 10);
        if (end == p) continue;
        p = end;
        for (;;) {
            const unsigned long long q = strtoull(p, &end, 10);
            if (end == p) break;
            p = end;
            if (q == 0 || q >= gm.size() || gm[q] != g || seen[q]) {
                set_error(path + ": read " + std::to_string(q) + " of group " + std::to_string(g) + " is not so in groupMap");
                return MTB_ERR_ARG;
            }
            seen[q] = 1;
        }
    }
    for (size_t q = 1; q < gm.size(); q++)
        if (gm[q] != 0 && !seen[q]) {
            set_error(path + ": read " + std::to_string(q) + " is in group " + std::to_string(gm[q]) + " in groupMap only");
            return MTB_ERR_ARG;
        }
    return MTB_OK;
}

void put_score(std::string& o, float v) {  // ostream << float (%g, 6 significant digits)
    char tmp[48];
    const auto r = std::to_chars(tmp, tmp + sizeof tmp, (double)v, std::chars_format::general, 6);
    o.append(tmp, (size_t)(r.ptr - tmp));
}

}  // namespace

extern "C" {

void mtb_group_apply_default_params(mtb_group_apply_params* par) {  // setGroupApplicationDefaults
    if (!par) return;
    memset(par, 0, sizeof(*par));
    par->weight_mode = 1;
    par->min_vote_score = 0.15f;
}

void mtb_group_apply_constants(uint32_t out[4]) {
    out[0] = kApplySlice;
    out[1] = kApplyThreadLabels;
    out[2] = kApplyWaveLabels;
    out[3] = 0;
}

int mtb_group_apply_lineage_ranks(const mtb_db_host* taxonomy, int32_t* out) {
    if (int rc = check_taxonomy_arg(taxonomy)) return rc;
    if (!out) { set_error("null argument"); return MTB_ERR_ARG; }
    HostTaxonomy T;
    if (!taxonomy_from_host(taxonomy, T)) return MTB_ERR_DB;
    const std::vector<int32_t> lr = lineage_ranks(T);
    memcpy(out, lr.data(), 4 * lr.size());
    return MTB_OK;
}

static int apply_entry(int device, const mtb_db_host* taxonomy, const mtb_group_apply_params* par,
                       const uint32_t* group_map, const int32_t* tax_ids, const float* scores, uint64_t n_reads,
                       uint32_t flags, ApplyIo io, mtb_group_apply_stats* stats) {
    if (int rc = check_apply_params(par)) return rc;
    if (int rc = check_taxonomy_arg(taxonomy)) return rc;
    if (flags & ~(uint32_t)MTB_INPUT_DEVICE) { set_error("a group application takes MTB_INPUT_DEVICE only"); return MTB_ERR_ARG; }
    if (n_reads >= 0xFFFFFFFFull) { set_error("2^32 - 1 reads or more"); return MTB_ERR_ARG; }
    if (!group_map || !io.nGroups) { set_error("null argument"); return MTB_ERR_ARG; }
    if (n_reads && (!tax_ids || (par->weight_mode != 0 && !scores) || !io.outTax || !io.outCls || !io.outApplied)) {
        set_error("null argument");
        return MTB_ERR_ARG;
    }
    if (io.repCap && (!io.repGroup || !io.repTax)) { set_error("null argument"); return MTB_ERR_ARG; }
    HostTaxonomy T;
    if (!taxonomy_from_host(taxonomy, T)) return MTB_ERR_DB;
    io.groupMap = group_map;
    io.taxIds = tax_ids;
    io.scores = scores;
    io.n = n_reads;
    io.devIn = (flags & MTB_INPUT_DEVICE) != 0;
    return apply_core(T, *par, device, io, stats);
}

int mtb_group_apply(int device, const mtb_db_host* taxonomy, const mtb_group_apply_params* par, const uint32_t* group_map,
                    const int32_t* tax_ids, const float* scores, uint64_t n_reads, uint32_t flags, uint32_t* rep_group,
                    int32_t* rep_tax, uint64_t* n_groups, int32_t* out_tax, uint8_t* out_classified, uint8_t* out_applied,
                    mtb_group_apply_stats* stats) {
    ApplyIo io{};
    io.repGroup = rep_group;
    io.repTax = rep_tax;
    io.repCap = n_groups ? *n_groups : 0;
    io.nGroups = n_groups;
    io.outTax = out_tax;
    io.outCls = out_classified;
    io.outApplied = out_applied;
    return apply_entry(device, taxonomy, par, group_map, tax_ids, scores, n_reads, flags, io, stats);
}

int mtb_group_apply_label_sums(int device, const mtb_db_host* taxonomy, const mtb_group_apply_params* par,
                               const uint32_t* group_map, const int32_t* tax_ids, const float* scores, uint64_t n_reads,
                               uint64_t* keys, double* sums, uint64_t cap, uint64_t* n) {
    if (!n || (cap && (!keys || !sums))) { set_error("null argument"); return MTB_ERR_ARG; }
    std::vector<int32_t> outTax(n_reads + 1);
    std::vector<uint8_t> cls(n_reads + 1), app(n_reads + 1);
    std::vector<uint32_t> rg(n_reads + 1);
    std::vector<int32_t> rt(n_reads + 1);
    uint64_t nG = n_reads + 1;
    ApplyIo io{};
    io.repGroup = rg.data();
    io.repTax = rt.data();
    io.repCap = nG;
    io.nGroups = &nG;
    io.outTax = outTax.data();
    io.outCls = cls.data();
    io.outApplied = app.data();
    io.labelKeys = keys;
    io.labelW = sums;
    io.labelCap = cap;
    io.nLabels = n;
    return apply_entry(device, taxonomy, par, group_map, tax_ids, scores, n_reads, 0, io, nullptr);
}

int mtb_group_apply_files(const char* groups_path, const char* groupmap_path, const char* taxonomy_dir,
                          const char* classifications_tsv, const char* out_dir, const mtb_group_apply_params* par,
                          int taxid_col, int score_col, int read_id_col, int device, mtb_group_apply_stats* stats) {
    if (int rc = check_apply_params(par)) return rc;
    if (!groupmap_path || !taxonomy_dir || !classifications_tsv || !out_dir) { set_error("null argument"); return MTB_ERR_ARG; }
    if (taxid_col < 1 || read_id_col < 1 || taxid_col > 20 || read_id_col > 20 || score_col > 20) {
        set_error("column indices are 1-based, within the first 20 columns");
        return MTB_ERR_ARG;
    }
    const bool uniform = par->weight_mode == 0 || score_col < 1;  // GroupApplier.cpp:65
    std::vector<OrgRow> rows;
    if (int rc = load_org_result(classifications_tsv, taxid_col - 1, score_col - 1, read_id_col - 1, uniform, rows)) return rc;
    std::vector<uint32_t> gm;
    if (int rc = load_group_map(groupmap_path, gm)) return rc;
    if (gm.size() - 1 != rows.size()) {
        set_error("groupMap holds " + std::to_string(gm.size() - 1) + " reads, the classifications " + std::to_string(rows.size()));
        return MTB_ERR_ARG;
    }
    if (groups_path)
        if (int rc = check_groups_file(groups_path, gm)) return rc;

    // The taxonomy with internal taxIDs as TaxonomyWrapper(names, nodes, merged, true) numbers them: from
    // 1, in order of first appearance in nodes.dmp, a row's taxID before its parent's
    // (TaxonomyWrapper.cpp:148-195).
    HostTaxonomy E;
    if (!load_dmp(taxonomy_dir, E)) return MTB_ERR_IO;
    const size_t nNodes = E.parent.size();
    std::vector<int32_t> internalOf(nNodes, 0), i2o(1, 0), taxI(nNodes), parI(nNodes);
    for (size_t i = 0; i < nNodes; i++) {
        for (const int x : {(int)i, E.parent[i]})
            if (!internalOf[x]) {
                internalOf[x] = (int32_t)i2o.size();
                i2o.push_back(E.nodeTax[x]);
            }
        taxI[i] = internalOf[i];
        parI[i] = internalOf[E.parent[i]];
    }
    if (internalOf[E.nodeOf[1]] != 1) {
        set_error("nodes.dmp does not begin with the root: its internal taxID would not be 1");
        return MTB_ERR_UNSUPPORTED;
    }
    HostTaxonomy T;
    if (!build_taxonomy(taxI.data(), parI.data(), nNodes, E.rank, E.name, nullptr, nullptr, 0, T)) return MTB_ERR_DB;

    const uint64_t n = rows.size();
    std::vector<int32_t> tax(n + 1, 0), outTax(n + 1);
    std::vector<float> score(n + 1, 1.0f);
    std::vector<uint8_t> cls(n + 1), app(n + 1);
    for (uint64_t r = 0; r < n; r++) {
        const int32_t t = rows[r].label;
        if (t != 0) {
            if (!E.exists(t)) {
                set_error("read " + std::to_string(r + 1) + " (" + rows[r].name + "): label " + std::to_string(t) +
                          " is not in the taxonomy");
                return MTB_ERR_ARG;
            }
            tax[r] = internalOf[E.nodeOf[t]];
        }
        score[r] = rows[r].score;
    }
    std::vector<uint32_t> rg(n + 1);
    std::vector<int32_t> rt(n + 1);
    uint64_t nG = n + 1;
    ApplyIo io{};
    io.groupMap = gm.data();
    io.taxIds = tax.data();
    io.scores = score.data();
    io.n = n;
    io.devIn = false;
    io.repGroup = rg.data();
    io.repTax = rt.data();
    io.repCap = nG;
    io.nGroups = &nG;
    io.outTax = outTax.data();
    io.outCls = cls.data();
    io.outApplied = app.data();
    if (int rc = apply_core(T, *par, device, io, stats)) {
        if (rc == MTB_RETRY) { set_error("more groups than reads"); return MTB_ERR_INTERNAL; }
        return rc;
    }

    const std::string dir = out_dir;
    {   // groupRep: "groupId \t original taxID", groups ascending
        std::string o;
        for (uint64_t j = 0; j < nG; j++) o += std::to_string(rg[j]) + "\t" + std::to_string(i2o[rt[j]]) + "\n";
        FILE* f = fopen((dir + "/groupRep").c_str(), "wb");
        if (!f) { set_error("cannot write " + dir + "/groupRep"); return MTB_ERR_IO; }
        const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
        if (fclose(f) != 0 || !ok) { set_error("cannot write " + dir + "/groupRep"); return MTB_ERR_IO; }
    }
    {   // Reporter::writeReadClassification(queryList, groupIdList) (Reporter.cpp:85-139) without lineage
        std::string o = "#is_classified\tname\ttaxID\tquery_length\tscore\trank\tgroup\ttaxID:match_count\n";
        for (uint64_t r = 0; r < n; r++) {
            const std::string grp = gm[r + 1] ? std::to_string(gm[r + 1]) : "-";
            o += cls[r] ? "1\t" : "0\t";
            o += rows[r].name;
            o += '\t';
            // a read that keeps its label prints it as the TSV named it (getOriginalTaxID of its own internal ID)
            o += std::to_string(cls[r] ? (app[r] ? i2o[outTax[r]] : rows[r].label) : 0);
            o += "\t0\t";
            put_score(o, rows[r].score);
            o += '\t';
            o += cls[r] ? T.rank[T.nodeOf[outTax[r]]] : std::string("-");
            o += '\t';
            o += grp;
            o += cls[r] ? "\t\n" : "\t-\t\n";
        }
        const std::string path = dir + "/updated_classifications.tsv";
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) { set_error("cannot write " + path); return MTB_ERR_IO; }
        const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
        if (fclose(f) != 0 || !ok) { set_error("cannot write " + path); return MTB_ERR_IO; }
    }
    return MTB_OK;
}

}  // extern "C"
