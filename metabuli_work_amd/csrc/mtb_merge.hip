// GPU merge of reference DBs: IndexCreator::mergeTargetFiles<DB_CREATION> (IndexCreator.h:322-472),
// what updateDB (updateDB.cpp:134-142) and builds of several flushes (numOfFlush > 1) end with.
//   per input: diffIdx -> 64-bit values (K3's decode_diff_chunk, on-disk form: no rank form here),
//   payload = taxId2speciesId[info & mask] << 32 | info (IndexCreator.h:355,399-400)
//   -> two-way merge-path merges of the two smallest streams until one is left, in
//   compareTargetKmer order (value, species, taxID; Kmer.h:77-87)
//   -> the builder's tail (encode_sorted_kmers, mtb_build.hip): one entry per (value, species) with
//   the LCA of its taxIDs, diffIdx / info, and the split table sized by the k-mer count BEFORE the
//   merge (IndexCreator.h:343), not by the unique count as a single build's (IndexCreator.cpp:819).
// The reference's pass-by-pass buffering (the `max` cut-offs) is a memory device of its own and
// does not change the result; here everything is resident.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mtb_host.h"
#include "mtb_launch.h"

namespace mtb {

constexpr int kMergeFlagNoSpecies = 1, kMergeFlagBit31 = 2;

// payload = species << 32 | taxID (the builder's layout); a taxID without a species in the dense
// table, or an info entry with bit 31 set, raises its flag bit (the host turns it into the error)
__global__ void k_merge_payload(const uint32_t* __restrict__ info, uint64_t n, const int32_t* __restrict__ spOf,
                                uint32_t maxTax, uint32_t mask, uint64_t* __restrict__ pay, int* __restrict__ flag) {
    MTB_GRID_STRIDE(i, n) {
        const uint32_t raw = info[i];
        const uint32_t t = raw & mask;
        const uint32_t sp = t <= maxTax ? (uint32_t)spOf[t] : 0u;
        int f = 0;
        if (raw >> 31) f |= kMergeFlagBit31;
        if (sp == 0) f |= kMergeFlagNoSpecies;
        if (f) atomicOr(flag, f);
        pay[i] = (uint64_t)sp << 32 | t;
    }
}

// (value, payload) order; equal keys take A (the lower-numbered input) first
__device__ __forceinline__ bool kv_le(uint64_t av, uint64_t ap, uint64_t bv, uint64_t bp) {
    return av < bv || (av == bv && ap <= bp);
}

// Merge path: of the first d outputs of merge(A, B), how many come from A. The smallest i with
// A[i] > B[d - i - 1] (ties go to A, so an A item equal to a B item is already counted).
template <typename KA, typename PA, typename KB, typename PB>
__device__ __forceinline__ uint64_t merge_path(const KA& ak, const PA& ap, uint64_t na, const KB& bk, const PB& bp,
                                               uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t i = lo + ((hi - lo) >> 1);
        if (kv_le(ak(i), ap(i), bk(d - i - 1), bp(d - i - 1))) lo = i + 1; else hi = i;
    }
    return lo;
}

// part[t]: A items among the first min(t * kMergeDbTile, nA + nB) outputs, t = 0 .. nTiles
__global__ void k_merge_partition(const uint64_t* __restrict__ aK, const uint64_t* __restrict__ aP, uint64_t nA,
                                  const uint64_t* __restrict__ bK, const uint64_t* __restrict__ bP, uint64_t nB,
                                  uint64_t nTiles, uint64_t* __restrict__ part) {
    MTB_GRID_STRIDE(t, nTiles + 1) {
        const uint64_t d = min(t * (uint64_t)kMergeDbTile, nA + nB);
        part[t] = merge_path([&](uint64_t i) { return aK[i]; }, [&](uint64_t i) { return aP[i]; }, nA,
                             [&](uint64_t i) { return bK[i]; }, [&](uint64_t i) { return bP[i]; }, nB, d);
    }
}

// LDS index of tile item x: one 8-B pad per kMergeDbPer items, so the threads' 8-item stretches
// (the write-back, and the neighbourhood each thread's search and merge read) start 18 dwords apart
// and a 16-lane group's 64-bit accesses fall on distinct banks instead of two
__device__ __forceinline__ uint32_t lds_at(uint32_t x) { return x + (x >> 3); }
constexpr uint32_t kMergeDbLds = kMergeDbTile + kMergeDbTile / 8;

// One workgroup, one tile of kMergeDbTile outputs: its A range [part[b], part[b + 1]) and B range
// (the rest of the tile) load coalesced into LDS (A first, then B), each thread finds its diagonal's
// split there and merges kMergeDbPer items serially into registers, and the tile goes back through
// LDS so the stores are coalesced. 2 x 18 KB of LDS: four workgroups per CU.
__global__ void __launch_bounds__(256) k_merge_tile(const uint64_t* __restrict__ aK, const uint64_t* __restrict__ aP,
                                                    uint64_t nA, const uint64_t* __restrict__ bK,
                                                    const uint64_t* __restrict__ bP, uint64_t nB,
                                                    const uint64_t* __restrict__ part, uint64_t* __restrict__ oK,
                                                    uint64_t* __restrict__ oP) {
    __shared__ uint64_t sK[kMergeDbLds], sP[kMergeDbLds];
    const uint64_t total = nA + nB;
    const uint64_t d0 = (uint64_t)blockIdx.x * kMergeDbTile;
    if (d0 >= total) return;
    const uint64_t d1 = min(d0 + kMergeDbTile, total);
    const uint64_t a0 = part[blockIdx.x], a1 = part[blockIdx.x + 1];
    const uint64_t b0 = d0 - a0;
    const uint32_t n = (uint32_t)(d1 - d0);
    // sorted inputs give a partition monotone in both inputs, so 0 <= a1 - a0 <= n and every read
    // below is inside its array; the clamp and the range test keep an unsorted (invalid) input, whose
    // searches need not be monotone, from reading outside them
    const uint32_t na = a1 > a0 ? (uint32_t)min(a1 - a0, (uint64_t)n) : 0u, nb = n - na;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const bool fromA = i < na;
        const uint64_t g = fromA ? a0 + i : b0 + (i - na);
        const bool in = g < (fromA ? nA : nB);
        sK[lds_at(i)] = !in ? 0ull : fromA ? aK[g] : bK[g];
        sP[lds_at(i)] = !in ? 0ull : fromA ? aP[g] : bP[g];
    }
    __syncthreads();
    const uint32_t d = min(threadIdx.x * kMergeDbPer, n);
    uint32_t i = (uint32_t)merge_path([&](uint64_t x) { return sK[lds_at((uint32_t)x)]; },
                                      [&](uint64_t x) { return sP[lds_at((uint32_t)x)]; }, na,
                                      [&](uint64_t x) { return sK[lds_at(na + (uint32_t)x)]; },
                                      [&](uint64_t x) { return sP[lds_at(na + (uint32_t)x)]; }, nb, d);
    uint32_t j = d - i;
    uint64_t k[kMergeDbPer], p[kMergeDbPer];
    uint64_t ak = 0, ap = 0, bk = 0, bp = 0;
    if (i < na) { ak = sK[lds_at(i)]; ap = sP[lds_at(i)]; }
    if (j < nb) { bk = sK[lds_at(na + j)]; bp = sP[lds_at(na + j)]; }
#pragma unroll
    for (uint32_t q = 0; q < kMergeDbPer; q++) {
        k[q] = 0;
        p[q] = 0;
        if (d + q >= n) continue;
        const bool takeA = j >= nb || (i < na && kv_le(ak, ap, bk, bp));
        if (takeA) {
            k[q] = ak; p[q] = ap;
            i++;
            if (i < na) { ak = sK[lds_at(i)]; ap = sP[lds_at(i)]; }
        } else {
            k[q] = bk; p[q] = bp;
            j++;
            if (j < nb) { bk = sK[lds_at(na + j)]; bp = sP[lds_at(na + j)]; }
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < kMergeDbPer; q++)
        if (d + q < n) { sK[lds_at(d + q)] = k[q]; sP[lds_at(d + q)] = p[q]; }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < n; x += 256) {
        oK[d0 + x] = sK[lds_at(x)];
        oP[d0 + x] = sP[lds_at(x)];
    }
}

void launch_merge_pairs(const uint64_t* aK, const uint64_t* aP, uint64_t nA, const uint64_t* bK, const uint64_t* bP,
                        uint64_t nB, uint64_t* part, uint64_t* oK, uint64_t* oP, hipStream_t s) {
    const uint64_t nTiles = (nA + nB + kMergeDbTile - 1) / kMergeDbTile;
    if (!nTiles) return;
    k_merge_partition<<<stride_grid(nTiles + 1), 256, 0, s>>>(aK, aP, nA, bK, bP, nB, nTiles, part);
    k_merge_tile<<<(unsigned)nTiles, 256, 0, s>>>(aK, aP, nA, bK, bP, nB, part, oK, oP);
}

namespace {

struct DevMem {  // one device allocation, freed on every return
    void* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }
    void reset() {
        if (p) hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(uint64_t bytes) {
        reset();
        return hipMalloc(&p, bytes ? bytes : 8);
    }
    template <typename T>
    T* as() const { return (T*)p; }
};

struct Stream {  // one sorted run of (value, payload) pairs on the device
    std::unique_ptr<DevMem> k, p;
    uint64_t n = 0;
    int first = 0;  // the lowest-numbered input it holds
};

struct MergeRun {  // stream and events of one merge, destroyed on every return
    hipStream_t s = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~MergeRun() {
        if (s) hipStreamSynchronize(s);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (s) hipStreamDestroy(s);
    }
};

float g_mergeMs[5] = {0, 0, 0, 0, 0};

#define HIP_M(x)                                                                                \
    do {                                                                                        \
        hipError_t e_ = (x);                                                                    \
        if (e_ != hipSuccess) {                                                                 \
            set_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x);            \
            return e_ == hipErrorOutOfMemory ? MTB_ERR_OOM : MTB_ERR_HIP;                        \
        }                                                                                       \
    } while (0)

// host to device: through the pinned staging lanes once an array is worth their set-up
int upload(const void* src, void* dst, uint64_t bytes, std::unique_ptr<StageLanes>& lanes, int device, hipStream_t s) {
    if (!bytes) return MTB_OK;
    if (bytes < StageLanes::kChunk && !lanes) {
        HIP_M(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        HIP_M(hipStreamSynchronize(s));
        return MTB_OK;
    }
    if (!lanes) lanes.reset(new StageLanes(device));
    return upload_to_device(src, dst, bytes, lanes.get()) ? MTB_OK : MTB_ERR_IO;
}

// One input's k-mers on the device: values decoded chunk by chunk (the check_db rule rides along:
// the terminal words counted over every chunk must equal n_info), payloads from info.
int load_input(const mtb_merge_input& in, int idx, const int32_t* dSpOf, uint32_t maxTax, uint32_t mask, int* dFlag,
               uint64_t W, DevMem& dDiff, DevMem& dFlagTmp, DevMem& dIdx, DevMem& dTmp, DevMem& dVal,
               std::unique_ptr<StageLanes>& lanes, int device, hipStream_t s, Stream& out) {
    const uint64_t D = in.n_info;
    out.k.reset(new DevMem);
    out.p.reset(new DevMem);
    out.n = D;
    out.first = idx;
    HIP_M(out.k->alloc(8 * D));
    HIP_M(out.p->alloc(8 * D));
    const std::string who = "merge input " + std::to_string(idx);
    uint64_t w0 = 0, k0 = 0, carry = 0, seen = 0;
    while (w0 < in.n_diff_idx) {
        const uint64_t n = std::min(W, in.n_diff_idx - w0);
        if (int rc = upload(in.diff_idx + w0, dDiff.p, 2 * n, lanes, device, s)) return rc;
        uint64_t lastTerm = 0, lastValue = 0;
        const uint64_t terms = decode_diff_chunk(dDiff.as<uint16_t>(), n, carry, dVal.as<uint64_t>(),
                                                 dFlagTmp.as<uint32_t>(), dIdx.as<uint64_t>(), dTmp.p, &lastTerm,
                                                 &lastValue, s);
        HIP_M(hipGetLastError());
        if (terms == 0 || (w0 + n == in.n_diff_idx && lastTerm != n - 1)) {
            set_error(who + ": diffIdx ends mid k-mer");
            return MTB_ERR_DB;
        }
        seen += terms;
        if (seen <= D) {  // counted to the end, written only up to n_info
            HIP_M(hipMemcpyAsync(out.k->as<uint64_t>() + k0, dVal.p, 8 * terms, hipMemcpyDeviceToDevice, s));
            HIP_M(hipStreamSynchronize(s));
            k0 += terms;
        }
        carry = lastValue;
        w0 += lastTerm + 1;
    }
    if (seen != D) {
        set_error(who + ": diffIdx k-mer count " + std::to_string(seen) + " != info entries " + std::to_string(D));
        return MTB_ERR_DB;
    }
    if (D) {
        DevMem dInfo;
        HIP_M(dInfo.alloc(4 * D));
        if (int rc = upload(in.info, dInfo.p, 4 * D, lanes, device, s)) return rc;
        k_merge_payload<<<stride_grid(D), 256, 0, s>>>(dInfo.as<uint32_t>(), D, dSpOf, maxTax, mask, out.p->as<uint64_t>(),
                                                       dFlag);
        HIP_M(hipGetLastError());
        HIP_M(hipStreamSynchronize(s));
    }
    return MTB_OK;
}

int merge_two(const Stream& a, const Stream& b, Stream& out, hipStream_t s) {
    const uint64_t total = a.n + b.n;
    const uint64_t nTiles = (total + kMergeDbTile - 1) / kMergeDbTile;
    out.k.reset(new DevMem);
    out.p.reset(new DevMem);
    out.n = total;
    out.first = std::min(a.first, b.first);
    HIP_M(out.k->alloc(8 * total));
    HIP_M(out.p->alloc(8 * total));
    if (!total) return MTB_OK;
    if (nTiles > 0x7FFFFFFFull) { set_error("merge of more than 2^31 tiles"); return MTB_ERR_UNSUPPORTED; }
    DevMem part;
    HIP_M(part.alloc(8 * (nTiles + 1)));
    // ties take the lower-numbered input first
    const Stream& x = a.first <= b.first ? a : b;
    const Stream& y = a.first <= b.first ? b : a;
    launch_merge_pairs(x.k->as<uint64_t>(), x.p->as<uint64_t>(), x.n, y.k->as<uint64_t>(), y.p->as<uint64_t>(), y.n,
                       part.as<uint64_t>(), out.k->as<uint64_t>(), out.p->as<uint64_t>(), s);
    HIP_M(hipGetLastError());
    HIP_M(hipStreamSynchronize(s));  // part and the inputs are freed by the caller
    return MTB_OK;
}

// Device bytes of a merge of N k-mers (U <= N unique): the merged pairs (16 N) next to the larger of
// the last pass's inputs (16 N) and the tail's arrays: unique values + info (12 U), then group heads +
// indices (12 N) or word counts + offsets (12 U) and the diffIdx words (taken at 4 per k-mer); and
// while the inputs load, their pairs (16 N) next to one decode chunk's temporaries (22 B per word).
uint64_t merge_device_bytes(uint64_t N, uint64_t W) {
    const uint64_t tail = 16 * N + 12 * N + 12 * N + 8 * N;
    const uint64_t load = 16 * N + 4 * N + 22 * W + 8 * scan_tmp_elems(W);
    return std::max(tail, load) + (64ull << 20);
}

// Everything after the argument checks. db: taxonomy, the union taxID list and its species map.
int merge_core(const mtb_merge_input* in, int nIn, const HostDb& db, const mtb_params* par, int splitNum, int device,
               mtb_db_built* out) {
    const HostTaxonomy& T = db.tax;
    uint64_t N = 0, maxWords = 0;
    for (int i = 0; i < nIn; i++) {
        N += in[i].n_info;
        maxWords = std::max(maxWords, in[i].n_diff_idx);
    }
    uint64_t W = 1ull << 27;  // words per decode chunk
    if (const char* e = getenv("MTB_DECODE_CHUNK_WORDS")) W = std::max<uint64_t>(8, strtoull(e, nullptr, 10));
    W = std::max<uint64_t>(std::min(W, maxWords), 1);
    HIP_M(hipSetDevice(device));
    {
        size_t freeB = 0, totalB = 0;
        HIP_M(hipMemGetInfo(&freeB, &totalB));
        const uint64_t need = merge_device_bytes(N, W);
        if (need > freeB) {
            set_error("merge of " + std::to_string(N) + " k-mers needs " + std::to_string(need) +
                      " bytes of device memory, " + std::to_string(freeB) + " are free");
            return MTB_ERR_OOM;
        }
    }
    MergeRun run;
    HIP_M(hipStreamCreateWithFlags(&run.s, hipStreamNonBlocking));
    for (hipEvent_t& e : run.ev) HIP_M(hipEventCreate(&e));
    hipStream_t s = run.s;
    HIP_M(hipEventRecord(run.ev[0], s));

    DevMem dSpOf, dFlag;
    HIP_M(dSpOf.alloc(4 * db.speciesOf.size()));
    HIP_M(hipMemcpyAsync(dSpOf.p, db.speciesOf.data(), 4 * db.speciesOf.size(), hipMemcpyHostToDevice, s));
    HIP_M(dFlag.alloc(4));
    HIP_M(hipMemsetAsync(dFlag.p, 0, 4, s));
    const uint32_t mask = ~((uint32_t)(par->skip_redundancy == 0) << 31);
    std::vector<Stream> streams((size_t)nIn);
    {
        DevMem dDiff, dFlagTmp, dIdx, dTmp, dVal;  // one chunk's temporaries, shared by the inputs
        HIP_M(dDiff.alloc(2 * W));
        HIP_M(dFlagTmp.alloc(4 * W));
        HIP_M(dIdx.alloc(8 * (W + 2)));
        HIP_M(dTmp.alloc(8 * scan_tmp_elems(W)));
        HIP_M(dVal.alloc(8 * W));
        std::unique_ptr<StageLanes> lanes;
        for (int i = 0; i < nIn; i++)
            if (int rc = load_input(in[i], i, dSpOf.as<int32_t>(), (uint32_t)T.maxTax, mask, dFlag.as<int>(), W, dDiff,
                                    dFlagTmp, dIdx, dTmp, dVal, lanes, device, s, streams[(size_t)i]))
                return rc;
        int flag = 0;
        HIP_M(hipMemcpyAsync(&flag, dFlag.p, 4, hipMemcpyDeviceToHost, s));
        HIP_M(hipStreamSynchronize(s));
        if (flag & kMergeFlagBit31) {
            set_error("an info entry has bit 31 set (a redundancy flag no builder here writes)");
            return MTB_ERR_UNSUPPORTED;
        }
        if (flag & kMergeFlagNoSpecies) {
            set_error("an info entry's taxID has no species in the union taxID list's map");
            return MTB_ERR_DB;
        }
    }
    HIP_M(hipEventRecord(run.ev[1], s));
    // k-way: the two smallest streams merge until one is left (an update is one pass over the old DB)
    while (streams.size() > 1) {
        std::sort(streams.begin(), streams.end(), [](const Stream& a, const Stream& b) {
            return a.n != b.n ? a.n < b.n : a.first < b.first;
        });
        Stream m;
        if (int rc = merge_two(streams[0], streams[1], m, s)) return rc;
        streams.erase(streams.begin(), streams.begin() + 2);  // frees the two inputs
        streams.push_back(std::move(m));
    }
    HIP_M(hipEventRecord(run.ev[2], s));
    if (int rc = encode_sorted_kmers(streams[0].k->as<uint64_t>(), streams[0].p->as<uint64_t>(), N, T, splitNum, N,
                                     false, par->kmer_format, nullptr, run.ev[3], s, out))
        return rc;
    HIP_M(hipEventRecord(run.ev[4], s));
    HIP_M(hipStreamSynchronize(s));
    out->n_taxid_list = db.taxIdList.size();
    out->taxid_list = (int32_t*)malloc(4 * db.taxIdList.size() + 4);
    memcpy(out->taxid_list, db.taxIdList.data(), 4 * db.taxIdList.size());
    for (int k = 0; k < 4; k++) HIP_M(hipEventElapsedTime(&g_mergeMs[k], run.ev[k], run.ev[k + 1]));
    HIP_M(hipEventElapsedTime(&g_mergeMs[4], run.ev[0], run.ev[4]));
    return MTB_OK;
}

// Host checks of the inputs shared by both entry points (after their own argument checks); sorts
// and uniques db's taxID list and builds its species map.
int check_merge_args(const mtb_merge_input* in, int nIn, const mtb_params* par, HostDb& db) {
    for (int i = 0; i < nIn; i++) {
        if ((in[i].n_diff_idx && !in[i].diff_idx) || (in[i].n_info && !in[i].info)) {
            set_error("merge input " + std::to_string(i) + " has a null array");
            return MTB_ERR_ARG;
        }
        if ((in[i].n_diff_idx == 0) != (in[i].n_info == 0)) {
            set_error("merge input " + std::to_string(i) + ": one of diffIdx and info is empty");
            return MTB_ERR_DB;
        }
        if (in[i].n_diff_idx && !(in[i].diff_idx[in[i].n_diff_idx - 1] & 0x8000u)) {
            set_error("merge input " + std::to_string(i) + ": diffIdx ends mid k-mer");
            return MTB_ERR_DB;
        }
    }
    if (par->reduced_aa) { set_error("reduced-AA DBs are out of scope"); return MTB_ERR_UNSUPPORTED; }
    if (par->kmer_format != 1 && par->kmer_format != 2) { set_error("kmer_format must be 1 or 2"); return MTB_ERR_UNSUPPORTED; }
    std::sort(db.taxIdList.begin(), db.taxIdList.end());
    db.taxIdList.erase(std::unique(db.taxIdList.begin(), db.taxIdList.end()), db.taxIdList.end());
    if (!build_species_map(db)) return MTB_ERR_DB;  // updateTaxId2SpeciesTaxId over the union list
    return MTB_OK;
}

template <typename T>
bool slurp(const std::string& path, std::vector<T>& out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamoff bytes = f.tellg();
    out.resize((size_t)bytes / sizeof(T));
    f.seekg(0);
    return out.empty() || (bool)f.read((char*)out.data(), (std::streamsize)(out.size() * sizeof(T)));
}

bool read_parameters(const std::string& dir, std::map<std::string, std::string>& kv) {
    std::ifstream f(dir + "/db.parameters");
    if (!f) return false;
    std::string line;
    while (std::getline(f, line)) {
        const size_t tab = line.find('\t');
        if (tab != std::string::npos) kv[line.substr(0, tab)] = line.substr(tab + 1);
    }
    return true;
}

bool write_array(const std::string& path, const void* p, uint64_t bytes) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) return false;
    if (bytes) f.write((const char*)p, (std::streamsize)bytes);
    return (bool)f;
}

}  // namespace
}  // namespace mtb

using namespace mtb;

extern "C" {

int mtb_merge_db(const mtb_merge_input* in, int n_in, const int32_t* taxid_list, uint64_t n_taxid_list,
                 const mtb_db_host* taxo, const mtb_params* par, int split_num, int device, mtb_db_built* out) {
    if (!taxo || !out || (n_taxid_list && !taxid_list)) { set_error("null argument"); return MTB_ERR_ARG; }
    memset(out, 0, sizeof(*out));
    // the arguments first: a bad call returns before the taxonomy is built and before any device call
    if (!in || !par) { set_error("null argument"); return MTB_ERR_ARG; }
    if (n_in < 1 || n_in > 64) { set_error("a merge takes 1 to 64 inputs"); return MTB_ERR_ARG; }
    if (split_num < 2) { set_error("split_num must be at least 2"); return MTB_ERR_ARG; }
    HostDb db;
    {
        if (!taxo->node_taxid || !taxo->node_parent || !taxo->rank_pool || !taxo->rank_off) {
            set_error("null taxonomy arrays");
            return MTB_ERR_ARG;
        }
        std::vector<std::string> ranks(taxo->n_nodes), names(taxo->n_nodes);
        for (uint64_t i = 0; i < taxo->n_nodes; i++) {
            ranks[i] = taxo->rank_pool + taxo->rank_off[i];
            if (taxo->name_pool) names[i] = taxo->name_pool + taxo->name_off[i];
        }
        if (!build_taxonomy(taxo->node_taxid, taxo->node_parent, taxo->n_nodes, ranks, names, taxo->merged_old,
                            taxo->merged_new, taxo->n_merged, db.tax))
            return MTB_ERR_DB;
    }
    db.taxIdList.assign(taxid_list, taxid_list + n_taxid_list);
    if (int rc = check_merge_args(in, n_in, par, db)) return rc;
    const int rc = merge_core(in, n_in, db, par, split_num, device, out);
    if (rc != MTB_OK) mtb_free_built(out);
    return rc;
}

int mtb_merge_db_dirs(const char* const* dirs, int n_dirs, const char* out_dir, int split_num, int device) {
    namespace fs = std::filesystem;
    if (!dirs || !out_dir) { set_error("null argument"); return MTB_ERR_ARG; }
    if (n_dirs < 1 || n_dirs > 64) { set_error("a merge takes 1 to 64 inputs"); return MTB_ERR_ARG; }
    if (split_num < 2) { set_error("split_num must be at least 2"); return MTB_ERR_ARG; }
    for (int i = 0; i < n_dirs; i++)
        if (!dirs[i]) { set_error("null directory"); return MTB_ERR_ARG; }
    // db.parameters: the DBs must hold the same kind of k-mer
    std::map<std::string, std::string> kv0;
    for (int i = 0; i < n_dirs; i++) {
        std::map<std::string, std::string> kv;
        if (!read_parameters(dirs[i], kv)) { set_error(std::string("cannot read ") + dirs[i] + "/db.parameters"); return MTB_ERR_IO; }
        if (i == 0) { kv0 = kv; continue; }
        for (const char* key : {"Kmer_format", "Syncmer", "Reduced_alphabet", "Accession_level"})
            if (kv[key] != kv0[key]) {
                set_error(std::string(dirs[i]) + "/db.parameters: " + key + " '" + kv[key] + "' differs from '" + kv0[key] +
                          "' of " + dirs[0]);
                return MTB_ERR_ARG;
            }
    }
    mtb_params par;
    mtb_default_params(&par);
    mtb_load_db_parameters(dirs[0], &par);
    // the files
    std::vector<std::vector<uint16_t>> diffs((size_t)n_dirs);
    std::vector<std::vector<uint32_t>> infos((size_t)n_dirs);
    std::vector<mtb_merge_input> in((size_t)n_dirs);
    HostDb db;
    for (int i = 0; i < n_dirs; i++) {
        const std::string d = dirs[i];
        if (!slurp(d + "/diffIdx", diffs[(size_t)i])) { set_error("cannot read " + d + "/diffIdx"); return MTB_ERR_IO; }
        if (!slurp(d + "/info", infos[(size_t)i])) { set_error("cannot read " + d + "/info"); return MTB_ERR_IO; }
        std::ifstream tl(d + "/taxID_list");
        if (!tl) { set_error("cannot read " + d + "/taxID_list"); return MTB_ERR_IO; }
        std::string line;
        while (std::getline(tl, line))
            if (!line.empty()) db.taxIdList.push_back((int32_t)std::stoul(line));
        in[(size_t)i] = mtb_merge_input{diffs[(size_t)i].data(), diffs[(size_t)i].size(), infos[(size_t)i].data(),
                                        infos[(size_t)i].size()};
    }
    // loadTaxonomy (common.cpp:50-86) of dirs[0]
    const std::string d0 = dirs[0];
    const bool haveTaxDb = std::ifstream(d0 + "/taxonomyDB").good();
    int trc = 1;
    if (haveTaxDb) trc = load_taxonomy_db(d0 + "/taxonomyDB", db.tax);
    if (trc < 0) return MTB_ERR_IO;
    if (trc == 1 && !load_dmp(d0 + "/taxonomy", db.tax)) return MTB_ERR_IO;
    if (int rc = check_merge_args(in.data(), n_dirs, &par, db)) return rc;
    mtb_db_built out;
    memset(&out, 0, sizeof(out));
    int rc = merge_core(in.data(), n_dirs, db, &par, split_num, device, &out);
    if (rc == MTB_OK) {
        const std::string o = out_dir;
        std::error_code ec;
        fs::create_directories(o, ec);
        bool ok = write_array(o + "/diffIdx", out.diff_idx, 2 * out.n_diff_idx) &&
                  write_array(o + "/info", out.info, 4 * out.n_info) &&
                  write_array(o + "/split", out.split, 24 * out.n_split);
        std::string ids;
        for (uint64_t i = 0; i < out.n_taxid_list; i++) ids += std::to_string(out.taxid_list[i]) + "\n";
        ok = ok && write_array(o + "/taxID_list", ids.data(), ids.size());
        const auto opt = fs::copy_options::overwrite_existing | fs::copy_options::recursive;
        if (ok && !fs::equivalent(d0, o, ec)) {
            ec.clear();
            fs::copy_file(d0 + "/db.parameters", o + "/db.parameters", fs::copy_options::overwrite_existing, ec);
            if (!ec && haveTaxDb) fs::copy_file(d0 + "/taxonomyDB", o + "/taxonomyDB", fs::copy_options::overwrite_existing, ec);
            if (!ec && fs::is_directory(d0 + "/taxonomy")) fs::copy(d0 + "/taxonomy", o + "/taxonomy", opt, ec);
            if (!ec && fs::exists(d0 + "/acc2taxid.map"))
                fs::copy_file(d0 + "/acc2taxid.map", o + "/acc2taxid.map", fs::copy_options::overwrite_existing, ec);
            ok = !ec;
        }
        if (!ok) {
            set_error("cannot write the merged DB to " + o);
            rc = MTB_ERR_IO;
        }
    }
    mtb_free_built(&out);
    return rc;
}

int mtb_merge_last_ms(float* ms, int n) {
    if (!ms || n < 0) { set_error("null argument"); return MTB_ERR_ARG; }
    const int k = std::min(n, 5);
    for (int i = 0; i < k; i++) ms[i] = g_mergeMs[i];
    return k;
}

uint32_t mtb_merge_tile_items(void) { return kMergeDbTile; }

}  // extern "C"
