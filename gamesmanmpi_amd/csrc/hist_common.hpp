// hist_common.hpp -- the census of a solved table by value and remoteness (gm_histogram):
// the host-side accumulator every engine's histogram entry fills, the byte-table kernel of the
// dense SUBTRACT engines (its host side: byte_histogram, byte_tables.hpp) and the bin helpers of
// the u16-score tables (sparse tiers, graph).
//
// Byte tables (gm_common.hpp 1-byte codes).  The kernel counts the 256 codes; the host maps
// code -> (value, remoteness) with record_of_code.  A lane loads 16 bytes (one CHUNK) at a
// time.  In both layouts a chunk's 16 bytes differ in the lowest coordinates only, so the
// region test is one 16-bit mask per chunk, never a compare per byte:
//   slot = key           the 16 bytes are heap 0 = 0..15 with heaps 1.. fixed: the chunk is
//                        out if a fixed heap exceeds the root's, else bytes 0..root's heap 0;
//   box << 12 | A << 4 | B   (box_common.hpp) the 16 bytes are B: the parity bits of heaps
//                        4-7.  The A heaps and the B heaps' box coordinates are fixed per
//                        chunk; a B heap on the root's boundary with an even root heap drops
//                        the bytes whose parity bit is set.
// The full lattice (every root heap 15) skips the mask altogether.
//
// Counters: HIST_COPIES = 32 sub-histograms per workgroup in LDS, u32, laid out
// bin * 32 + (lane & 31).  ds_add_u32 is served in two 32-lane groups over 32 banks
// (bank = dword address mod 32), so within a group every lane owns its bank whatever codes
// the lanes hold: the fullest code (6.7 % of the 8-heap table) and the runs of nearby
// remoteness inside a box cost no bank conflict and no same-address serialisation.  The
// workgroup flushes once: thread t sums bin t over the copies and makes at most one global
// atomicAdd (u64), so <= 256 per workgroup.
#pragma once
#include "gm_internal.hpp"

#include <algorithm>

namespace gm {

// counts[value][remoteness], grown on demand
struct Hist {
    std::vector<uint64_t> v[3];
    uint64_t other = 0;   // positions counted that have no row: the DRAW nodes of a loopy graph table
    void add(int value, uint32_t rem, uint64_t n) {
        if (!n) return;
        if (v[value].size() <= rem) v[value].resize(rem + 1, 0);
        v[value][rem] += n;
    }
    void clear() { for (auto &x : v) x.clear(); other = 0; }
    uint32_t n_rem() const { return (uint32_t)std::max({v[0].size(), v[1].size(), v[2].size()}); }
    uint64_t total() const {
        uint64_t s = other;
        for (auto &x : v)
            for (uint64_t k : x) s += k;
        return s;
    }
};

constexpr int HIST_COPIES = 32;
constexpr int HIST_THREADS = 256;
constexpr int HIST_UNROLL = 4;                    // 16-byte loads in flight per lane
constexpr uint32_t HIST_LDS_BUDGET = 48u << 10;   // score bins beyond this go straight to global memory
enum : uint32_t { HIST_ERR_RANGE = 1, HIST_ERR_UNSOLVED = 2 };

namespace {

// the 16-bit mask of the bytes of chunk `c16` (table index >> 4) inside the root's region
template <int BOX>
__host__ __device__ __forceinline__ uint32_t hist_chunk_mask(uint32_t c16, uint32_t root, int heaps) {
    if (BOX) {
        const uint32_t box = c16 >> 8, A = c16 & 255u;
        uint32_t m = 0xFFFFu;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t h = (((box >> (2 * i)) & 3u) << 2) | ((A >> (2 * i)) & 3u);
            if (h > ((root >> (4 * i)) & 15u)) m = 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t c = (box >> (8 + 3 * j)) & 7u, r = (root >> (16 + 4 * j)) & 15u;
            // bytes whose bit j (heap 4 + j's parity) is set
            const uint32_t odd = j == 0 ? 0xAAAAu : j == 1 ? 0xCCCCu : j == 2 ? 0xF0F0u : 0xFF00u;
            if (c > (r >> 1)) m = 0;
            else if (c == (r >> 1) && !(r & 1u)) m &= ~odd;
        }
        return m;
    }
    for (int j = 1; j < heaps; j++)
        if (((c16 >> (4 * (j - 1))) & 15u) > ((root >> (4 * j)) & 15u)) return 0;
    return (2u << (root & 15u)) - 1u;
}

// Census of the codes of a byte table.  The table is walked in chunks of 16 bytes; chunk g
// lies in unit g >> cshift (a unit = 2^cshift chunks that are contiguous in the table: a box,
// a block of the sharded block engine, or the whole table), whose place in the table is
// list[unit] (list == nullptr: the unit's own number).  bins: u64[256], added to.
template <int BOX>
__global__ __launch_bounds__(HIST_THREADS) void byte_hist_kernel(const uint8_t *__restrict__ table,
                                                                 const uint32_t *__restrict__ list, uint64_t nchunks,
                                                                 int cshift, int heaps, uint32_t root, int full,
                                                                 unsigned long long *bins) {
    __shared__ uint32_t cnt[256 * HIST_COPIES];
    for (int i = threadIdx.x; i < 256 * HIST_COPIES; i += HIST_THREADS) cnt[i] = 0;
    __syncthreads();
    uint32_t *mine = cnt + (threadIdx.x & (HIST_COPIES - 1));
    const uint64_t stride = (uint64_t)gridDim.x * HIST_THREADS;
    const uint32_t within = (1u << cshift) - 1u;
    for (uint64_t g0 = blockIdx.x * (uint64_t)HIST_THREADS + threadIdx.x; g0 < nchunks; g0 += HIST_UNROLL * stride) {
        uint4 v[HIST_UNROLL];
        uint32_t m[HIST_UNROLL];
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            const uint64_t g = g0 + u * stride;
            m[u] = 0;
            if (g < nchunks) {
                const uint32_t unit = (uint32_t)(g >> cshift);
                const uint32_t c16 = ((list ? list[unit] : unit) << cshift) | ((uint32_t)g & within);
                m[u] = full ? 0xFFFFu : hist_chunk_mask<BOX>(c16, root, heaps);
                if (m[u]) v[u] = *(const uint4 *)(table + ((uint64_t)c16 << 4));
            }
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            if (!m[u]) continue;
            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            if (m[u] == 0xFFFFu) {
#pragma unroll
                for (int b = 0; b < 16; b++) atomicAdd(mine + (((w[b >> 2] >> (8 * (b & 3))) & 255u) * HIST_COPIES), 1u);
            } else {
#pragma unroll
                for (int b = 0; b < 16; b++)
                    if ((m[u] >> b) & 1u) atomicAdd(mine + (((w[b >> 2] >> (8 * (b & 3))) & 255u) * HIST_COPIES), 1u);
            }
        }
    }
    __syncthreads();
    // thread t owns bin t; the copies are read rotated by t so a wave's lanes spread over the banks
    uint64_t s = 0;
    for (int j = 0; j < HIST_COPIES; j++) s += cnt[threadIdx.x * HIST_COPIES + ((j + threadIdx.x) & (HIST_COPIES - 1))];
    if (s) atomicAdd(bins + threadIdx.x, (unsigned long long)s);
}

// One (score, weight) of a u16-score table into bins[value * nbin + remoteness]: the
// workgroup's LDS copy when it fits (lds != nullptr), else the global u64 array.  A
// remoteness beyond the bins, or an unscored entry, only raises a flag in bins[3 * nbin].
__device__ __forceinline__ void score_bin_add(uint32_t *lds, unsigned long long *bins, uint32_t nbin, uint16_t score,
                                              uint32_t weight) {
    const uint16_t rec = record_of_score(score);
    if (rec == REC_UNSOLVED) { atomicOr(bins + 3 * (uint64_t)nbin, (unsigned long long)HIST_ERR_UNSOLVED); return; }
    const uint32_t val = rec >> 14, rem = rec & 0x3FFFu;
    if (rem >= nbin) { atomicOr(bins + 3 * (uint64_t)nbin, (unsigned long long)HIST_ERR_RANGE); return; }
    if (lds) atomicAdd(lds + val * nbin + rem, weight);
    else atomicAdd(bins + val * nbin + rem, (unsigned long long)weight);
}
__device__ __forceinline__ uint32_t *score_bins_open(uint32_t nbin, int use_lds) {
    extern __shared__ uint32_t hist_lds[];
    if (!use_lds) return nullptr;
    for (uint32_t i = threadIdx.x; i < 3 * nbin; i += blockDim.x) hist_lds[i] = 0;
    __syncthreads();
    return hist_lds;
}
__device__ __forceinline__ void score_bins_flush(const uint32_t *lds, unsigned long long *bins, uint32_t nbin) {
    if (!lds) return;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 3 * nbin; i += blockDim.x)
        if (lds[i]) atomicAdd(bins + i, (unsigned long long)lds[i]);
}

}  // namespace

// ---------------------------------------------------------------- host side
// resident workgroups of byte_hist_kernel on the device: its grid (one generation, no tail)
template <int BOX>
inline unsigned byte_hist_grid(int device) {
    static int cached_dev = -1;
    static unsigned cached = 0;
    if (cached_dev == device) return cached;
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, byte_hist_kernel<BOX>, HIST_THREADS, 0) != hipSuccess ||
        per_cu < 1)
        per_cu = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
    cached_dev = device;
    return cached = (unsigned)(per_cu * cus);
}

// the 256 code counters of one gm_histogram call over byte tables
struct CodeBins {
    unsigned long long *d = nullptr;
};
inline int code_bins_begin(Ctx *c, CodeBins *b) {
    GM_TRY(dev_alloc(c, (void **)&b->d, 256 * 8));
    GM_HIP(hipMemsetAsync(b->d, 0, 256 * 8, c->stream));
    return GM_OK;
}
// units of 2^(ushift) bytes; box layout (BOX = 1) or slot = key over `heaps` heaps (BOX = 0)
template <int BOX>
inline int code_bins_launch(Ctx *c, CodeBins *b, const uint8_t *table, const uint32_t *list, uint64_t nunits, int ushift,
                            int heaps) {
    if (!nunits || !table) return GM_OK;
    if (((uintptr_t)table & 15u) || ushift < 4) { set_error("gm_histogram needs a 16-byte aligned table"); return GM_E_STATE; }
    const uint64_t nchunks = nunits << (ushift - 4);
    const uint32_t root = (uint32_t)c->root;
    const int full = root == (heaps >= 8 ? 0xFFFFFFFFu : (1u << (4 * heaps)) - 1u);
    const uint64_t want = (nchunks + HIST_THREADS - 1) / HIST_THREADS;
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, byte_hist_grid<BOX>(c->device)));
    hipLaunchKernelGGL(byte_hist_kernel<BOX>, dim3(grid), dim3(HIST_THREADS), 0, c->stream, table, list, nchunks,
                       ushift - 4, heaps, root, full, b->d);
    GM_HIP(hipGetLastError());
    return GM_OK;
}
inline int code_bins_end(Ctx *c, CodeBins *b, Hist *out) {
    uint64_t h[256];
    hipError_t e = hipMemcpyAsync(h, b->d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(c, b->d);
    b->d = nullptr;
    GM_HIP(e);
    if (h[0]) { set_error("%llu positions of the region hold no code", (unsigned long long)h[0]); return GM_E_STATE; }
    for (int code = 1; code < 256; code++) {
        const uint16_t rec = record_of_code((uint8_t)code);
        out->add(rec >> 14, rec & 0x3FFFu, h[code]);
    }
    return GM_OK;
}

// the bins of one gm_histogram call over u16-score tables: u64[3 * nbin] and the flag word
struct ScoreBins {
    unsigned long long *d = nullptr;
    uint32_t nbin = 0;
    int use_lds = 0;
    size_t lds_bytes = 0;
};
inline int score_bins_begin(Ctx *c, uint32_t nbin, ScoreBins *b) {
    b->nbin = std::min<uint32_t>(std::max<uint32_t>(nbin, 1), MAX_REMOTENESS + 2);
    b->use_lds = 3ull * b->nbin * 4 <= HIST_LDS_BUDGET;
    b->lds_bytes = b->use_lds ? 3 * (size_t)b->nbin * 4 : 0;
    const uint64_t bytes = (3ull * b->nbin + 1) * 8;
    GM_TRY(dev_alloc(c, (void **)&b->d, bytes));
    GM_HIP(hipMemsetAsync(b->d, 0, bytes, c->stream));
    return GM_OK;
}
// deeper: when given, a remoteness beyond the bins is no error: *deeper is set, `out` is left
// as it was and the caller counts again with more bins
inline int score_bins_end(Ctx *c, ScoreBins *b, Hist *out, bool *deeper = nullptr) {
    std::vector<uint64_t> h(3ull * b->nbin + 1);
    hipError_t e = hipMemcpyAsync(h.data(), b->d, h.size() * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(c, b->d);
    b->d = nullptr;
    GM_HIP(e);
    if (deeper) *deeper = false;
    if (deeper && h.back() == HIST_ERR_RANGE) { *deeper = true; return GM_OK; }
    if (h.back()) {
        if (h.back() & HIST_ERR_UNSOLVED) set_error("the table holds an unscored position");
        else set_error("a remoteness exceeds the %u bins of the census", b->nbin);
        return GM_E_STATE;
    }
    for (int val = 0; val < 3; val++)
        for (uint32_t r = 0; r < b->nbin; r++) out->add(val, r, h[(size_t)val * b->nbin + r]);
    return GM_OK;
}

}  // namespace gm
