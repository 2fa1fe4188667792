// select_common.hpp -- the positions of a solved table with a wanted value and a remoteness in
// range (gm_select): the device accumulator every engine's select entry appends to, the predicate,
// the wave-aggregated append and the byte-table kernel of the dense SUBTRACT engines (its host
// side: byte_select, byte_tables.hpp).
//
// A selection is the census pass (hist_common.hpp) with a predicate and a compacted output.
// Accumulator: u64 words [0] matches, [1] the list's cursor; the list is `cap` keys and `cap`
// records.  A filter may match nothing or everything, so nothing is paid per match beyond its
// store:
//   count    a thread counts its matches in a register; the workgroup adds them once (block_add);
//   append   places are reserved per wave: a ballot (byte tables: a scan of the lanes' match
//            counts, up to 16 per lane and chunk), then ONE atomicAdd on the cursor for all the
//            wave's matches, each lane storing at base + its rank.  Atomics on one address
//            serialise (sparse_common.hpp block_add), so a match-everything filter reserving
//            per match would run at the atomic rate, not the memory rate;
//   the cap  a wave whose reservation starts at or past the list's capacity stops reserving
//            and only counts from then on: past the cap the pass costs what the census costs.
//            Every store is guarded by `at < cap`, so none lands beyond the list.
// No LDS staging (graph_loopy.hip WaveStage): there a wave appends a few entries per ballot to
// a queue that takes every entry; here a narrow filter makes almost no reservations, and a wide
// one fills the list and closes its waves after one or two reservations each -- the steady
// state has no atomics either way, so a stage would only add LDS traffic to the match path.
// The list is unordered; gm_api.hip sorts what it copied back.
#pragma once
#include "verify_common.hpp"

namespace gm {

constexpr int SEL_WORDS = 2;                    // match count and cursor before the list
constexpr uint64_t SEL_FIRST_CAP = 1u << 16;    // keys kept by the first pass (gm_api.hip runs a second when more are asked for)
constexpr int SEL_THREADS = 256;
constexpr int SEL_UNROLL = 4;                   // 16-byte loads in flight per lane

struct SelectDev {
    unsigned long long *acc;   // SEL_WORDS words
    void *keys;                // cap keys: uint64_t, or K128 on a wide context
    uint16_t *recs;            // cap records
    uint64_t cap;
    uint32_t values, rem_lo, rem_hi;   // gm_select_t
    uint32_t codes[8];         // byte tables: the set of the 1-byte codes that match, bit c of word c >> 5
};

// the predicate: a record that is there, of a wanted value, with a remoteness in range.  DRAW
// (0xC000, a loopy graph table's) is value code 3 with remoteness 0
GM_HD bool select_match(uint32_t values, uint32_t rem_lo, uint32_t rem_hi, uint16_t rec) {
    if (rec == REC_UNSOLVED) return false;
    const uint32_t val = rec >> 14, rem = rec & 0x3FFFu;
    return ((values >> val) & 1u) && rem >= rem_lo && rem <= rem_hi;
}

namespace {

struct SelectTally {
    uint64_t n = 0;     // this thread's matches
    bool open = true;   // this lane still reserves places
};

// One candidate per lane; any subset of a wave's lanes may call it together (the orbit loops
// of the sparse kernels diverge), so the leader is the first lane that takes part.
template <class K>
__device__ __forceinline__ void select_note(const SelectDev &s, SelectTally &t, bool got, const K &key, uint16_t rec) {
    t.n += got;
    const unsigned long long m = __ballot(got && t.open);
    if (!(got && t.open)) return;
    const int lane = threadIdx.x & 63, leader = __ffsll(m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(s.acc + 1, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    if (base >= s.cap) { t.open = false; return; }
    const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (at < s.cap) {
        ((K *)s.keys)[at] = key;
        s.recs[at] = rec;
    }
}
// every thread of the workgroup, once, at the kernel's end
__device__ __forceinline__ void select_flush(const SelectDev &s, const SelectTally &t) { block_add(s.acc, t.n); }

// bit `code` of the 256-bit set: the eight words are kernel arguments (wave-uniform), picked by
// a three-level select on the code's top bits
__device__ __forceinline__ uint32_t select_code_hit(const SelectDev &s, uint32_t code) {
    const uint32_t a0 = (code & 32u) ? s.codes[1] : s.codes[0], a1 = (code & 32u) ? s.codes[3] : s.codes[2];
    const uint32_t a2 = (code & 32u) ? s.codes[5] : s.codes[4], a3 = (code & 32u) ? s.codes[7] : s.codes[6];
    const uint32_t b0 = (code & 64u) ? a1 : a0, b1 = (code & 64u) ? a3 : a2;
    return (((code & 128u) ? b1 : b0) >> (code & 31u)) & 1u;
}

// Selection over a byte table, walked as byte_hist_kernel walks it (hist_common.hpp): chunks of
// 16 bytes, chunk g in unit g >> cshift placed by list[unit], one hist_chunk_mask per chunk, the
// full lattice without it.  The loop runs per wave (every lane of a wave makes the same trips),
// so the ballot and the scan below see all 64 lanes.  A match's key is its table index, through
// box_key_of_index in the box layout; its record is record_of_code.
template <int BOX>
__global__ __launch_bounds__(SEL_THREADS) void byte_select_kernel(const uint8_t *__restrict__ table,
                                                                  const uint32_t *__restrict__ list, uint64_t nchunks,
                                                                  int cshift, int heaps, uint32_t root, int full,
                                                                  SelectDev s) {
    SelectTally t;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * SEL_THREADS;
    const uint32_t within = (1u << cshift) - 1u;
    for (uint64_t w0 = blockIdx.x * (uint64_t)SEL_THREADS + (threadIdx.x & ~63u); w0 < nchunks; w0 += SEL_UNROLL * stride) {
        uint4 v[SEL_UNROLL];
        uint32_t m[SEL_UNROLL], at16[SEL_UNROLL];
#pragma unroll
        for (int u = 0; u < SEL_UNROLL; u++) {
            const uint64_t g = w0 + lane + u * stride;
            m[u] = 0;
            at16[u] = 0;
            if (g < nchunks) {
                const uint32_t unit = (uint32_t)(g >> cshift);
                const uint32_t c16 = ((list ? list[unit] : unit) << cshift) | ((uint32_t)g & within);
                at16[u] = c16;
                m[u] = full ? 0xFFFFu : hist_chunk_mask<BOX>(c16, root, heaps);
                if (m[u]) v[u] = *(const uint4 *)(table + ((uint64_t)c16 << 4));
            }
        }
#pragma unroll
        for (int u = 0; u < SEL_UNROLL; u++) {
            uint32_t hit = 0;
            if (m[u]) {
                const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int b = 0; b < 16; b++) hit |= select_code_hit(s, (w[b >> 2] >> (8 * (b & 3))) & 255u) << b;
                hit &= m[u];
            }
            const uint32_t cnt = (uint32_t)__popc(hit);
            t.n += cnt;
            if (!__ballot(hit != 0u) || !t.open) continue;   // both the same in every lane
            // the lanes' counts scanned, one reservation for the wave
            uint32_t incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                if (lane >= (uint32_t)o) incl += up;
            }
            const uint32_t total = (uint32_t)__shfl((int)incl, 63);
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(s.acc + 1, (unsigned long long)total);
            base = __shfl(base, 0);
            if (base >= s.cap) { t.open = false; continue; }
            uint64_t at = base + incl - cnt;
            for (uint32_t left = hit; left; left &= left - 1u, at++) {
                if (at >= s.cap) break;
                const uint32_t b = (uint32_t)__ffs((int)left) - 1u;
                const uint32_t word = b < 4 ? v[u].x : b < 8 ? v[u].y : b < 12 ? v[u].z : v[u].w;
                const uint32_t idx = (at16[u] << 4) | b;
                ((uint64_t *)s.keys)[at] = BOX ? box_key_of_index(idx) : idx;
                s.recs[at] = record_of_code((uint8_t)(word >> (8 * (b & 3u))));
            }
        }
    }
    select_flush(s, t);
}

}  // namespace

// ---------------------------------------------------------------- host side
// units of 2^ushift bytes; box layout (BOX = 1) or slot = key over `heaps` heaps (BOX = 0):
// code_bins_launch's arguments.  At most 2,048 workgroups (grid_counted): one generation, and
// the match counter sees one atomic per workgroup.
template <int BOX>
inline int byte_select_launch(Ctx *c, const SelectDev &s, const uint8_t *table, const uint32_t *list, uint64_t nunits,
                              int ushift, int heaps) {
    if (!nunits || !table) return GM_OK;
    if (((uintptr_t)table & 15u) || ushift < 4) { set_error("gm_select needs a 16-byte aligned table"); return GM_E_STATE; }
    const uint64_t nchunks = nunits << (ushift - 4);
    const uint32_t root = (uint32_t)c->root;
    const int full = root == (heaps >= 8 ? 0xFFFFFFFFu : (1u << (4 * heaps)) - 1u);
    hipLaunchKernelGGL(byte_select_kernel<BOX>, dim3(grid_counted(nchunks)), dim3(SEL_THREADS), 0, c->stream, table, list,
                       nchunks, ushift - 4, heaps, root, full, s);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// one gm_select pass: the accumulator and a list with room for `cap` keys of `key_bytes` each
struct SelectRun {
    SelectDev dev{};
    uint64_t key_bytes = 8;
};
inline int select_begin(Ctx *c, const gm_select_t &what, uint64_t cap, uint64_t key_bytes, SelectRun *r) {
    r->key_bytes = key_bytes;
    SelectDev &d = r->dev;
    d.cap = cap;
    d.values = what.values;
    d.rem_lo = what.rem_lo;
    d.rem_hi = std::min<uint32_t>(what.rem_hi, 0x3FFFu);
    // the filter as a set of 1-byte codes (a TIE, a DRAW, a remoteness past 126 has none)
    for (uint32_t &w : d.codes) w = 0;
    for (uint32_t val : {(uint32_t)WIN, (uint32_t)LOSS})
        for (uint32_t rem = d.rem_lo; rem <= std::min<uint32_t>(d.rem_hi, 126u) && ((d.values >> val) & 1u); rem++) {
            const int code = code_of_record((uint16_t)(val << 14 | rem));
            if (code > 0) d.codes[code >> 5] |= 1u << (code & 31);
        }
    // acc (16 bytes), the keys (16-byte aligned for K128), the records
    GM_TRY(dev_alloc(c, (void **)&d.acc, SEL_WORDS * 8 + cap * key_bytes + cap * 2));
    d.keys = d.acc + SEL_WORDS;
    d.recs = (uint16_t *)((unsigned char *)d.keys + cap * key_bytes);
    GM_HIP(hipMemsetAsync(d.acc, 0, SEL_WORDS * 8, c->stream));
    return GM_OK;
}
// *n = matches; the keys and records written (raw, unsorted) into keys / recs
inline int select_end(Ctx *c, SelectRun *r, uint64_t *n, std::vector<unsigned char> *keys, std::vector<uint16_t> *recs) {
    uint64_t h[SEL_WORDS];
    hipError_t e = hipMemcpyAsync(h, r->dev.acc, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) {
        const uint64_t m = std::min<uint64_t>(h[0], r->dev.cap);
        keys->resize(m * r->key_bytes);
        recs->resize(m);
        if (m) e = hipMemcpyAsync(keys->data(), r->dev.keys, m * r->key_bytes, hipMemcpyDeviceToHost, c->stream);
        if (m && e == hipSuccess) e = hipMemcpyAsync(recs->data(), r->dev.recs, m * 2, hipMemcpyDeviceToHost, c->stream);
        if (m && e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    dev_free(c, r->dev.acc);
    r->dev.acc = nullptr;
    GM_HIP(e);
    *n = h[0];
    return GM_OK;
}

}  // namespace gm
