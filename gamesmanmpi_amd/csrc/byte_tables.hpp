// byte_tables.hpp -- the host read side of the four engines that hold the subtraction game as
// 1-byte codes (gm_common.hpp): dense_sub (block engine), dense_box (box engine) and their
// splits over ranks, dist_sub and dist_box.  What sparse_tables.hpp is to the two sparse engines.
//
// An engine describes its tables once, in the view function its Engine record names (`bytes`);
// query, digest, histogram, select, verify, moves and poke are written here against that
// description alone, and the four records name these functions.  The kernels of the analysis
// passes stay where they are (hist_common.hpp, select_common.hpp, verify_common.hpp,
// moves_common.hpp); the query and digest kernels are below.
#pragma once
#include "gm_internal.hpp"
#include "hist_common.hpp"
#include "verify_common.hpp"
#include "select_common.hpp"
#include "moves_common.hpp"
#include "reach_common.hpp"

#include <type_traits>

namespace gm {

// One entry of d_tables: a table and the units of it this context computed.  A part with no
// units or no table (a rank of a multi-process solve that holds nothing) is skipped.
struct BytePart {
    uint8_t *table;         // the host's copy of the device pointer d_tables[i]
    const uint32_t *list;   // device: the units' places in the table (nullptr: units 0 .. nunits - 1)
    uint64_t nunits;
};

struct ByteTables {
    int box = 0;       // table index: 0 the key itself, 1 box_index_of_key(key) (box_common.hpp)
    int heaps = 0;
    int ushift = 0;    // a unit is 2^ushift contiguous bytes: the whole table, a block, a 4 KiB box
    int oshift = 0;    // key layout: d_owner is indexed by key >> oshift (box layout: by box id)
    // code 0 inside the region is a position the table does not hold (an imported table with
    // holes, dense_sub only): digest skips it.  The other engines fill their region and count it.
    bool skip_empty = false;
    const uint8_t *const *d_tables = nullptr;   // device: one table pointer per part
    const uint8_t *d_owner = nullptr;           // device: the part holding a unit, 0xFF none (nullptr: part 0 holds all)
    std::vector<BytePart> parts;
};

inline ByteTables byte_tables_of(Ctx *c) {
    ByteTables t;
    c->solved_by->bytes(c, &t);
    return t;
}
// f(std::integral_constant<int, BOX>) for the tables' layout: the kernels take it as a template argument
template <class F>
inline int byte_layout(const ByteTables &t, F &&f) {
    return t.box ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}

namespace {

// Records of keys.  REC_UNSOLVED for a key that is no position, one outside the root's region
// (its slot may hold an earlier solve's code, include/gmsolve.h gm_query) and one whose unit no
// table of this context holds.
template <int BOX>
__global__ __launch_bounds__(256) void byte_query_kernel(const uint8_t *const *__restrict__ tables,
                                                         const uint8_t *__restrict__ owner, int oshift, int heaps,
                                                         uint64_t root, const uint64_t *__restrict__ keys,
                                                         uint16_t *__restrict__ out, uint64_t n) {
    const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    uint32_t code = 0;
    if (sub_in_region(k, root, heaps))
        code = byte_code_at<BOX>(tables, owner, oshift, BOX ? box_index_of_key((uint32_t)k) : (uint32_t)k);
    out[i] = record_of_code((uint8_t)code);
}

// Digest of the region's positions in `nunits` units of one table: acc[0] += the terms (a
// wrapping sum, so the walk's order does not matter), acc[1] += their number.  The walk is
// bound by its instructions (2^32 positions: 11 ms), so the two tests that do not change from
// one position to the next are template arguments of its loop: LISTED is list != nullptr,
// SKIP is skip_empty.
template <int BOX, bool LISTED, bool SKIP>
__device__ __forceinline__ void byte_digest_walk(const uint8_t *__restrict__ table, const uint32_t *__restrict__ list,
                                                 uint64_t nunits, int ushift, int heaps, uint64_t root, uint64_t &sum,
                                                 uint64_t &cnt) {
    const uint64_t total = nunits << ushift;
    const uint32_t within = ushift < 32 ? (1u << ushift) - 1u : ~0u;
    for (uint64_t x = blockIdx.x * 256ull + threadIdx.x; x < total; x += (uint64_t)gridDim.x * 256ull) {
        const uint32_t unit = (uint32_t)(x >> ushift), place = LISTED ? list[unit] : unit;
        const uint32_t idx = (ushift < 32 ? place << ushift : 0u) | ((uint32_t)x & within);
        const uint32_t k = BOX ? box_key_of_index(idx) : idx;
        if (!sub_in_region(k, root, heaps)) continue;
        const uint8_t code = table[idx];
        if (SKIP && !code) continue;
        sum += digest_term(k, record_of_code(code));
        cnt++;
    }
}

template <int BOX>
__global__ __launch_bounds__(256) void byte_digest_kernel(const uint8_t *__restrict__ table,
                                                          const uint32_t *__restrict__ list, uint64_t nunits,
                                                          int ushift, int heaps, uint64_t root, int skip_empty,
                                                          unsigned long long *acc) {
    if (BOX) heaps = 8, ushift = 12;   // the box layout is the 8-heap game's in 4 KiB boxes: constants for the walk
    uint64_t sum = 0, cnt = 0;
    if (list && skip_empty) byte_digest_walk<BOX, true, true>(table, list, nunits, ushift, heaps, root, sum, cnt);
    else if (list) byte_digest_walk<BOX, true, false>(table, list, nunits, ushift, heaps, root, sum, cnt);
    else if (skip_empty) byte_digest_walk<BOX, false, true>(table, list, nunits, ushift, heaps, root, sum, cnt);
    else byte_digest_walk<BOX, false, false>(table, list, nunits, ushift, heaps, root, sum, cnt);
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        cnt += __shfl_xor(cnt, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(acc, (unsigned long long)sum);
        atomicAdd(acc + 1, (unsigned long long)cnt);
    }
}

// ---------------------------------------------------------------- the readers
// (in the unnamed namespace with the kernels they launch: every engine's translation unit has its own)
int byte_query(Ctx *c, const void *keys_in, uint16_t *recs, uint64_t n) {
    const uint64_t *keys = (const uint64_t *)keys_in;
    const ByteTables t = byte_tables_of(c);
    const auto kernel = t.box ? byte_query_kernel<1> : byte_query_kernel<0>;
    return query_keys(c, keys, recs, n, BOX_QUERY_CHUNK, [&](const uint64_t *dk, uint16_t *dr, uint64_t m) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, t.d_tables, t.d_owner,
                           t.oshift, t.heaps, c->root, dk, dr, m);
    });
}

// Every part into one accumulator: the whole region over one table or all virtual ranks, this
// rank's share in a multi-process solve (the shares sum to the whole).
int byte_digest(Ctx *c, uint64_t *digest, uint64_t *n) {
    const ByteTables t = byte_tables_of(c);
    const auto kernel = t.box ? byte_digest_kernel<1> : byte_digest_kernel<0>;
    unsigned long long *acc = nullptr, h[2];
    GM_TRY(dev_alloc(c, (void **)&acc, 16));
    hipError_t e = hipMemsetAsync(acc, 0, 16, c->stream);
    for (const BytePart &p : t.parts) {
        if (!p.table || !p.nunits) continue;
        const uint64_t want = ((p.nunits << t.ushift) + 255) / 256;
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<uint64_t>(want, 4096)), dim3(256), 0, c->stream, p.table,
                           p.list, p.nunits, t.ushift, t.heaps, c->root, (int)t.skip_empty, acc);
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, acc, 16, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    dev_free(c, acc);
    GM_HIP(e);
    *digest = h[0];
    *n = h[1];
    return GM_OK;
}

int byte_histogram(Ctx *c, Hist *out) {
    const ByteTables t = byte_tables_of(c);
    CodeBins b;
    GM_TRY(code_bins_begin(c, &b));
    int rc = GM_OK;
    for (const BytePart &p : t.parts)
        if (rc == GM_OK) rc = byte_layout(t, [&](auto B) {
            return code_bins_launch<decltype(B)::value>(c, &b, p.table, p.list, p.nunits, t.ushift, t.heaps);
        });
    const int rc2 = code_bins_end(c, &b, out);
    return rc != GM_OK ? rc : rc2;
}

int byte_select(Ctx *c, const SelectDev &s) {
    const ByteTables t = byte_tables_of(c);
    for (const BytePart &p : t.parts)
        GM_TRY(byte_layout(t, [&](auto B) {
            return byte_select_launch<decltype(B)::value>(c, s, p.table, p.list, p.nunits, t.ushift, t.heaps);
        }));
    return GM_OK;
}

// a position's own code and its children's are read where byte_query reads them
int byte_verify(Ctx *c, const VerifyDev &v) {
    const ByteTables t = byte_tables_of(c);
    for (const BytePart &p : t.parts)
        if (p.table) GM_TRY(byte_layout(t, [&](auto B) {
            return byte_verify_launch<decltype(B)::value>(c, v, t.d_tables, t.d_owner, p.list, p.nunits, t.ushift,
                                                          t.oshift, t.heaps);
        }));
    return GM_OK;
}

int byte_moves(Ctx *c, const MovesReq &r) {
    const ByteTables t = byte_tables_of(c);
    return moves_run(c, r, [&](const MovesDev &mv) {
        return byte_layout(t, [&](auto B) {
            return byte_moves_launch<decltype(B)::value>(c, mv, t.d_tables, t.d_owner, t.oshift, t.heaps);
        });
    });
}

// gm_reach: one mark unit per key of the heaps' lattice in either layout; the positions that
// can be marked are the root's region, a position has at most two moves per heap
int byte_reach(Ctx *c, const ReachReq &q) {
    const ByteTables t = byte_tables_of(c);
    if (t.heaps < 1 || t.heaps > 8) { set_error("gm_reach: byte tables of %d heaps", t.heaps); return GM_E_STATE; }
    const uint64_t units = 1ull << (4 * t.heaps);
    uint64_t region = 1;
    for (int j = 0; j < t.heaps; j++) region *= ((c->root >> (4 * j)) & 15u) + 1u;
    return byte_layout(t, [&](auto B) {
        constexpr int BOX = decltype(B)::value;
        const ReachBytes<BOX> acc{t.d_tables, t.d_owner, t.oshift, t.heaps, (uint32_t)c->root};
        return reach_run(
            c, q, ReachDims{units, region, 2ull * (uint64_t)t.heaps},
            [&](const ReachDev &r) {
                hipLaunchKernelGGL(reach_level_kernel<ReachBytes<BOX>>, dim3(grid_counted(r.m)), dim3(256), 0, c->stream,
                                   acc, r);
                GM_HIP(hipGetLastError());
                return GM_OK;
            },
            [&](const ReachDev &r) {
                hipLaunchKernelGGL(byte_reach_sweep_kernel<BOX>, dim3(grid_counted(units)), dim3(256), 0, c->stream, acc,
                                   units, r);
                GM_HIP(hipGetLastError());
                return GM_OK;
            });
    });
}

// gm_poke: one byte of the table that holds the key's unit
int byte_poke(Ctx *c, const void *key, uint16_t rec) {
    const ByteTables t = byte_tables_of(c);
    const uint64_t k = *(const uint64_t *)key;
    const bool in = sub_in_region(k, c->root, t.heaps);
    const uint32_t idx = !in ? 0u : t.box ? box_index_of_key((uint32_t)k) : (uint32_t)k;
    uint8_t own = in ? 0 : 0xFF;
    if (in && t.d_owner) GM_HIP(hipMemcpy(&own, t.d_owner + (t.box ? idx >> 12 : idx >> t.oshift), 1, hipMemcpyDeviceToHost));
    if (own >= t.parts.size() || !t.parts[own].table) { set_error("gm_poke: the key is not a stored position"); return GM_E_KEY; }
    const int code = code_of_record(rec);
    if (code < 0) { set_error("gm_poke: the 1-byte codes hold WIN / LOSS with remoteness <= 126"); return GM_E_ARG; }
    const uint8_t b = (uint8_t)code;
    GM_HIP(hipMemcpyAsync(t.parts[own].table + idx, &b, 1, hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    return GM_OK;
}

}  // namespace

}  // namespace gm
