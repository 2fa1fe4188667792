// verify_common.hpp -- the consistency check of a solved table against the game rules
// (gm_verify): the device accumulator every engine's verify entry adds to, the one function that
// names a position's class, and the byte-table kernel of the dense SUBTRACT engines (its host
// side, and gm_poke's: byte_verify and byte_poke, byte_tables.hpp).
//
// A table of an acyclic game is the solution iff the root is in it, every primitive position
// stored carries (primitive value, 0), and every interior position stored has all its children
// in the table and the reduction of their records as its own (parent_score
// of the max child score, gm_common.hpp).  The check reads every stored position once and
// every child record once per edge -- the backward pass's lookups without its sorted lists.
//
// Accumulator (u64 words): [0] checked, [1..5] the classes in gm_verify_t's order, [6] child
// lookups, [7] the offender cursor; the offender list (cap keys) follows.  A thread tallies in
// registers and the workgroup adds each counter once (block_add); an offender appends its key
// through a plain atomicAdd on the cursor -- they are rare.
#pragma once
#include "sparse_common.hpp"
#include "box_common.hpp"

namespace gm {

enum { VF_OK = -1, VF_BAD_KEY = 0, VF_MISPLACED = 1, VF_BAD_PRIMITIVE = 2, VF_MISSING_CHILD = 3, VF_BAD_VALUE = 4 };
constexpr int VF_WORDS = 8;                 // counters and cursor before the offender list
constexpr uint64_t VF_FIRST_CAP = 1u << 16;   // offenders kept by the first pass (gm_api.hip runs a second when more are asked for)

struct VerifyDev {
    unsigned long long *acc;   // VF_WORDS words, then the list
    uint64_t cap;              // keys the list holds
};

// The class of a stored position whose key and slot are sound: its stored score against its
// primitive() code, or against the best of its children's scores.  The order of the classes
// (include/gmsolve.h: the first that applies) lives here and in the two key tests before it.
GM_HD int verify_class(uint32_t stored, int prim, uint32_t best, bool missing) {
    if (prim != UNDECIDED) return stored == score_of_primitive(prim) ? VF_OK : VF_BAD_PRIMITIVE;
    if (missing) return VF_MISSING_CHILD;
    return stored == parent_score(best) ? VF_OK : VF_BAD_VALUE;
}

// the u16 preference score of a 1-byte code (gm_common.hpp; 0 stays 0)
GM_HD uint32_t score_of_code(uint32_t code) { return score_of_record(record_of_code((uint8_t)code)); }

namespace {

struct VerifyTally {
    uint64_t n[7] = {0, 0, 0, 0, 0, 0, 0};
};

template <class K>
__device__ __forceinline__ void verify_note(const VerifyDev &v, VerifyTally &t, int cls, const K &key) {
    t.n[0]++;
    if (cls < 0) return;
    t.n[1 + cls]++;
    const unsigned long long at = atomicAdd(v.acc + 7, 1ull);
    if (at < v.cap) ((K *)(v.acc + VF_WORDS))[at] = key;
}
// every thread of the workgroup, once, at the kernel's end
__device__ __forceinline__ void verify_flush(const VerifyDev &v, const VerifyTally &t) {
#pragma unroll
    for (int i = 0; i < 7; i++) block_add(v.acc + i, t.n[i]);
}

// Byte tables of the subtraction game (1-byte codes), in the two layouts code_bins_launch
// distinguishes: slot = key (BOX = 0) and box-indexed (BOX = 1).  The walk is over units of
// 2^ushift contiguous bytes (the whole table, a block of the partitioned engine, a box) named
// by `list`; a position's own code and its children's are read where gm_query reads them:
// tables[owner[unit]] (owner == nullptr: tables[0]; unit = key >> oshift, or the box id).
// idx is the table index: the key, or box_index_of_key(key).  A child differs from its parent
// in one heap, so its box index is the parent's with that heap's fields replaced
// (box_index_with_heap).
// The children are DescSub::visit's -- heap i less 1 when it holds 1, less 2 when it holds 2 --
// made here by an unrolled loop over the 16 (heap, take) pairs, so that all 16 one-byte loads
// are issued before the first is used: a pair that is no move loads the position's own byte
// and is ignored.  With visit()'s loop every load was waited for before the next was issued
// and the walk was bound by that latency (2^32 positions: 188 ms).
template <int BOX>
__device__ __forceinline__ uint32_t byte_code_at(const uint8_t *const *__restrict__ tables,
                                                 const uint8_t *__restrict__ owner, int oshift, uint32_t idx) {
    const uint32_t r = owner ? owner[BOX ? idx >> 12 : idx >> oshift] : 0u;
    return r == 0xFFu ? 0u : tables[r][idx];
}

template <int BOX>
__global__ __launch_bounds__(256) void byte_verify_kernel(const uint8_t *const *__restrict__ tables,
                                                          const uint8_t *__restrict__ owner,
                                                          const uint32_t *__restrict__ list, uint64_t nunits, int ushift,
                                                          int oshift, int heaps, uint32_t root, VerifyDev v) {
    VerifyTally t;
    const uint64_t total = nunits << ushift, within = (1ull << ushift) - 1ull;
    DescSub d;
    d.heaps = heaps;
    if (BOX) heaps = 8;   // the box layout is the 8-heap game's: a constant for the unrolled loops
    for (uint64_t x = blockIdx.x * 256ull + threadIdx.x; x < total; x += (uint64_t)gridDim.x * 256ull) {
        const uint64_t unit = x >> ushift;
        const uint32_t idx = (uint32_t)((((uint64_t)(list ? list[unit] : (uint32_t)unit)) << ushift) | (x & within));
        const uint32_t key = BOX ? box_key_of_index(idx) : idx;
        if (!sub_in_region(key, root, heaps)) continue;
        const uint32_t stored = score_of_code(byte_code_at<BOX>(tables, owner, oshift, idx));
        const int prim = d.primitive(key);
        uint32_t best = 0;
        bool missing = false;
        uint32_t code[16];
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const int heap = m >> 1;
            const uint32_t take = 1u + (m & 1), h = (key >> (4 * heap)) & 15u;
            const bool move = heap < heaps && h >= take;
            const uint32_t c = key - (take << (4 * heap));
            const uint32_t cidx = !move ? idx : BOX ? box_index_with_heap(idx, heap, h - take) : c;
            code[m] = byte_code_at<BOX>(tables, owner, oshift, cidx);
        }
#pragma unroll
        for (int m = 0; m < 16; m++) {
            const int heap = m >> 1;
            const uint32_t take = 1u + (m & 1), h = (key >> (4 * heap)) & 15u;
            if (!(heap < heaps && h >= take)) continue;
            // the one primitive, all heaps empty: LOSS in 0, answered without the lookup
            const bool leaf = key == (take << (4 * heap));
            const uint32_t cd = leaf ? 255u : code[m];
            t.n[6] += !leaf;
            missing |= cd == 0u;
            best = max(best, cd);
        }
        verify_note(v, t, verify_class(stored, prim, score_of_code(best), missing), (uint64_t)key);
    }
    verify_flush(v, t);
}

}  // namespace

// ---------------------------------------------------------------- host side
template <int BOX>
inline int byte_verify_launch(Ctx *c, const VerifyDev &v, const uint8_t *const *tables, const uint8_t *owner,
                              const uint32_t *list, uint64_t nunits, int ushift, int oshift, int heaps) {
    if (!nunits) return GM_OK;
    const uint64_t total = nunits << ushift;
    hipLaunchKernelGGL(byte_verify_kernel<BOX>, dim3(grid_counted(total)), dim3(256), 0, c->stream, tables, owner, list,
                       nunits, ushift, oshift, heaps, (uint32_t)c->root, v);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// one gm_verify pass: the accumulator with room for `cap` offender keys of `key_bytes` each
struct VerifyRun {
    VerifyDev dev{nullptr, 0};
    uint64_t key_bytes = 8;
};
inline int verify_begin(Ctx *c, uint64_t cap, uint64_t key_bytes, VerifyRun *r) {
    r->key_bytes = key_bytes;
    r->dev.cap = cap;
    const uint64_t bytes = VF_WORDS * 8 + cap * key_bytes;
    GM_TRY(dev_alloc(c, (void **)&r->dev.acc, bytes));
    GM_HIP(hipMemsetAsync(r->dev.acc, 0, VF_WORDS * 8, c->stream));
    return GM_OK;
}
// counters into out (root_ok is the caller's), the offender keys written (raw, unsorted) into list
inline int verify_end(Ctx *c, VerifyRun *r, gm_verify_t *out, std::vector<unsigned char> *list) {
    uint64_t h[VF_WORDS];
    hipError_t e = hipMemcpyAsync(h, r->dev.acc, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) {
        const uint64_t n = std::min<uint64_t>(h[7], r->dev.cap);
        list->resize(n * r->key_bytes);
        if (n) e = hipMemcpy(list->data(), r->dev.acc + VF_WORDS, n * r->key_bytes, hipMemcpyDeviceToHost);
    }
    dev_free(c, r->dev.acc);
    r->dev.acc = nullptr;
    GM_HIP(e);
    out->checked = h[0];
    out->bad_key = h[1];
    out->misplaced = h[2];
    out->bad_primitive = h[3];
    out->missing_child = h[4];
    out->bad_value = h[5];
    out->child_lookups = h[6];
    return GM_OK;
}

// poke of a 1-byte code table: the code of a record (0xFFFF: 0, "no code"), or -1 when the
// codes cannot express it (a TIE, a remoteness past 126)
inline int code_of_record(uint16_t rec) {
    if (rec == REC_UNSOLVED) return 0;
    const uint32_t val = rec >> 14, rem = rec & 0x3FFFu;
    if (rem > 126 || (val != WIN && val != LOSS)) return -1;
    return val == WIN ? (int)rem + 1 : 255 - (int)rem;
}

}  // namespace gm
