// reach_common.hpp -- the positions reachable from a set of starts when each side follows a
// move policy (gm_reach): the request an engine's reach entry answers, the level-synchronous
// driver the device engines share (reach_run, gm_api.hip), the level kernel and its helpers, the
// byte-table accessor of the dense SUBTRACT engines (its host side: byte_reach, byte_tables.hpp)
// and the host twin for a host record table.  The tier-table accessor is ReachTiers
// (sparse_tables.hpp), the graph engine's ReachGraph (graph.hip).
//
// It is gm_moves' edge pass (moves_common.hpp: parent -> children -> records) run level by
// level as a frontier breadth-first search, with a visited set in place of an output array.
// The side of a reached position is the parity of its ply, so the visited set is over
// (position, side): two mark bits per position, 16 positions to a u32 mark word, and a frontier
// is a plain key array with no side per entry.  Per level (reach_run):
//   level kernel   one thread per frontier entry: its children made as moves_of_key makes them,
//                  the policy of the side to move applied (BEST and FIRST visit the children
//                  twice: the ranks first, then the selection), and for each selected child the
//                  engine's mark index, an atomicOr of the side bit, and -- only in the thread
//                  that flipped the bit -- an append to the next frontier
//   append         places are reserved per wave: a ballot, then ONE atomicAdd on the cursor for
//                  the wave's new entries (select_common.hpp select_note); atomics on one
//                  address serialise
//   counters       edges, missing and the orbit-weighted counts stay in registers; the workgroup
//                  adds each once (block_add)
// The next frontier cannot overflow: it is sized from min(2 x positions - pairs marked so far,
// entries x the engine's maximum move count); every store is guarded all the same, and a cursor
// past the capacity fails the call.  No kernel waits on another; every launch is bounded by its
// frontier; the loop ends when a level marks nothing or max_plies is reached.
//
// The key list is a final sweep over the marks, run only when a list is wanted: a counts-only
// call never pays for it, and no frontier is kept beyond the next level.  The list is unordered;
// gm_api.hip sorts what it copied back.
//
// An accessor A (a kernel argument) is what an engine's table looks like to the level kernel:
//   A::Key                      uint64_t or K128
//   find(k, rec, stored)        the mark index of k's stored representative and its record, or
//                               -1 (rec = 0xFFFF) when k has no record -- gm_query's answer
//   interior(k)                 k is not primitive
//   visit(k, f)                 f(child, place) for every child, place = its index in gm_moves'
//                               order (Othello: its slot in the plugin's walk, which orders alike)
//   weight(stored)              the orbit size of a stored representative
#pragma once
#include "moves_common.hpp"

#include <functional>
#include <vector>

namespace gm {

constexpr uint64_t REACH_CHUNK = 1ull << 20;   // frontier entries per launch (GM_REACH_CHUNK overrides)

// the device accumulator: u64 words
enum { RA_CURSOR = 0, RA_PAIRS = 1, RA_EDGES = 2, RA_MISSING = 3, RA_FRESH = 4, RA_STARTS = 5, RA_OVER = 6, RA_WORDS = 8 };

// gm_reach as an engine sees it: start keys of the engine's key type (uint64_t, or K128 on a
// wide context -- a key that is no position arrives as K128{0, 0}, which valid() refuses)
struct ReachReq {
    gm_reach_t how;
    const void *starts;
    uint64_t key_bytes;                   // 8 or sizeof(K128)
    uint64_t n_starts;
    uint64_t cap;                         // list entries wanted; 0: counts only
    gm_reach_out_t *out;
    std::vector<uint64_t> *ply_counts;    // one entry per ply reached
    std::vector<unsigned char> *keys;     // the list, raw and unsorted: keys, records, side bits
    std::vector<uint16_t> *recs;
    std::vector<uint8_t> *sides;
};

// what the driver sizes its buffers from
struct ReachDims {
    uint64_t units;       // mark indices: 2 bits each
    uint64_t positions;   // at most this many stored positions can be marked (<= units)
    uint64_t max_moves;   // children of one position at most; 0: unknown
};

// one launch: a chunk of a frontier (or of the starts), or the sweep
struct ReachDev {
    const void *in;            // m keys
    uint64_t m;
    void *next;                // the next frontier, next_cap keys
    uint64_t next_cap;
    uint32_t *marks;
    unsigned long long *acc;   // RA_WORDS words
    uint32_t side;             // the parity of the entries marked by this launch
    uint32_t policy;           // of the side to move at the entries of `in`
    uint32_t seed;             // 1: `in` holds start keys, marked themselves and not expanded
    void *keys;                // sweep: the list, cap entries
    uint16_t *recs;
    uint8_t *sides;
    uint64_t cap;
};

// the level loop (gm_api.hip): `level` enqueues the engine's level kernel for one ReachDev,
// `sweep` the engine's pass over its marks into the list
int reach_run(Ctx *c, const ReachReq &q, const ReachDims &dim, const std::function<int(const ReachDev &)> &level,
              const std::function<int(const ReachDev &)> &sweep);

inline bool reach_wants_first(const ReachReq &q) {
    return q.how.mover == GM_REACH_FIRST || q.how.other == GM_REACH_FIRST;
}

namespace {

struct ReachTally {
    uint64_t edges = 0, missing = 0, pairs = 0, fresh = 0, starts = 0;
};

// The side bit of mark index `at` set; the thread that flipped it counts the pair (and the
// position, when neither of its bits was set) and appends the stored key to the next frontier.
// Any subset of a wave's lanes may call it together, so the leader is the first that takes part.
template <class A>
__device__ __forceinline__ void reach_mark(const A &a, const ReachDev &r, ReachTally &t, int64_t at,
                                           const typename A::Key &stored) {
    using K = typename A::Key;
    const uint32_t sh = 2u * (uint32_t)(at & 15);
    const uint32_t bit = 1u << (sh + r.side);
    const uint32_t old = atomicOr(r.marks + (at >> 4), bit);
    const bool fresh = !(old & bit);
    if (fresh) {
        const uint32_t w = a.weight(stored);
        t.pairs += w;
        if (!((old >> sh) & 3u)) t.fresh += w;
    }
    const unsigned long long m = __ballot(fresh);
    if (!fresh) return;
    const int lane = threadIdx.x & 63, leader = __ffsll(m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(r.acc + RA_CURSOR, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < r.next_cap) ((K *)r.next)[pos] = stored;
    else atomicOr(r.acc + RA_OVER, 1ull);
}

template <class A>
__device__ __forceinline__ void reach_of_entry(const A &a, const ReachDev &r, ReachTally &t, uint64_t i) {
    using K = typename A::Key;
    const K k = ((const K *)r.in)[i];
    if (r.seed) {
        uint16_t rec;
        K st;
        const int64_t at = a.find(k, rec, st);
        if (at >= 0) {
            t.starts++;
            reach_mark(a, r, t, at, st);
        }
        return;
    }
    if (!a.interior(k)) return;
    if (r.policy == GM_REACH_ALL) {
        a.visit(k, [&](const K &ch, uint32_t) {
            uint16_t rec;
            K st;
            const int64_t at = a.find(ch, rec, st);
            t.edges++;
            if (at < 0) t.missing++;
            else reach_mark(a, r, t, at, st);
        });
        return;
    }
    // the ranks first: the maximum and the first place that has it
    int64_t best = -1;
    uint32_t first = 0;
    a.visit(k, [&](const K &ch, uint32_t pos) {
        uint16_t rec;
        K st;
        (void)a.find(ch, rec, st);
        const int64_t rk = (int64_t)moves_rank(rec);
        if (rk > best || (rk == best && pos < first)) {
            best = rk;
            first = pos;
        }
    });
    a.visit(k, [&](const K &ch, uint32_t pos) {
        uint16_t rec;
        K st;
        const int64_t at = a.find(ch, rec, st);
        if ((int64_t)moves_rank(rec) != best) return;
        if (r.policy == GM_REACH_FIRST && pos != first) return;
        t.edges++;
        if (at < 0) t.missing++;
        else reach_mark(a, r, t, at, st);
    });
}

// every thread of the workgroup, once, at the kernel's end
__device__ __forceinline__ void reach_flush(const ReachDev &r, const ReachTally &t) {
    block_add(r.acc + RA_PAIRS, t.pairs);
    block_add(r.acc + RA_EDGES, t.edges);
    block_add(r.acc + RA_MISSING, t.missing);
    block_add(r.acc + RA_FRESH, t.fresh);
    block_add(r.acc + RA_STARTS, t.starts);
}

template <class A>
__global__ __launch_bounds__(256) void reach_level_kernel(A a, ReachDev r) {
    ReachTally t;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < r.m; i += (uint64_t)gridDim.x * 256ull)
        reach_of_entry(a, r, t, i);
    reach_flush(r, t);
}

// the two mark bits of mark index `at`
__device__ __forceinline__ uint32_t reach_bits(const ReachDev &r, uint64_t at) {
    return (r.marks[at >> 4] >> (2u * (uint32_t)(at & 15))) & 3u;
}

// the sweep: one reached position into the list, places reserved per wave as in reach_mark
template <class K>
__device__ __forceinline__ void reach_emit(const ReachDev &r, const K &key, uint16_t rec, uint32_t bits) {
    const unsigned long long m = __ballot(1);
    const int lane = threadIdx.x & 63, leader = __ffsll(m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(r.acc + RA_CURSOR, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    const uint64_t at = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (at < r.cap) {
        ((K *)r.keys)[at] = key;
        r.recs[at] = rec;
        r.sides[at] = (uint8_t)bits;
    }
}

// Byte tables of the subtraction game, read where gm_query reads them (byte_moves_kernel,
// moves_common.hpp): the mark index is the key itself in both layouts, 16^heaps units.  A key
// outside the root's region has no record; a child of a key of the region is in the region.
// The children are DescSub::visit's, heap by heap, take 1 then take 2: key arithmetic.
template <int BOX>
struct ReachBytes {
    using Key = uint64_t;
    const uint8_t *const *tables;
    const uint8_t *owner;
    int oshift, heaps;
    uint32_t root;
    __device__ __forceinline__ int64_t find(const uint64_t &k, uint16_t &rec, uint64_t &st) const {
        rec = REC_UNSOLVED;
        st = k;
        if (!sub_in_region(k, root, heaps)) return -1;
        const uint32_t key = (uint32_t)k;
        rec = record_of_code((uint8_t)byte_code_at<BOX>(tables, owner, oshift, BOX ? box_index_of_key(key) : key));
        return rec == REC_UNSOLVED ? -1 : (int64_t)k;
    }
    __device__ __forceinline__ bool interior(const uint64_t &k) const { return k != 0; }
    template <class F>
    __device__ __forceinline__ void visit(const uint64_t &k, F &&f) const {
        uint32_t pos = 0;
        for (int j = 0; j < heaps; j++) {
            const uint32_t h = (uint32_t)(k >> (4 * j)) & 15u;
            if (h >= 1u) f(k - (1ull << (4 * j)), pos++);
            if (h >= 2u) f(k - (2ull << (4 * j)), pos++);
        }
    }
    __device__ __forceinline__ uint32_t weight(const uint64_t &) const { return 1u; }
};

// the sweep over the keys of the heaps' lattice: a marked key is a stored position
template <int BOX>
__global__ __launch_bounds__(256) void byte_reach_sweep_kernel(ReachBytes<BOX> a, uint64_t units, ReachDev r) {
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < units; k += (uint64_t)gridDim.x * 256ull) {
        const uint32_t bits = reach_bits(r, k);
        if (!bits) continue;
        uint16_t rec;
        uint64_t st;
        (void)a.find(k, rec, st);
        reach_emit(r, k, rec, bits);
    }
}

}  // namespace

// The same answer from a host record table (small_dense: tic-tac-toe's 19,683 records): a host
// breadth-first search over the accessor moves_host uses.  No device.  rec(key) is gm_query's
// answer; slot = key, `slots` of them.
template <class D, class R>
inline int reach_host(const D &d, const ReachReq &q, uint64_t slots, R &&rec) {
    const uint64_t *starts = (const uint64_t *)q.starts;
    std::vector<uint8_t> marks(slots, 0);
    std::vector<uint64_t> cur, next;
    gm_reach_out_t o{};
    q.ply_counts->clear();
    auto mark = [&](uint64_t k, uint32_t side) {
        const uint8_t bit = (uint8_t)(1u << side);
        if (marks[k] & bit) return;
        if (!marks[k]) o.n++;
        marks[k] |= bit;
        next.push_back(k);
    };
    for (uint64_t i = 0; i < q.n_starts; i++)
        if (rec(starts[i]) != REC_UNSOLVED) {
            o.n_starts++;
            mark(starts[i], 0);
        }
    for (uint32_t ply = 0; !next.empty(); ply++) {
        q.ply_counts->push_back(next.size());
        (ply & 1 ? o.n_other : o.n_mover) += next.size();
        cur.swap(next);
        next.clear();
        if (q.how.max_plies && ply >= q.how.max_plies) break;
        const uint32_t policy = ply & 1 ? q.how.other : q.how.mover;
        for (const uint64_t k : cur) {
            if (d.primitive(k) != UNDECIDED) continue;
            uint64_t ch[32];
            const int cnt = d.children(k, ch);
            MovesBest best;
            for (int j = 0; j < cnt; j++) best.add(moves_rank(rec(ch[j])), (uint32_t)j);
            for (int j = 0; j < cnt; j++) {
                const uint16_t cr = rec(ch[j]);
                if (policy != GM_REACH_ALL && (int64_t)moves_rank(cr) != best.rank) continue;
                if (policy == GM_REACH_FIRST && (uint32_t)j != best.at) continue;
                o.edges++;
                if (cr == REC_UNSOLVED) o.missing++;
                else mark(ch[j], (ply + 1) & 1);
            }
        }
    }
    o.plies = (int32_t)q.ply_counts->size();
    *q.out = o;
    q.keys->clear();
    q.recs->clear();
    q.sides->clear();
    for (uint64_t k = 0; k < slots && q.recs->size() < q.cap; k++)
        if (marks[k]) {
            const unsigned char *p = (const unsigned char *)&k;
            q.keys->insert(q.keys->end(), p, p + 8);
            q.recs->push_back(rec(k));
            q.sides->push_back(marks[k]);
        }
    return GM_OK;
}

}  // namespace gm
