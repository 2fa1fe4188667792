// moves_common.hpp -- every move of a batch of positions valued on the device (gm_moves): the
// request an engine's moves entry answers, the chunked two-pass driver the device engines share,
// the order and rank helpers of the kernels, and the byte-table kernel of the dense SUBTRACT
// engines (its host side: byte_moves, byte_tables.hpp).  The tier-table kernel is res_moves_kernel (sparse_tables.hpp), the graph engine's
// graph_moves_kernel (graph.hip).
//
// It is gm_verify's edge pass (verify_common.hpp: parent -> children -> records) driven by the
// caller's keys instead of the stored positions, with the children, their records and the
// mover's choice as output.  Per chunk of keys on the device (moves_run, gm_api.hip):
//   count pass   a key's own record, looked up as gm_query looks it up, and the number of its
//                children: move generation only, no child lookup
//   scan         exclusive sum of the counts (hipcub): every key's place in the child arrays,
//                so the output is in key order, gap-free and the same on every run
//   fill pass    the children made again, each looked up once, keys and records written at the
//                key's place, the best child and the count of its equals into the head
// No atomics: the scan gives every key its place.  The fill pass runs in the heads-only form
// too (best / n_best need the children's records); it then writes no child.
//
// Order.  A key's children are the plugin's gen_moves order, what gm_expand_host returns: the
// descriptor's visit() order, except that Othello's plugin walks the squares x outer, y inner
// where visit() walks the plane bits.  move_slot gives a child's place in the plugin's walk;
// a first visit() collects the slots taken into a 64-bit mask and the second puts each child
// at the number of taken slots below its own -- no child array, no sort.
//
// Rank.  move_rank of solver.py (loopy_key of graph_common.hpp) on records: LOSS (shortest) >
// TIE (shortest) > DRAW > WIN (longest) > no record.  best is the first child of maximal rank,
// n_best the children of that rank.
#pragma once
#include "sparse_common.hpp"
#include "box_common.hpp"
#include "verify_common.hpp"

#include <functional>
#include <type_traits>
#include <vector>

namespace gm {

constexpr uint64_t MOVES_CHUNK = 1ull << 20;   // keys on the device at a time (GM_MOVES_CHUNK overrides)

// gm_moves as an engine sees it: keys of the engine's key type (uint64_t, or K128 on a wide
// context -- a key that is no position arrives as K128{0, 0}, which valid() refuses)
struct MovesReq {
    const void *keys;
    uint64_t key_bytes;       // 8 or sizeof(K128)
    int words;                // ABI words per child key (1 or 3)
    uint64_t n;
    gm_moves_t *heads;
    uint64_t *child_words;    // null: heads and the total only
    uint16_t *child_records;  // may be null
    uint64_t cap;
    uint64_t *n_children;
};

// one pass over one chunk of keys on the device
struct MovesDev {
    const void *keys;         // m keys
    uint64_t m;
    uint64_t *count;          // count pass: children per key (the scan's input)
    const uint64_t *first;    // fill pass: the exclusive sum of count
    gm_moves_t *heads;        // count pass: record, count, best = -1; fill pass: first, best, n_best
    uint64_t *child_words;    // fill pass: this chunk's children (null: none wanted)
    uint16_t *child_records;
    uint64_t base;            // children of the chunks before this one (added to first)
    int fill;                 // 0 count pass, 1 fill pass
};

// the chunk loop (gm_api.hip): uploads, scans and downloads; `pass` enqueues one engine pass
int moves_run(Ctx *c, const MovesReq &r, const std::function<int(const MovesDev &)> &pass);

// move_rank of a record
GM_HD uint32_t moves_rank(uint32_t rec) { return rec == 0xC000u ? 0xFFFFu : 2u * score_of_record((uint16_t)rec); }

// A child's place in the plugin's gen_moves walk where that differs from visit()'s: < 64, or
// -1 for "visit() order".  Othello (othello_bit_new.py:137-143, 163-166): squares x outer, y
// inner; the square played is the one bit the occupied plane gains, plane bit A - 1 - (L y + x);
// the pass is a single child.
template <class D, class K>
GM_HD int move_slot(const D &, const K &, const K &) { return -1; }
GM_HD int move_slot(const DescOthello &o, const uint64_t &k, const uint64_t &ch) {
    const uint32_t placed = (o.wplane(ch) | o.bplane(ch)) ^ (o.wplane(k) | o.bplane(k));
    if (!placed) return 0;
    const int j = o.A - 1 - __builtin_ctz(placed);
    return o.L * (j % o.L) + j / o.L;
}
GM_HD int move_slot(const DescOthello8 &, const K128 &k, const K128 &ch) {
    const uint64_t placed = DescOthello8::occ(ch) ^ DescOthello8::occ(k);
    if (!placed) return 0;
    const int j = 63 - __builtin_ctzll(placed);
    return 8 * (j % 8) + j / 8;
}
template <class D>
struct slot_order_t {
    static constexpr bool value = std::is_same<D, DescOthello>::value || std::is_same<D, DescOthello8>::value;
};

// a key as ABI words (DescOthello8::to_words on the device)
GM_HD void moves_put_key(uint64_t *w, uint64_t at, uint64_t k) { w[at] = k; }
GM_HD void moves_put_key(uint64_t *w, uint64_t at, const K128 &k) {
    const uint64_t wp = k.lo, b = DescOthello8::occ(k) & ~wp;
    w[3 * at] = (b << 16) | ((uint64_t)DescOthello8::turn(k) << 8) | (uint64_t)DescOthello8::pass(k);
    w[3 * at + 1] = (b >> 48) | (wp << 16);
    w[3 * at + 2] = wp >> 48;
}

// the running choice of the fill pass: children may arrive out of place (Othello), so the
// first of equals is the one with the smallest place
struct MovesBest {
    int64_t rank = -1;
    uint32_t at = 0, n = 0;
    GM_HD void add(uint32_t r, uint32_t pos) {
        if ((int64_t)r > rank) { rank = r; at = pos; n = 1; }
        else if ((int64_t)r == rank) { n++; at = pos < at ? pos : at; }
    }
};

GM_HD gm_moves_t moves_head(uint64_t first, uint32_t count, int best, uint16_t rec, uint32_t n_best) {
    gm_moves_t h;
    h.first = first;
    h.count = (uint16_t)count;
    h.best = (int16_t)best;
    h.record = rec;
    h.n_best = (uint16_t)n_best;
    return h;
}

// Both passes over a descriptor D and a table T (T::record(d, key) is gm_query's answer for a
// key, valid or not): the body of res_moves_kernel (sparse_tables.hpp).  A key with a record
// is a position of the game, so primitive() and visit() are only ever called on valid keys.
template <class D, class T>
__device__ __forceinline__ void moves_of_key(const D &d, const T &tab, const MovesDev &mv, uint64_t i) {
    using K = key_t<D>;
    const K k = ((const K *)mv.keys)[i];
    const auto plain = unreduced(d);   // the plugin's own moves: a child need not be canonical
    if (!mv.fill) {
        const uint16_t rec = tab.record(d, k);
        uint32_t cnt = 0;
        if (rec != REC_UNSOLVED && d.primitive(k) == UNDECIDED) {
            if constexpr (step_count_t<D>::value) {
                int dt;
                cnt = (uint32_t)d.count_children(k, &dt);
            } else {
                plain.visit(k, [&](const K &) {
                    cnt++;
                    return true;
                });
            }
        }
        mv.count[i] = cnt;
        mv.heads[i] = moves_head(0, cnt, -1, rec, 0);
        return;
    }
    gm_moves_t h = mv.heads[i];
    const uint64_t first = mv.first[i];
    h.first = mv.base + first;
    if (h.count) {
        uint64_t taken = 0;
        if constexpr (slot_order_t<D>::value)
            plain.visit(k, [&](const K &ch) {
                taken |= 1ull << move_slot(plain, k, ch);
                return true;
            });
        MovesBest best;
        uint32_t seq = 0;
        plain.visit(k, [&](const K &ch) {
            uint32_t pos = seq++;
            if constexpr (slot_order_t<D>::value) pos = (uint32_t)popc64(taken & ((1ull << move_slot(plain, k, ch)) - 1ull));
            const uint16_t rec = tab.record(d, ch);
            if (pos < h.count) {   // the count pass made the same children: never past the key's place
                if (mv.child_words) moves_put_key(mv.child_words, first + pos, ch);
                if (mv.child_records) mv.child_records[first + pos] = rec;
            }
            best.add(moves_rank(rec), pos);
            return true;
        });
        h.best = (int16_t)best.at;
        h.n_best = (uint16_t)best.n;
    }
    mv.heads[i] = h;
}

namespace {

// Byte tables of the subtraction game, in byte_verify_kernel's two layouts (verify_common.hpp:
// slot = key, BOX = 0; box-indexed, BOX = 1) and read where gm_query reads them
// (tables[owner[unit]]).  A key outside the root's region -- a nibble above the root's, or past
// the table -- has no record, as in byte_query_kernel (byte_tables.hpp).  The children are
// DescSub::visit's, heap by heap, take 1 then take 2; a child of a key of the region is in the
// region.  As in byte_verify_kernel all 16 one-byte loads are issued before the first is used
// (a pair that is no move loads the position's own byte and is ignored), and the 16 codes stay
// in registers: the loops are unrolled, no array is indexed at run time.
template <int BOX>
__global__ __launch_bounds__(256) void byte_moves_kernel(const uint8_t *const *__restrict__ tables,
                                                         const uint8_t *__restrict__ owner, int oshift, int heaps,
                                                         uint32_t root, MovesDev mv) {
    if (BOX) heaps = 8;   // the box layout is the 8-heap game's: a constant for the unrolled loops
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < mv.m; i += (uint64_t)gridDim.x * 256ull) {
        const uint64_t k64 = ((const uint64_t *)mv.keys)[i];
        const uint32_t key = (uint32_t)k64;
        if (!mv.fill) {
            const bool in = sub_in_region(k64, root, heaps);
            uint16_t rec = REC_UNSOLVED;
            uint32_t cnt = 0;
            if (in) {
                rec = record_of_code((uint8_t)byte_code_at<BOX>(tables, owner, oshift, BOX ? box_index_of_key(key) : key));
                if (rec != REC_UNSOLVED)
                    for (int j = 0; j < heaps; j++) {
                        const uint32_t h = (key >> (4 * j)) & 15u;
                        cnt += (h >= 1u) + (h >= 2u);
                    }
            }
            mv.count[i] = cnt;
            mv.heads[i] = moves_head(0, cnt, -1, rec, 0);
            continue;
        }
        gm_moves_t h = mv.heads[i];
        const uint64_t first = mv.first[i];
        h.first = mv.base + first;
        if (h.count) {
            const uint32_t idx = BOX ? box_index_of_key(key) : key;
            uint32_t code[16];
#pragma unroll
            for (int m = 0; m < 16; m++) {
                const int heap = m >> 1;
                const uint32_t take = 1u + (m & 1), hh = (key >> (4 * heap)) & 15u;
                const bool move = heap < heaps && hh >= take;
                const uint32_t cidx = !move ? idx : BOX ? box_index_with_heap(idx, heap, hh - take) : key - (take << (4 * heap));
                code[m] = byte_code_at<BOX>(tables, owner, oshift, cidx);
            }
            MovesBest best;
            uint32_t pos = 0;
#pragma unroll
            for (int m = 0; m < 16; m++) {
                const int heap = m >> 1;
                const uint32_t take = 1u + (m & 1), hh = (key >> (4 * heap)) & 15u;
                if (!(heap < heaps && hh >= take)) continue;
                const uint16_t rec = record_of_code((uint8_t)code[m]);
                if (pos < h.count) {
                    if (mv.child_words) mv.child_words[first + pos] = (uint64_t)(key - (take << (4 * heap)));
                    if (mv.child_records) mv.child_records[first + pos] = rec;
                }
                best.add(moves_rank(rec), pos);
                pos++;
            }
            h.best = (int16_t)best.at;
            h.n_best = (uint16_t)best.n;
        }
        mv.heads[i] = h;
    }
}

}  // namespace

// one pass over a chunk, for the four byte-table engines (byte_moves, byte_tables.hpp)
template <int BOX>
inline int byte_moves_launch(Ctx *c, const MovesDev &mv, const uint8_t *const *tables, const uint8_t *owner, int oshift,
                             int heaps) {
    if (!mv.m) return GM_OK;
    hipLaunchKernelGGL(byte_moves_kernel<BOX>, dim3(grid_counted(mv.m)), dim3(256), 0, c->stream, tables, owner, oshift,
                       heaps, (uint32_t)c->root, mv);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// The same answer from a host record table (small_dense: tic-tac-toe's 19,683 records, which
// its query and select read too): no chunks, no device.  rec(key) is gm_query's answer.
template <class D, class R>
inline int moves_host(const D &d, const MovesReq &r, R &&rec) {
    const uint64_t *keys = (const uint64_t *)r.keys;
    uint64_t total = 0;
    std::vector<uint64_t> kids;
    std::vector<uint16_t> recs;
    for (uint64_t i = 0; i < r.n; i++) {
        const uint16_t own = rec(keys[i]);
        uint64_t ch[32];
        const int cnt = own != REC_UNSOLVED && d.primitive(keys[i]) == UNDECIDED ? d.children(keys[i], ch) : 0;
        MovesBest best;
        for (int j = 0; j < cnt; j++) {
            const uint16_t cr = rec(ch[j]);
            kids.push_back(ch[j]);
            recs.push_back(cr);
            best.add(moves_rank(cr), (uint32_t)j);
        }
        r.heads[i] = moves_head(total, (uint32_t)cnt, cnt ? (int)best.at : -1, own, best.n);
        total += (uint64_t)cnt;
    }
    *r.n_children = total;
    if (!r.child_words || !r.cap) return GM_OK;
    if (r.cap < total) { set_error("gm_moves: the child arrays hold %llu, need %llu", (unsigned long long)r.cap, (unsigned long long)total); return GM_E_CAP; }
    for (uint64_t j = 0; j < total; j++) {
        r.child_words[j] = kids[j];
        if (r.child_records) r.child_records[j] = recs[j];
    }
    return GM_OK;
}

}  // namespace gm
