// box_common.hpp -- box geometry of the 8-heap synthetic game, shared by the one-GPU box engine
// (dense_box.hip) and its split over ranks (dist_box.hip).
//
// The 16^8 lattice is cut into BOXES of 4 x 4 x 4 x 4 x 2 x 2 x 2 x 2 positions: heaps 0-3
// in quarters ("A" heaps, box coordinate c_i = h_i >> 2, 0..3), heaps 4-7 in halves ("B" heaps,
// c_j = h_j >> 1, 0..7).  Table index = box << 12 | A << 4 | B, A = sum over heaps 0-3 of
// (h_i & 3) << 2i, B = sum over heaps 4-7 of (h_j & 1) << (j - 4); the box id packs c_i at
// bits 2i (i < 4) and c_j at bits 8 + 3 (j - 4) (j >= 4).
//
// Heap transpositions.  Every heap plays by the same rules and the only primitive position
// has all heaps empty, so swapping two heaps maps a position to one of equal value and
// remoteness.  Swapping two A heaps or two B heaps maps boxes to boxes and keeps the box-tier
// (the sum of the box coordinates).  Code of a transposition: 0 = none, 1..6 = the A heaps of
// pair code - 1, 7..12 = the B heaps 4 + q, 4 + p of pair code - 7, pairs in the order
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3).  On a box it swaps two coordinate fields; on a row of
// 16 codes (one A, B = 0..15) an A transposition moves the row (A's digits q, p swap: row A
// of box C is row swap(A) of box swap(C)), a B transposition permutes its bytes (byte B of a
// row of C is byte swap(B) of the same row of swap(C)).
#pragma once
#include <stdint.h>

#ifndef GM_HD
#define GM_HD __host__ __device__ __forceinline__
#endif

namespace gm {

GM_HD uint32_t box_index_of_key(uint32_t k) {
    uint32_t off = 0, box = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t h = (k >> (4 * i)) & 15u;
        off |= (h & 3u) << (4 + 2 * i);
        box |= (h >> 2) << (2 * i);
    }
    for (int j = 0; j < 4; j++) {
        const uint32_t h = (k >> (16 + 4 * j)) & 15u;
        off |= (h & 1u) << j;
        box |= (h >> 1) << (8 + 3 * j);
    }
    return (box << 12) | off;
}
GM_HD uint32_t box_key_of_index(uint32_t x) {
    const uint32_t off = x & 4095u, box = x >> 12;
    uint32_t k = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t h = (((box >> (2 * i)) & 3u) << 2) | ((off >> (4 + 2 * i)) & 3u);
        k |= h << (4 * i);
    }
    for (int j = 0; j < 4; j++) {
        const uint32_t h = (((box >> (8 + 3 * j)) & 7u) << 1) | ((off >> j) & 1u);
        k |= h << (16 + 4 * j);
    }
    return k;
}
// the table index of the position that differs from the one at index x in heap `heap` alone,
// which holds h there: the heap's two fields replaced, no other heap decoded (gm_verify walks
// up to 16 children per position)
GM_HD uint32_t box_index_with_heap(uint32_t x, int heap, uint32_t h) {
    if (heap < 4) {
        const int o = 4 + 2 * heap, b = 12 + 2 * heap;
        return (x & ~((3u << o) | (3u << b))) | ((h & 3u) << o) | ((h >> 2) << b);
    }
    const int o = heap - 4, b = 20 + 3 * (heap - 4);
    return (x & ~((1u << o) | (7u << b))) | ((h & 1u) << o) | ((h >> 1) << b);
}
GM_HD int box_coord(uint32_t box, int dim) {
    return dim < 4 ? (int)((box >> (2 * dim)) & 3u) : (int)((box >> (8 + 3 * (dim - 4))) & 7u);
}
GM_HD uint32_t box_unit(int dim) { return dim < 4 ? 1u << (2 * dim) : 1u << (8 + 3 * (dim - 4)); }
GM_HD int box_tier(uint32_t box) {
    int t = 0;
    for (int i = 0; i < 8; i++) t += box_coord(box, i);
    return t;
}

// transposition codes (see the file comment)
constexpr int BX_NSWAP = 13;
GM_HD uint32_t bx_pair_q(uint32_t pc) { return pc < 3 ? 0u : pc < 5 ? 1u : 2u; }
GM_HD uint32_t bx_pair_p(uint32_t pc) { return pc < 3 ? pc + 1 : pc < 5 ? pc - 1 : 3u; }
GM_HD bool bx_swap_is_a(uint32_t code) { return code >= 1 && code <= 6; }
GM_HD bool bx_swap_is_b(uint32_t code) { return code >= 7; }
// the transposition's two heaps (0..7)
GM_HD void bx_swap_heaps(uint32_t code, int *q, int *p) {
    const uint32_t pc = bx_swap_is_a(code) ? code - 1 : code - 7, o = bx_swap_is_a(code) ? 0u : 4u;
    *q = (int)(o + bx_pair_q(pc));
    *p = (int)(o + bx_pair_p(pc));
}
GM_HD uint32_t bx_swap_box(uint32_t code, uint32_t b) {
    if (!code) return b;
    if (bx_swap_is_a(code)) {
        const uint32_t q = 2u * bx_pair_q(code - 1), p = 2u * bx_pair_p(code - 1);
        const uint32_t t = ((b >> q) ^ (b >> p)) & 3u;
        return b ^ (t << q) ^ (t << p);
    }
    const uint32_t q = 8u + 3u * bx_pair_q(code - 7), p = 8u + 3u * bx_pair_p(code - 7);
    const uint32_t t = ((b >> q) ^ (b >> p)) & 7u;
    return b ^ (t << q) ^ (t << p);
}
// row index A (0..255) of the box read through an A transposition (identity for the others)
GM_HD uint32_t bx_swap_row(uint32_t code, uint32_t A) {
    if (!bx_swap_is_a(code)) return A;
    const uint32_t q = 2u * bx_pair_q(code - 1), p = 2u * bx_pair_p(code - 1);
    const uint32_t t = ((A >> q) ^ (A >> p)) & 3u;
    return A ^ (t << q) ^ (t << p);
}
// a key through a transposition (heap i at bits 4 i)
GM_HD uint32_t bx_swap_key(uint32_t code, uint32_t k) {
    if (!code) return k;
    int q, p;
    bx_swap_heaps(code, &q, &p);
    const uint32_t t = ((k >> (4 * q)) ^ (k >> (4 * p))) & 15u;
    return k ^ (t << (4 * q)) ^ (t << (4 * p));
}


// Mirror of heaps 6 and 7 (the one-GPU box engine, GM_OPT_SYMMETRY).  swap67(C) is box C with
// the coordinate fields c6 (bits 14-16) and c7 (bits 17-19) exchanged; heaps 6 and 7 are bits 2
// and 3 of B, so row m of swap67(C) is row m of C with bytes B and swap(B) exchanged: dwords 1
// and 2 of the 16-byte row exchanged, the row's address inside the box unchanged.  Of a pair
// {C, swap67(C)} that lies in the root's region whole, the box with c6 > c7 is computed and
// carries the mirror flag (it also stores its twin); the box with c6 < c7 is mirrored-to and
// never computed.  Every other region box (c6 == c7, or the twin outside the region) is
// computed and stored once.  (This is the 6/7 factor of the rule; the 4/5 factor follows.)
constexpr uint32_t BX_MIRROR_FLAG = 0x80000000u;   // bit 31 of a compute-list entry (box ids have 20 bits)
constexpr uint32_t BX_BOX_MASK = 0x000FFFFFu;
GM_HD uint32_t bx_swap67(uint32_t b) {
    const uint32_t t = ((b >> 14) ^ (b >> 17)) & 7u;
    return b ^ (t << 14) ^ (t << 17);
}
GM_HD bool box_in_region(uint32_t box, uint32_t root_box) {
    bool in = true;
    for (int i = 0; i < 8; i++) in = in && box_coord(box, i) <= box_coord(root_box, i);
    return in;
}
// a region box of the root whose top box is root_box: 0 = computed, stored once; 1 = computed,
// stored to itself and to swap67(box) (the mirror flag); 2 = mirrored-to (not computed)
GM_HD int bx_mirror_class(uint32_t box, uint32_t root_box) {
    const int c6 = box_coord(box, 6), c7 = box_coord(box, 7);
    if (c6 == c7 || !box_in_region(bx_swap67(box), root_box)) return 0;
    return c6 > c7 ? 1 : 2;
}

// Mirror of heaps 4 and 5, the same rule on the fields c4 (bits 8-10) and c5 (bits 11-13).
// Heaps 4 and 5 are bits 0 and 1 of B, so row m of swap45(C) is row m of C with bytes 1 and 2 of
// each dword exchanged (v_perm_b32 selector BX_PERM45), the row's address unchanged; through
// both mirrors, the permuted dwords in the order {0, 2, 1, 3}.  Region membership factorises
// over the coordinates, so a box's two classes are independent: a box is computed iff neither
// class is 2; a computed box stores itself, swap67 of itself if its 6/7 class is 1 (bit 31 of its
// list entry), swap45 of itself if its 4/5 class is 1 (bit 30), and swap45(swap67()) of itself
// if both are.  Every region box is then written exactly once and nothing outside the region is.
constexpr uint32_t BX_MIRROR45_FLAG = 0x40000000u;   // bit 30 of a compute-list entry
constexpr uint32_t BX_PERM45 = 0x03010200u;
GM_HD uint32_t bx_swap45(uint32_t b) {
    const uint32_t t = ((b >> 8) ^ (b >> 11)) & 7u;
    return b ^ (t << 8) ^ (t << 11);
}
GM_HD int bx_mirror_class67(uint32_t box, uint32_t root_box) { return bx_mirror_class(box, root_box); }
GM_HD int bx_mirror_class45(uint32_t box, uint32_t root_box) {
    const int c4 = box_coord(box, 4), c5 = box_coord(box, 5);
    if (c4 == c5 || !box_in_region(bx_swap45(box), root_box)) return 0;
    return c4 > c5 ? 1 : 2;
}

// Mirror of heaps 2 and 3 (the dataflow launches of the hybrid schedule only), the same rule on
// the fields c2 (bits 4-5) and c3 (bits 6-7).  Heaps 2 and 3 are the digits at bits 4-5 and 6-7
// of the row index A, so row m of swap23(C) holds the 16 bytes of row swap(m) of C
// (bx_swap_row(BX_SWAP23, m): the two digits exchanged): the bytes unchanged, the row's address
// moved, 16 consecutive rows (256 B) staying together.  The third class is independent of the
// other two like them: a box is computed iff no class is 2, and stores itself and every
// composition of its flagged swaps, up to eight boxes (bit 29 of its list entry the 2/3 flag).
constexpr uint32_t BX_MIRROR23_FLAG = 0x20000000u;   // bit 29 of a compute-list entry
constexpr uint32_t BX_SWAP23 = 6;                    // the transposition code of heaps (2, 3)
GM_HD uint32_t bx_swap23(uint32_t b) {
    const uint32_t t = ((b >> 4) ^ (b >> 6)) & 3u;
    return b ^ (t << 4) ^ (t << 6);
}
GM_HD int bx_mirror_class23(uint32_t box, uint32_t root_box) {
    const int c2 = box_coord(box, 2), c3 = box_coord(box, 3);
    if (c2 == c3 || !box_in_region(bx_swap23(box), root_box)) return 0;
    return c2 > c3 ? 1 : 2;
}
// variant v (0..7) of a compute-list entry's box: bit 0 through the 6/7 mirror, bit 1 the 4/5,
// bit 2 the 2/3; and whether the entry's flags say that its group stores it
GM_HD uint32_t bx_twin_box(uint32_t entry, uint32_t v) {
    uint32_t b = entry & BX_BOX_MASK;
    if (v & 1u) b = bx_swap67(b);
    if (v & 2u) b = bx_swap45(b);
    if (v & 4u) b = bx_swap23(b);
    return b;
}
GM_HD bool bx_twin_stored(uint32_t entry, uint32_t v) {
    return (!(v & 1u) || (entry & BX_MIRROR_FLAG)) && (!(v & 2u) || (entry & BX_MIRROR45_FLAG)) &&
           (!(v & 4u) || (entry & BX_MIRROR23_FLAG));
}

}  // namespace gm
