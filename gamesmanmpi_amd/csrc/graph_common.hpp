// graph_common.hpp -- what the two solves of the explicit-graph engine share (graph.hip: rounds
// over every node, acyclic graphs only; graph_loopy.hip: frontier retrograde over the reverse
// graph, cycles allowed): the device state of a solved graph and the DRAW score.
//
// DRAW.  A loopy table holds a fourth value, (DRAW, 0), record 0xC000.  Its score is 0x0001:
// class 0, which no other score uses (gm_common.hpp: 0 is "no score", the classes 1..3 are WIN,
// TIE, LOSS).  It is known to the graph engine only -- record_of_score / score_of_record stay
// as every other engine reads them -- and it is NOT in preference order: a mover prefers a
// DRAW child to a WIN child and a TIE or LOSS child to a DRAW child, so the loopy reduction
// (loopy_key, loopy_parent_score) orders the scores through a key of its own instead of the
// plain max.
#pragma once
#include "gm_internal.hpp"

namespace gm {

struct Graph {
    uint64_t n = 0;
    uint8_t *prim = nullptr;
    uint64_t *off = nullptr;
    uint32_t *kid = nullptr;
    uint16_t *score = nullptr;
    unsigned long long *d_count = nullptr;
    uint32_t *d_err = nullptr;
    double t0 = 0;        // now_ms() when the upload began: the start of solve_ms
    bool loopy = false;   // the table of a loopy solve: DRAW scores, the loopy rule in gm_verify
};

constexpr uint16_t SCORE_DRAW = 0x0001;
constexpr uint16_t REC_DRAW = 0xC000;

GM_HD uint16_t graph_record(uint16_t s) { return s == SCORE_DRAW ? REC_DRAW : record_of_score(s); }
GM_HD uint16_t graph_score(uint16_t r) { return r == REC_DRAW ? SCORE_DRAW : score_of_record(r); }

// The child preference with DRAW: LOSS (shortest) > TIE (shortest) > DRAW > WIN (longest).
// The scores of the three classes keep their order when doubled, and DRAW goes between the
// largest WIN (0x7FFF -> 0xFFFE) and the smallest TIE (0x8000 -> 0x10000).  0 stays 0.
GM_HD uint32_t loopy_key(uint32_t s) { return s == SCORE_DRAW ? 0xFFFFu : s << 1; }
// the parent of a best child with key b: DRAW under a DRAW child, else as every engine
GM_HD uint16_t loopy_parent_score(uint32_t b) { return b == 0xFFFFu ? SCORE_DRAW : parent_score(b >> 1); }

inline unsigned grid_of(uint64_t n) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 8192));
}

void graph_free(Ctx *c);
int graph_upload(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid);
int graph_solve_loopy(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid);

}  // namespace gm
