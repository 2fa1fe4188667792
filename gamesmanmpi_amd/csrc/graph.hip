// graph.hip -- retrograde over an explicit position graph (GM_GAME_GRAPH).
//
// For plugins that no device descriptor reproduces: the host
// walks the plugin itself (initial_position / gen_moves / do_move / primitive,
// reference README.md:28-88) and hands over the graph in CSR form -- position i's
// primitive() code and the indices of its children; the device resolves it with
// the same canonical reduction as every other engine (Appendix A,
// gm_common.hpp preference scores).
//
// Rounds: every unresolved position whose children are all resolved takes
// parent_score(max child score); a round that resolves nothing while positions
// remain means a cycle (the reference would never terminate either) and fails.
// Rounds = the height of the graph; a position is written once, when final, so
// reading a child in the round it is written is benign.
//
// GM_OPT_LOOPY 1 solves with graph_loopy.hip instead (cycles, DRAW); the table it leaves is read
// by the kernels below, which know the DRAW score (graph_common.hpp) and its rule in gm_verify.
#include "graph_common.hpp"
#include "hist_common.hpp"
#include "verify_common.hpp"
#include "moves_common.hpp"
#include "reach_common.hpp"
#include "select_common.hpp"

#include <algorithm>

namespace gm {

__global__ __launch_bounds__(256) void graph_init_kernel(const uint8_t *__restrict__ prim, uint64_t n,
                                                         uint16_t *__restrict__ score, uint32_t *err) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const int p = prim[i];
        if (p > UNDECIDED) atomicOr(err, DEV_ERR_TIER);   // not a primitive() code
        if (p == DRAW) atomicOr(err, DEV_ERR_DRAW);
        score[i] = p == UNDECIDED ? 0 : score_of_primitive(p);
    }
}

__global__ __launch_bounds__(256) void graph_round_kernel(const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ kid, uint64_t n,
                                                          uint16_t *score, unsigned long long *resolved,
                                                          uint32_t *err) {
    uint64_t done = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (score[i]) continue;
        const uint64_t a = off[i], b = off[i + 1];
        if (a == b) { atomicOr(err, DEV_ERR_NOMOVES); continue; }
        uint32_t best = 0;
        bool ready = true;
        for (uint64_t e = a; e < b; e++) {
            const uint32_t s = ((const volatile uint16_t *)score)[kid[e]];
            if (!s) { ready = false; break; }
            best = max(best, s);
        }
        if (!ready) continue;
        if (score_overflows(best)) atomicOr(err, DEV_ERR_OVERFLOW);
        ((volatile uint16_t *)score)[i] = parent_score(best);
        done++;
    }
    for (int o = 32; o > 0; o >>= 1) done += __shfl_xor(done, o);
    if ((threadIdx.x & 63) == 0 && done) atomicAdd(resolved, (unsigned long long)done);
}

__global__ void graph_records_kernel(const uint16_t *__restrict__ score, const uint64_t *__restrict__ idx,
                                     uint16_t *__restrict__ out, uint64_t n, uint64_t total) {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = idx ? idx[i] : i;
    out[i] = k < total ? graph_record(score[k]) : REC_UNSOLVED;
}

__global__ void graph_digest_kernel(const uint16_t *__restrict__ score, uint64_t n, unsigned long long *acc) {
    uint64_t sum = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        sum += digest_term(i, graph_record(score[i]));
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) atomicAdd(acc, (unsigned long long)sum);
}

// census of the nodes' scores (hist_common.hpp score bins: LDS, or global for deep graphs); the
// DRAW nodes of a loopy table have no row and are left out (Hist::other counts them)
__global__ void graph_hist_kernel(const uint16_t *__restrict__ score, uint64_t n, unsigned long long *bins,
                                  uint32_t nbin, int use_lds, int loopy) {
    uint32_t *lds = score_bins_open(nbin, use_lds);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint16_t s = score[i];
        if (loopy && s == SCORE_DRAW) continue;
        score_bin_add(lds, bins, nbin, s, 1u);
    }
    score_bins_flush(lds, bins, nbin);
}

// the graph on the device and an empty score table, for either solve
int graph_upload(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid) {
    graph_free(c);
    if (!n) { set_error("empty graph"); return GM_E_ARG; }
    Graph *g = c->graph = new Graph();
    g->n = n;
    const uint64_t m = off[n];
    for (uint64_t i = 0; i < m; i++)
        if (kid[i] >= n) { set_error("child index %u out of range", kid[i]); return GM_E_ARG; }
    g->t0 = now_ms();
    GM_TRY(dev_alloc(c, (void **)&g->prim, n));
    GM_TRY(dev_alloc(c, (void **)&g->off, (n + 1) * 8));
    GM_TRY(dev_alloc(c, (void **)&g->kid, std::max<uint64_t>(m, 1) * 4));
    GM_TRY(dev_alloc(c, (void **)&g->score, (n + 1) / 2 * 4));   // whole words: the loopy solve's atomics are 32-bit
    GM_TRY(dev_alloc(c, (void **)&g->d_count, 8));
    GM_TRY(dev_alloc(c, (void **)&g->d_err, 4));
    GM_HIP(hipMemcpyAsync(g->prim, prim, n, hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipMemcpyAsync(g->off, off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (m) GM_HIP(hipMemcpyAsync(g->kid, kid, m * 4, hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipMemsetAsync(g->d_err, 0, 4, c->stream));
    return GM_OK;
}

int graph_solve(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid) {
    if (c->loopy) return graph_solve_loopy(c, n, prim, off, kid);
    GM_TRY(graph_upload(c, n, prim, off, kid));
    Graph *g = c->graph;
    const double t0 = g->t0;
    const uint64_t m = off[n];
    hipLaunchKernelGGL(graph_init_kernel, dim3(grid_of(n)), dim3(256), 0, c->stream, g->prim, n, g->score, g->d_err);
    uint64_t interior = 0;
    for (uint64_t i = 0; i < n; i++) interior += prim[i] == UNDECIDED;
    uint64_t left = interior;
    int rounds = 0;
    while (left) {
        GM_HIP(hipMemsetAsync(g->d_count, 0, 8, c->stream));
        hipLaunchKernelGGL(graph_round_kernel, dim3(grid_of(n)), dim3(256), 0, c->stream, g->off, g->kid, n, g->score,
                           g->d_count, g->d_err);
        unsigned long long got = 0;
        uint32_t e = 0;
        GM_HIP(hipMemcpyAsync(&got, g->d_count, 8, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipMemcpyAsync(&e, g->d_err, 4, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        if (e) return dev_error_to_gm(e);
        rounds++;
        if (!got) {
            set_error("%llu positions never resolve: the graph has a cycle", (unsigned long long)left);
            return GM_E_STATE;
        }
        left -= got;
    }
    uint32_t e = 0;
    GM_HIP(hipMemcpyAsync(&e, g->d_err, 4, hipMemcpyDeviceToHost, c->stream));
    uint16_t rs;
    GM_HIP(hipMemcpyAsync(&rs, g->score, 2, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    if (e) return dev_error_to_gm(e);
    double t1 = now_ms();
    c->root = 0;
    c->root_record = record_of_score(rs);
    c->n_positions = n;
    c->stats.n_positions = n;
    c->stats.n_primitive = n - interior;
    c->stats.n_tiers = rounds;
    c->stats.n_edges = m;
    c->stats.solve_ms = t1 - t0;
    c->stats.backward_ms = t1 - t0;
    c->stats.table_bytes = n * 11 + m * 4;
    c->tier_counts.clear();
    return GM_OK;
}

static int graph_export(Ctx *c, void *keys_out, uint16_t *recs, uint64_t cap, uint64_t *n) {
    uint64_t *keys = (uint64_t *)keys_out;
    Graph *g = c->graph;
    *n = g->n;
    if (!keys) return GM_OK;
    if (cap < g->n) { set_error("export buffer too small"); return GM_E_CAP; }
    DevBuf<uint16_t> dr;
    GM_TRY(dr.alloc(g->n));
    hipLaunchKernelGGL(graph_records_kernel, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0, c->stream, g->score,
                       (const uint64_t *)nullptr, dr.p, g->n, g->n);
    GM_HIP(hipMemcpyAsync(recs, dr, g->n * 2, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < g->n; i++) keys[i] = i;
    return GM_OK;
}

static int graph_query(Ctx *c, const void *keys_in, uint16_t *recs, uint64_t n) {
    const uint64_t *keys = (const uint64_t *)keys_in;
    Graph *g = c->graph;
    return query_keys(c, keys, recs, n, n, [&](const uint64_t *dk, uint16_t *dr, uint64_t m) {
        hipLaunchKernelGGL(graph_records_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, g->score, dk,
                           dr, m, g->n);
    });
}

static int graph_digest(Ctx *c, uint64_t *digest, uint64_t *n) {
    Graph *g = c->graph;
    GM_HIP(hipMemsetAsync(g->d_count, 0, 8, c->stream));
    hipLaunchKernelGGL(graph_digest_kernel, dim3(grid_of(g->n)), dim3(256), 0, c->stream, g->score, g->n, g->d_count);
    unsigned long long h;
    GM_HIP(hipMemcpyAsync(&h, g->d_count, 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    *digest = h;
    *n = g->n;
    return GM_OK;
}

// Remoteness is below the node count (a round may resolve several levels, so the rounds do not
// bound it) and at most 0x3FFF, which a chain ending in a LOSS or TIE leaf reaches (score_overflows
// lets the last step through): first the bins that fit in LDS, and for a graph deeper than those the
// global bins
static int graph_histogram(Ctx *c, Hist *out) {
    Graph *g = c->graph;
    const uint32_t full = (uint32_t)std::min<uint64_t>(g->n, MAX_REMOTENESS + 2), lds = HIST_LDS_BUDGET / 12;
    for (uint32_t nbin : {std::min(full, lds), full}) {
        ScoreBins b;
        GM_TRY(score_bins_begin(c, nbin, &b));
        hipLaunchKernelGGL(graph_hist_kernel, dim3(std::min(grid_of(g->n), 2048u)), dim3(256), b.lds_bytes, c->stream,
                           g->score, g->n, b.d, b.nbin, b.use_lds, (int)g->loopy);
        bool deeper = false;
        GM_TRY(score_bins_end(c, &b, out, nbin < full ? &deeper : nullptr));
        if (!deeper) break;
    }
    // every node of a loopy table has a score, so what has no row is DRAW
    if (g->loopy) out->other = g->n - out->total();
    return GM_OK;
}

// gm_select over the nodes (select_common.hpp): a node's key is its index, its record
// graph_record of its score, so a loopy table's DRAW is selectable
__global__ __launch_bounds__(256) void graph_select_kernel(const uint16_t *__restrict__ score, uint64_t n, SelectDev s) {
    SelectTally t;
    // per wave, so that every lane makes the same trips
    for (uint64_t w0 = blockIdx.x * 256ull + (threadIdx.x & ~63u); w0 < n; w0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = w0 + (threadIdx.x & 63u);
        const uint16_t rec = i < n ? graph_record(score[i]) : REC_UNSOLVED;
        select_note(s, t, select_match(s.values, s.rem_lo, s.rem_hi, rec), i, rec);
    }
    select_flush(s, t);
}

static int graph_select(Ctx *c, const SelectDev &s) {
    Graph *g = c->graph;
    hipLaunchKernelGGL(graph_select_kernel, dim3(grid_counted(g->n)), dim3(256), 0, c->stream, g->score, g->n, s);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// gm_verify over the nodes (verify_common.hpp): a node's score against its primitive() code or
// the best of its children's scores, read through the CSR the solve left on the device.  A
// node's key is its index, so no key or placement class exists here.
//
// LOOPY: the rule of a loopy table (graph_common.hpp).  A primitive carries its value's score,
// DRAW included; an interior node the loopy reduction of its children -- the best child under
// LOSS > TIE > DRAW > WIN, a DRAW best child making the parent DRAW.  That local rule is also
// sufficient: a W/L/T label with finite remoteness is sound by induction on the remoteness
// (its witness chain strictly descends to a primitive), every truly decided node is then
// forced to its label by induction on its true remoteness, and what remains is DRAW.
GM_HD int verify_class_loopy(uint32_t stored, int prim, uint32_t best_key, bool missing) {
    if (prim != UNDECIDED) return stored == (prim == DRAW ? SCORE_DRAW : score_of_primitive(prim)) ? VF_OK : VF_BAD_PRIMITIVE;
    if (missing) return VF_MISSING_CHILD;
    return stored == loopy_parent_score(best_key) ? VF_OK : VF_BAD_VALUE;
}

template <bool LOOPY>
__global__ __launch_bounds__(256) void graph_verify_kernel(const uint8_t *__restrict__ prim,
                                                           const uint64_t *__restrict__ off,
                                                           const uint32_t *__restrict__ kid,
                                                           const uint16_t *__restrict__ score, uint64_t n, VerifyDev v) {
    VerifyTally t;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
        const int p = prim[i];
        uint32_t best = 0;
        bool missing = false;
        if (p == UNDECIDED)
            for (uint64_t e = off[i]; e < off[i + 1]; e++) {
                const uint32_t s = score[kid[e]];
                t.n[6]++;
                missing |= s == 0u;
                best = max(best, LOOPY ? loopy_key(s) : s);
            }
        verify_note(v, t, LOOPY ? verify_class_loopy(score[i], p, best, missing) : verify_class(score[i], p, best, missing),
                    i);
    }
    verify_flush(v, t);
}

static int graph_verify(Ctx *c, const VerifyDev &v) {
    Graph *g = c->graph;
    if (g->loopy)
        hipLaunchKernelGGL(graph_verify_kernel<true>, dim3(grid_counted(g->n)), dim3(256), 0, c->stream, g->prim, g->off,
                           g->kid, g->score, g->n, v);
    else
        hipLaunchKernelGGL(graph_verify_kernel<false>, dim3(grid_counted(g->n)), dim3(256), 0, c->stream, g->prim, g->off,
                           g->kid, g->score, g->n, v);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// gm_moves over node indices (moves_common.hpp): the children are the CSR's, in its order; a
// key >= n has no record; a DRAW child of a loopy table ranks between TIE and WIN (moves_rank).
// The count and the choice are 16-bit in gm_moves_t: a node lists at most 32,767 children.
__global__ __launch_bounds__(256) void graph_moves_kernel(const uint8_t *__restrict__ prim,
                                                          const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ kid,
                                                          const uint16_t *__restrict__ score, uint64_t n, MovesDev mv) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < mv.m; i += (uint64_t)gridDim.x * 256ull) {
        const uint64_t k = ((const uint64_t *)mv.keys)[i];
        if (!mv.fill) {
            const uint16_t rec = k < n ? graph_record(score[k]) : REC_UNSOLVED;
            uint32_t cnt = 0;
            if (rec != REC_UNSOLVED && prim[k] == UNDECIDED) cnt = (uint32_t)min(off[k + 1] - off[k], (uint64_t)0x7FFF);
            mv.count[i] = cnt;
            mv.heads[i] = moves_head(0, cnt, -1, rec, 0);
            continue;
        }
        gm_moves_t h = mv.heads[i];
        const uint64_t first = mv.first[i];
        h.first = mv.base + first;
        if (h.count) {
            MovesBest best;
            const uint64_t e0 = off[k];
            for (uint32_t pos = 0; pos < h.count; pos++) {
                const uint32_t ch = kid[e0 + pos];
                const uint16_t rec = ch < n ? graph_record(score[ch]) : REC_UNSOLVED;
                if (mv.child_words) mv.child_words[first + pos] = ch;
                if (mv.child_records) mv.child_records[first + pos] = rec;
                best.add(moves_rank(rec), pos);
            }
            h.best = (int16_t)best.at;
            h.n_best = (uint16_t)best.n;
        }
        mv.heads[i] = h;
    }
}

static int graph_moves(Ctx *c, const MovesReq &r) {
    Graph *g = c->graph;
    return moves_run(c, r, [&](const MovesDev &mv) {
        hipLaunchKernelGGL(graph_moves_kernel, dim3(grid_counted(mv.m)), dim3(256), 0, c->stream, g->prim, g->off, g->kid,
                           g->score, g->n, mv);
        GM_HIP(hipGetLastError());
        return GM_OK;
    });
}

// gm_reach over node indices (reach_common.hpp): the mark index is the node, the children are
// the whole CSR row in its order, a key >= n or a node without a score has no record.  A loopy
// table's cycles end at the marks.
struct ReachGraph {
    using Key = uint64_t;
    const uint8_t *prim;
    const uint64_t *off;
    const uint32_t *kid;
    const uint16_t *score;
    uint64_t n;
    __device__ __forceinline__ int64_t find(const uint64_t &k, uint16_t &rec, uint64_t &st) const {
        st = k;
        rec = k < n ? graph_record(score[k]) : REC_UNSOLVED;
        return rec == REC_UNSOLVED ? -1 : (int64_t)k;
    }
    __device__ __forceinline__ bool interior(const uint64_t &k) const { return prim[k] == UNDECIDED; }
    template <class F>
    __device__ __forceinline__ void visit(const uint64_t &k, F &&f) const {
        const uint64_t e0 = off[k], e1 = off[k + 1];
        for (uint64_t e = e0; e < e1; e++) f((uint64_t)kid[e], (uint32_t)(e - e0));
    }
    __device__ __forceinline__ uint32_t weight(const uint64_t &) const { return 1u; }
};

__global__ __launch_bounds__(256) void graph_reach_sweep_kernel(ReachGraph a, ReachDev r) {
    for (uint64_t k = blockIdx.x * 256ull + threadIdx.x; k < a.n; k += (uint64_t)gridDim.x * 256ull) {
        const uint32_t bits = reach_bits(r, k);
        if (bits) reach_emit(r, k, graph_record(a.score[k]), bits);
    }
}

static int graph_reach(Ctx *c, const ReachReq &q) {
    Graph *g = c->graph;
    const ReachGraph acc{g->prim, g->off, g->kid, g->score, g->n};
    // a row's length is not bounded here: the marks alone size the frontiers
    return reach_run(
        c, q, ReachDims{g->n, g->n, 0},
        [&](const ReachDev &r) {
            hipLaunchKernelGGL(reach_level_kernel<ReachGraph>, dim3(grid_counted(r.m)), dim3(256), 0, c->stream, acc, r);
            GM_HIP(hipGetLastError());
            return GM_OK;
        },
        [&](const ReachDev &r) {
            hipLaunchKernelGGL(graph_reach_sweep_kernel, dim3(grid_counted(g->n)), dim3(256), 0, c->stream, acc, r);
            GM_HIP(hipGetLastError());
            return GM_OK;
        });
}

static int graph_poke(Ctx *c, const void *key, uint16_t rec) {
    Graph *g = c->graph;
    const uint64_t k = *(const uint64_t *)key;
    if (k >= g->n) { set_error("gm_poke: the key is not a stored position"); return GM_E_KEY; }
    if (rec == REC_DRAW && !g->loopy) { set_error("gm_poke: not a record"); return GM_E_ARG; }
    const uint16_t s = graph_score(rec);
    GM_HIP(hipMemcpyAsync(g->score + k, &s, 2, hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    return GM_OK;
}

void graph_free(Ctx *c) {
    Graph *g = c->graph;
    if (!g) return;
    for (void *p : {(void *)g->prim, (void *)g->off, (void *)g->kid, (void *)g->score, (void *)g->d_count,
                    (void *)g->d_err})
        dev_free(c, p);
    (void)hipStreamSynchronize(c->stream);
    delete g;
    c->graph = nullptr;
}

GM_ENGINE_RECORD(graph_engine, GM_ENGINE_GRAPH, nullptr, graph_export,
                 graph_query, graph_digest, graph_histogram, graph_select, nullptr, graph_free, graph_verify, graph_poke,
                 nullptr, graph_moves, nullptr, graph_reach)

}  // namespace gm
