// graph_loopy.hip -- the loopy solve of an explicit position graph (GM_OPT_LOOPY 1): frontier
// retrograde over the reverse graph.  Cycles are allowed, and what neither side can decide is
// DRAW (include/gmsolve.h gm_solve_graph).
//
// The solution is the least fixed point, by levels.  Win/loss phase: level 0 is the WIN and
// LOSS primitives; at level k >= 1 an undecided node with a LOSS child of remoteness k - 1 is
// WIN in k, one whose children are all WIN with largest remoteness k - 1 is LOSS in k.  Tie
// phase, over what is still undecided: level 0 is the TIE primitives, a node with a TIE child
// of remoteness k - 1 is TIE in k.  What is left is DRAW.
//
// State per node: its u16 score (0 = undecided), a u32 count of its children not yet known to
// be WIN, and its parents (reverse CSR, built once per solve by count / scan / fill; an edge
// listed twice is counted twice and listed twice, so counter and parent list agree; edges out
// of primitives are left out, a primitive's children do not count).  The nodes decided at
// level k are the frontier of the launch for level k + 1, which pushes to their parents:
//
//   from a LOSS node (tie phase: a TIE node)  every undecided parent is claimed: 0 -> WIN
//       (TIE) in k + 1.  All claimants of a level write the same value, so the claim is one
//       atomic fetch-or on the score and the claimant that saw 0 owns the parent: it appends
//       it to the next frontier.  (HIP has no 16-bit compare-and-swap; the fetch-or on the
//       aligned word that holds the score claims it just the same, and needs no retry loop.)
//   from a WIN node  every parent's counter is decremented; the thread that brings it to 0
//       writes LOSS in k + 1 and appends the parent.
//
// The two writes cannot race: a node with a LOSS child never reaches 0, because that child
// never decrements, and a node whose counter reaches 0 has WIN children only, so nobody
// claims it.  A counter that reaches 0 does so at the level of its last -- longest -- WIN
// child, and a claim happens at the level of the first -- shortest -- LOSS or TIE child: the
// remoteness rules of gm_common.hpp.  A node enters a frontier once, so one queue of n
// entries holds every frontier back to back; its tail is the only thing the host reads per
// level, and the order inside a frontier (which does vary from run to run) never reaches a
// record.
//
// Work per level is the parent lists of its frontier, O(n + m) over the solve, against the
// default mode's O(n) per round.  Parent lists are skewed -- a primitive or a hub has
// thousands of parents -- so no lane walks a long list alone (wave_walk): a lane keeps lists
// of up to WALK_SHORT entries to itself, and longer ones are walked by the whole wave, 64
// entries a step.  Appends are aggregated per wave: a ballot places them in the wave's stage in
// LDS, one atomic on the tail moves a full stage to the queue (WaveStage).
//
// No kernel waits for another: one launch per level, the host reads the tail and the error
// word between launches, and every device loop is bounded by a list length.
#include "graph_common.hpp"

#include <hipcub/hipcub.hpp>

namespace gm {

namespace {

constexpr uint32_t WALK_SHORT = 32;
enum { PHASE_WINLOSS = 0, PHASE_TIE = 1 };
enum : uint32_t { PUSH_CLAIM = 0, PUSH_COUNT = 1 };

// Every lane of the wave calls this with its own list [a, b) and a tag (a == b: no list).
// f(active, e, tag) is called by all 64 lanes together, `active` lanes each with one entry e
// of a list and that list's tag, so f may use wave-wide operations.
template <class F>
__device__ __forceinline__ void wave_walk(uint64_t a, uint64_t b, uint32_t tag, F &&f) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t len = b - a;
    const bool is_long = len > WALK_SHORT;
    // short lists: one per lane, as many steps as the wave's longest
    const uint32_t mine = is_long ? 0u : (uint32_t)len;
    uint32_t most = mine;
    for (int o = 32; o > 0; o >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, o));
    for (uint32_t j = 0; j < most; j++) f(j < mine, a + j, tag);
    // long lists: one after the other, 64 entries a step
    for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1ull) {
        const int src = __ffsll(todo) - 1;
        const uint64_t a0 = __shfl((unsigned long long)a, src), b0 = __shfl((unsigned long long)b, src);
        const uint32_t t0 = (uint32_t)__shfl((int)tag, src);
        for (uint64_t e = a0 + lane; e - lane < b0; e += 64) f(e < b0, e, t0);
    }
}

// Appends to the frontier queue, aggregated per wave.  Every wave of a launch appends to the
// one tail, and an atomic per ballot (a few entries each) made that address the bottleneck of a
// level: 0.45 ms for a level of 435 k nodes, 0.03 ms of it launch and read-back.  So a wave
// stages its entries in STAGE words of LDS of its own -- the ballot gives each lane its place,
// the count is wave-uniform and lives in a register, no LDS atomic -- and moves them to the
// queue with one atomic on the tail when the stage is full and when the kernel ends.  A wave's
// LDS accesses are served in order, so the lanes read what other lanes of the wave staged
// without a workgroup barrier; the fence keeps the compiler from moving them.
constexpr uint32_t STAGE = 256;

struct WaveStage {
    uint32_t *lds;     // this wave's STAGE words
    uint32_t held;     // entries staged: the same in every lane
    uint32_t *queue, *tail, *err;
    uint64_t cap;
};

#define WAVE_STAGE(name, queue, tail, cap, err)          \
    __shared__ uint32_t name##_lds[(256 / 64) * STAGE];  \
    WaveStage name{name##_lds + (threadIdx.x >> 6) * STAGE, 0u, queue, tail, err, cap}

// all 64 lanes call
__device__ __forceinline__ void stage_flush(WaveStage &s) {
    if (!s.held) return;
    __threadfence_block();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(s.tail, s.held);
    base = (uint32_t)__shfl((int)base, 0);
    for (uint32_t j = lane; j < s.held; j += 64) {
        const uint64_t at = (uint64_t)base + j;
        if (at < s.cap) s.queue[at] = s.lds[j];
        else atomicOr(s.err, DEV_ERR_TABLE_FULL);   // a node entered a frontier twice: never, by the argument above
    }
    __threadfence_block();
    s.held = 0;
}

// append v for the lanes with `got` (all 64 lanes call)
__device__ __forceinline__ void wave_append(WaveStage &s, bool got, uint32_t v) {
    const unsigned long long m = __ballot(got);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63u, add = (uint32_t)__popcll(m);
    if (s.held + add > STAGE) stage_flush(s);
    if (got) s.lds[s.held + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
    s.held += add;
}

// 0 -> val on node p's score, through the aligned word that holds it; true for the one caller
// that saw 0.  Callers of one launch that meet on p all bring the same val.
__device__ __forceinline__ bool claim_score(uint16_t *score, uint32_t p, uint32_t val) {
    const uint32_t shift = (p & 1u) * 16u;
    const uint32_t old = atomicOr((uint32_t *)score + (p >> 1), val << shift);
    return ((old >> shift) & 0xFFFFu) == 0u;
}

// scores and counters from the primitive() codes; the WIN and LOSS primitives are level 0
__global__ __launch_bounds__(256) void loopy_init_kernel(const uint8_t *__restrict__ prim,
                                                         const uint64_t *__restrict__ off, uint64_t n,
                                                         uint16_t *__restrict__ score, uint32_t *__restrict__ pcount,
                                                         uint32_t *__restrict__ indeg, uint32_t *__restrict__ queue,
                                                         uint32_t *ctl) {
    WAVE_STAGE(stage, queue, ctl, n, ctl + 1);
    for (uint64_t i0 = blockIdx.x * 256ull; i0 < n; i0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = i0 + threadIdx.x;
        bool seed = false;
        if (i < n) {
            const int p = prim[i];
            const uint64_t deg = off[i + 1] - off[i];
            if (p > UNDECIDED) atomicOr(ctl + 1, DEV_ERR_TIER);   // not a primitive() code
            if (p == UNDECIDED && !deg) atomicOr(ctl + 1, DEV_ERR_NOMOVES);
            score[i] = p == UNDECIDED ? 0 : (p >= DRAW ? SCORE_DRAW : score_of_primitive(p));
            pcount[i] = p == UNDECIDED ? (uint32_t)deg : 0u;
            indeg[i] = 0;
            seed = p == WIN || p == LOSS;
        }
        if (i == n - 1) indeg[n] = 0;
        wave_append(stage, seed, (uint32_t)i);
    }
    stage_flush(stage);
}

// transpose, 1: a node's parent entries
__global__ __launch_bounds__(256) void loopy_count_kernel(const uint8_t *__restrict__ prim,
                                                          const uint64_t *__restrict__ off,
                                                          const uint32_t *__restrict__ kid, uint64_t n, uint32_t *indeg) {
    for (uint64_t i0 = blockIdx.x * 256ull; i0 < n; i0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = i0 + threadIdx.x;
        const bool interior = i < n && prim[i] == UNDECIDED;
        const uint64_t a = interior ? off[i] : 0, b = interior ? off[i + 1] : 0;
        wave_walk(a, b, 0u, [&](bool active, uint64_t e, uint32_t) {
            if (active) atomicAdd(indeg + kid[e], 1u);
        });
    }
}

// transpose, 3: the parent lists.  indeg still holds the counts: counted down, it hands every
// entry of a list its place (any order; nothing depends on it)
__global__ __launch_bounds__(256) void loopy_fill_kernel(const uint8_t *__restrict__ prim,
                                                         const uint64_t *__restrict__ off,
                                                         const uint32_t *__restrict__ kid, uint64_t n,
                                                         const uint32_t *__restrict__ poff, uint32_t *indeg,
                                                         uint32_t *__restrict__ par, uint64_t npar) {
    for (uint64_t i0 = blockIdx.x * 256ull; i0 < n; i0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = i0 + threadIdx.x;
        const bool interior = i < n && prim[i] == UNDECIDED;
        const uint64_t a = interior ? off[i] : 0, b = interior ? off[i + 1] : 0;
        wave_walk(a, b, (uint32_t)i, [&](bool active, uint64_t e, uint32_t parent) {
            if (!active) return;
            const uint32_t k = kid[e];
            const uint64_t at = (uint64_t)poff[k] + (atomicSub(indeg + k, 1u) - 1u);
            if (at < npar) par[at] = parent;
        });
    }
}

// One level: the frontier queue[head, head + count) -- the nodes decided at remoteness rem - 1
// -- pushes to its parents, which are decided at remoteness rem and appended behind the tail.
// rem past the 14 bits of a record: nothing is written, the first node that would be decided
// raises DEV_ERR_OVERFLOW instead.
__global__ __launch_bounds__(256) void loopy_level_kernel(uint32_t *queue, uint64_t head, uint64_t count,
                                                          const uint32_t *__restrict__ poff,
                                                          const uint32_t *__restrict__ par, uint16_t *score,
                                                          uint32_t *pcount, uint32_t *ctl, uint64_t n, int phase,
                                                          uint32_t rem) {
    const bool over = rem > 0x3FFFu;
    const uint32_t low = 0x3FFFu - rem;
    const uint32_t claim_val = phase == PHASE_TIE ? 0x8000u | low : 0x4000u | rem;   // TIE / WIN in rem
    const uint32_t loss_val = 0xC000u | low;                                         // LOSS in rem
    WAVE_STAGE(stage, queue, ctl, n, ctl + 1);
    for (uint64_t i0 = blockIdx.x * 256ull; i0 < count; i0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t a = 0, b = 0;
        uint32_t push = PUSH_CLAIM;
        if (i < count) {
            const uint32_t node = queue[head + i];
            a = poff[node];
            b = poff[node + 1];
            // win/loss phase: a LOSS node (class 3) claims, a WIN node (class 1) counts down
            if (phase == PHASE_WINLOSS && (score[node] >> 14) == 1u) push = PUSH_COUNT;
        }
        wave_walk(a, b, push, [&](bool active, uint64_t e, uint32_t how) {
            bool got = false;
            uint32_t p = 0;
            if (active) {
                p = par[e];
                if (how == PUSH_CLAIM) {
                    if (((const volatile uint16_t *)score)[p] == 0) {
                        if (over) atomicOr(ctl + 1, DEV_ERR_OVERFLOW);
                        else got = claim_score(score, p, claim_val);
                    }
                } else if (atomicSub(pcount + p, 1u) == 1u) {
                    // p's last child is known WIN: no child of p is LOSS, so nobody claims p
                    if (over) atomicOr(ctl + 1, DEV_ERR_OVERFLOW);
                    else got = claim_score(score, p, loss_val);
                }
            }
            wave_append(stage, got, p);
        });
    }
    stage_flush(stage);
}

// level 0 of the tie phase: the TIE primitives
__global__ __launch_bounds__(256) void loopy_tie_seed_kernel(const uint8_t *__restrict__ prim, uint64_t n,
                                                             uint32_t *__restrict__ queue, uint32_t *ctl) {
    WAVE_STAGE(stage, queue, ctl, n, ctl + 1);
    for (uint64_t i0 = blockIdx.x * 256ull; i0 < n; i0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = i0 + threadIdx.x;
        wave_append(stage, i < n && prim[i] == TIE, (uint32_t)i);
    }
    stage_flush(stage);
}

// what no level decided is DRAW; the DRAW nodes, primitives included, are counted
__global__ __launch_bounds__(256) void loopy_final_kernel(uint16_t *__restrict__ score, uint64_t n,
                                                          unsigned long long *draws) {
    uint64_t mine = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
        uint16_t s = score[i];
        if (!s) score[i] = s = SCORE_DRAW;
        mine += s == SCORE_DRAW;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(draws, (unsigned long long)mine);
}

// the solve's own buffers: back to the context's cache when it ends, however it ends
struct LoopyTemp {
    Ctx *c;
    uint32_t *pcount = nullptr, *indeg = nullptr, *poff = nullptr, *par = nullptr, *queue = nullptr;
    void *scan = nullptr;
    explicit LoopyTemp(Ctx *ctx) : c(ctx) {}
    ~LoopyTemp() {
        (void)hipStreamSynchronize(c->stream);
        for (void *p : {(void *)pcount, (void *)indeg, (void *)poff, (void *)par, (void *)queue, scan}) dev_free(c, p);
    }
};

}  // namespace

int graph_solve_loopy(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid) {
    GM_TRY(graph_upload(c, n, prim, off, kid));
    Graph *g = c->graph;
    g->loopy = true;
    const double t0 = g->t0;
    const uint64_t m = off[n];
    if (n >= (1ull << 31) || m >= (1ull << 32)) {
        set_error("loopy graphs are limited to 2^31 - 1 positions and 2^32 - 1 edges");
        return GM_E_ARG;
    }
    uint64_t interior = 0, npar = 0;
    for (uint64_t i = 0; i < n; i++)
        if (prim[i] == UNDECIDED) { interior++; npar += off[i + 1] - off[i]; }
    LoopyTemp t(c);
    GM_TRY(dev_alloc(c, (void **)&t.pcount, n * 4));
    GM_TRY(dev_alloc(c, (void **)&t.indeg, (n + 1) * 4));
    GM_TRY(dev_alloc(c, (void **)&t.poff, (n + 1) * 4));
    GM_TRY(dev_alloc(c, (void **)&t.par, std::max<uint64_t>(npar, 1) * 4));
    GM_TRY(dev_alloc(c, (void **)&t.queue, n * 4));
    size_t scan_bytes = 0;
    GM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, t.indeg, t.poff, (int)(n + 1), c->stream));
    GM_TRY(dev_alloc(c, &t.scan, scan_bytes));
    // ctl[0]: the queue's tail, ctl[1]: the error flags -- read together after every level
    uint32_t *ctl = (uint32_t *)g->d_count;
    uint32_t got[2] = {0, 0};
    auto read_ctl = [&]() -> int {
        GM_HIP(hipMemcpyAsync(got, ctl, 8, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        if (got[1]) return dev_error_to_gm(got[1]);
        if (got[0] > n) { set_error("the frontier queue overran"); return GM_E_STATE; }
        return GM_OK;
    };
    const dim3 all(grid_of(n)), wg(256);
    GM_HIP(hipMemsetAsync(ctl, 0, 8, c->stream));
    hipLaunchKernelGGL(loopy_init_kernel, all, wg, 0, c->stream, g->prim, g->off, n, g->score, t.pcount, t.indeg, t.queue,
                       ctl);
    GM_HIP(hipGetLastError());
    GM_TRY(read_ctl());
    const double t_init = now_ms();
    // the reverse graph
    hipLaunchKernelGGL(loopy_count_kernel, all, wg, 0, c->stream, g->prim, g->off, g->kid, n, t.indeg);
    GM_HIP(hipcub::DeviceScan::ExclusiveSum(t.scan, scan_bytes, t.indeg, t.poff, (int)(n + 1), c->stream));
    hipLaunchKernelGGL(loopy_fill_kernel, all, wg, 0, c->stream, g->prim, g->off, g->kid, n, t.poff, t.indeg, t.par,
                       npar);
    GM_HIP(hipGetLastError());
    GM_HIP(hipStreamSynchronize(c->stream));
    const double t_rev = now_ms();
    // the levels of both phases: a level with an empty frontier ends its phase, and a node enters
    // the queue once, so at most n levels run
    uint64_t head = 0, tail = got[0];
    int levels = 0;
    for (int phase : {PHASE_WINLOSS, PHASE_TIE}) {
        if (phase == PHASE_TIE) {
            hipLaunchKernelGGL(loopy_tie_seed_kernel, all, wg, 0, c->stream, g->prim, n, t.queue, ctl);
            GM_TRY(read_ctl());
            tail = got[0];
        }
        for (uint32_t rem = 1; tail > head; rem++) {
            const double tl = trace_on() ? now_ms() : 0;
            hipLaunchKernelGGL(loopy_level_kernel, dim3(grid_of(tail - head)), wg, 0, c->stream, t.queue, head,
                               tail - head, t.poff, t.par, g->score, t.pcount, ctl, n, phase, rem);
            GM_TRY(read_ctl());
            if (trace_on())
                fprintf(stderr, "[gm] loopy %s level %u: frontier %llu, decided %llu, %.3f ms\n",
                        phase == PHASE_TIE ? "tie" : "win/loss", rem, (unsigned long long)(tail - head),
                        (unsigned long long)(got[0] - tail), now_ms() - tl);
            head = tail;
            tail = got[0];
            levels += tail > head;   // a level that decided something
        }
    }
    GM_HIP(hipMemsetAsync(g->d_count, 0, 8, c->stream));
    hipLaunchKernelGGL(loopy_final_kernel, all, wg, 0, c->stream, g->score, n, g->d_count);
    unsigned long long draws = 0;
    uint16_t rs = 0;
    GM_HIP(hipMemcpyAsync(&draws, g->d_count, 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipMemcpyAsync(&rs, g->score, 2, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    GM_HIP(hipGetLastError());
    const double t1 = now_ms();
    c->root = 0;
    c->root_record = graph_record(rs);
    c->n_positions = n;
    c->n_draw = draws;
    c->stats.n_positions = n;
    c->stats.n_primitive = n - interior;
    c->stats.n_tiers = levels;
    c->stats.n_edges = m;
    c->stats.solve_ms = t1 - t0;
    c->stats.forward_ms = t_rev - t_init;   // the reverse graph (count, scan, fill)
    c->stats.backward_ms = t1 - t_rev;      // the levels and the DRAW pass
    c->stats.table_bytes = n * 11 + m * 4 + n * 16 + 8 + npar * 4;
    c->tier_counts.clear();
    return GM_OK;
}

}  // namespace gm
