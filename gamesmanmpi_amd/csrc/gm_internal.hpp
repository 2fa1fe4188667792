// gm_internal.hpp -- context and helpers shared by the libgmsolve translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdarg.h>
#include <stdio.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/gmsolve.h"
#include "games.hpp"

namespace gm {

void set_error(const char *fmt, ...);

#define GM_HIP(expr)                                                              \
    do {                                                                          \
        hipError_t e_ = (expr);                                                   \
        if (e_ != hipSuccess) {                                                   \
            ::gm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                  \
            return GM_E_HIP;                                                      \
        }                                                                         \
    } while (0)

#define GM_TRY(expr)            \
    do {                        \
        int r_ = (expr);        \
        if (r_ != GM_OK) return r_; \
    } while (0)

#define GM_NCCL(expr)                                                              \
    do {                                                                           \
        ncclResult_t r_ = (expr);                                                  \
        if (r_ != ncclSuccess) {                                                   \
            ::gm::set_error("%s failed: %s", #expr, ncclGetErrorString(r_));       \
            return GM_E_COMM;                                                      \
        }                                                                          \
    } while (0)

// Device error flags written by kernels (bitwise OR).
enum : uint32_t {
    DEV_ERR_DRAW = 1,
    DEV_ERR_NOMOVES = 2,
    DEV_ERR_TABLE_FULL = 4,
    DEV_ERR_MISSING_CHILD = 8,
    DEV_ERR_OVERFLOW = 16,
    DEV_ERR_TIER = 32
};

int dev_error_to_gm(uint32_t flags);

struct DenseSub;
struct DenseBox;
struct SmallDense;
struct Sparse;
struct DistSub;
struct DistBox;
struct DistSparse;
struct Graph;
struct Hist;   // hist_common.hpp: counts by value and remoteness (gm_histogram)
struct VerifyDev;   // verify_common.hpp: the device accumulator of gm_verify
struct SelectDev;   // select_common.hpp: the filter and the device accumulator of gm_select
struct MovesReq;    // moves_common.hpp: the keys and the output arrays of gm_moves
struct ReachReq;    // reach_common.hpp: the starts, the policies and the outputs of gm_reach
struct ByteTables;  // byte_tables.hpp: where a byte-table SUBTRACT engine keeps its 1-byte codes
struct Engine;

struct Ctx {
    int game = 0;
    int device = 0;
    int32_t params[4] = {0, 0, 0, 0};
    DescF2O f2o;
    DescTTT ttt;
    DescToot toot;
    DescConnect con;
    DescOthello oth;
    DescSub sub;
    DescOthello8 oth8;       // GM_GAME_OTHELLO at 8x8: 128-bit keys (wide)
    bool wide = false;       // keys of more than 64 bits: gm_*_key entry points, the sharded sparse engine

    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    int engine_opt = GM_ENGINE_AUTO;
    int sub_low = 3;
    int sub_threads = 128;
    int sub_interleave = 20;     // 20 box engine at 8 heaps, else the walker (default); 10 walker, 6 four-block, 13 row dataflow, 1 one block
    int sub_order = 2;   // block order inside a tier: 0 key, 1 Morton, 2 Hilbert (default)
    bool use_graph = true;
    int timing = 0;          // 1: event pair around the dominant kernel's launches; 2 (split box engine) also per op

    // multi-GPU
    int rank = 0, world = 1;
    ncclComm_t comm = nullptr;   // made on first use from uid (ensure_comm): a transport that needs none never makes it
    bool have_uid = false;
    unsigned char uid[128] = {};
    int box_transport = 0;       // split box engine across processes: 0 RCCL, 1 peer copies over IPC (GM_OPT_BOX_TRANSPORT)
    int box_prepares = 0;        // split box contexts built so far (names the IPC rendezvous of each)
    int sparse_transport = 0;    // hash-sharded sparse engine across processes: 0 RCCL, 1 IPC pulls (GM_OPT_SPARSE_TRANSPORT)
    int sparse_solves = 0;       // sharded sparse solves run with the IPC transport (names each one's segment)
    int poison = 0;              // test hook (GM_OPT_POISON): received data pre-filled with 0xFF; 2 = early flag
    int virtual_ranks = 1;   // >1: run that many ranks inside this context (loopback transport)
    hipStream_t comm_stream = nullptr;
    int dist_batch = 4;      // sharded dense path: tiers per halo exchange
    int dist_slots = 4;      // sharded dense path: ring of exchange buffers, in batches
    int dist_solo = 0;       // diagnostic (loopback): enqueue only rank dist_solo-1's tier launches
    int dist_symmetry = 1;   // sharded dense path: halo blocks derivable by a heap swap are filled locally
    int dist_owner = 0;      // sharded dense path: 0 = split heaps in halves, 1 = tier-balanced comparisons
    int box_flow = -1;       // box engine, one GPU: -1 / 0 tier launches, 1 dataflow (GM_OPT_BOX_FLOW)
    bool box_flow_failed = false;   // a dataflow solve timed out: tier launches until GM_OPT_BOX_FLOW is set again
    int box_flow_fallbacks = 0;     // dataflow solves of this context that fell back to tier launches
    int box_split = 0;       // split box engine (N > 1): 0 halves, 1 comparisons (GM_OPT_BOX_SPLIT)
    int symmetry = 1;        // sparse engines: store one representative per symmetry orbit (games.hpp)
    int loopy = 0;           // graph engine: 1 = the loopy solve, cycles and DRAW allowed (GM_OPT_LOOPY)

    // results
    bool solved = false;
    const Engine *solved_by = nullptr;   // the engine whose table the context holds (set with solved)
    uint64_t root = 0;
    K128 root_wide{0, 0};    // a wide context's root (gm_solve_key, gm_import)
    // the root as Engine's entries take keys
    const void *root_key() const { return wide ? (const void *)&root_wide : (const void *)&root; }
    uint64_t n_positions = 0;
    uint16_t root_record = REC_UNSOLVED;
    uint64_t n_draw = 0;     // DRAW positions of the last solve (gm_draw_count): a loopy graph solve's, else 0
    gm_stats_t stats{};
    std::vector<uint64_t> tier_counts;
    // gm_histogram: the census a counts == NULL query computed, kept for the fill call that follows
    std::vector<uint64_t> hist_kept[3];
    uint64_t hist_kept_other = 0;
    bool hist_is_kept = false;

    // device buffer cache (dev_alloc / dev_free)
    std::vector<std::pair<void *, uint64_t>> buf_live, buf_cache;

    // adopted buffers
    void *adopted_dense = nullptr;
    uint64_t adopted_dense_bytes = 0;

    DenseSub *dsub = nullptr;
    DenseBox *dbox = nullptr;   // the box engine (GM_OPT_SUB_INTERLEAVE 20, 8 heaps)
    SmallDense *sd = nullptr;
    Sparse *sp = nullptr;
    DistSub *dist_sub = nullptr;
    DistBox *dist_box = nullptr;  // the box engine split over ranks (dist_box.hip)
    DistSparse *dist_sp = nullptr;
    Graph *graph = nullptr;
};

// One engine's entry points (each returns GM_OK or a GM_E_* code).  Every engine defines one
// record next to its functions; the solve entry points pick one from the context's options
// (gm_api.hip choose_engine) and store it in Ctx::solved_by, and every read of the solved table
// (export, query, digest, histogram, select, verify, moves, reach, poke, dense table, rank stats)
// goes through it.  Keys cross the record in the context's device key type -- uint64_t, or K128
// when Ctx::wide -- behind void pointers: gm_api.hip converts ABI words on the way in
// (device_keys) and orders and converts them on the way out (abi_sorted), an engine that stores
// one-word keys casts at the top of its entry, and the hash-sharded sparse engine, the one that
// also stores K128, dispatches on the descriptor (with_desc_wide).
struct Engine {
    int id;                                            // GM_ENGINE_*, reported as gm_stats_t.engine
    int (*solve)(Ctx *c, const void *root);            // null: the graph engine (graph_solve)
    int (*export_)(Ctx *c, void *keys, uint16_t *recs, uint64_t cap, uint64_t *n);   // ascending device keys
    int (*query)(Ctx *c, const void *keys, uint16_t *recs, uint64_t n);
    int (*digest)(Ctx *c, uint64_t *digest, uint64_t *n);
    int (*histogram)(Ctx *c, Hist *out);
    int (*select)(Ctx *c, const SelectDev &s);         // gm_select: every matching position into the accumulator
    int (*table)(Ctx *c, void **p, uint64_t *bytes);   // null: the engine has no dense table
    void (*free_)(Ctx *c);
    int (*verify)(Ctx *c, const VerifyDev &v);         // gm_verify: every stored position into the accumulator
    int (*poke)(Ctx *c, const void *key, uint16_t rec);   // gm_poke: one stored record overwritten (test hook)
    // gm_import: the table of root c->root (c->root_wide) built from n (key, record) pairs.  Sets
    // n_positions, tier_counts and the table's share of stats; on failure the caller frees the
    // engine.  null: the engine's tables cannot be imported
    int (*import_)(Ctx *c, const void *keys, const uint16_t *recs, uint64_t n);
    // gm_moves: every key's record, children (the plugin's gen_moves order), their records and
    // the mover's choice into the request's arrays (moves_common.hpp)
    int (*moves)(Ctx *c, const MovesReq &r);
    // the four byte-table SUBTRACT engines: the one description of their tables that the shared
    // readers of byte_tables.hpp (the byte_* entries of their records) work from, reached through
    // Ctx::solved_by.  null: another engine
    void (*bytes)(Ctx *c, ByteTables *t);
    // gm_reach: the closure of the request's starts under its move policies, level by level over
    // the engine's own marks (reach_common.hpp)
    int (*reach)(Ctx *c, const ReachReq &q);
};
// A record is host data, defined in the host pass only: the device pass of a translation unit
// would emit a const record too, with references to the host functions it names.
#ifdef __HIP_DEVICE_COMPILE__
#define GM_ENGINE_RECORD(name, ...)
#else
#define GM_ENGINE_RECORD(name, ...) const Engine name = {__VA_ARGS__};
#endif
extern const Engine graph_engine;         // graph.hip, graph_loopy.hip
extern const Engine small_dense_engine;   // small_dense.hip
extern const Engine dense_sub_engine;     // dense_sub.hip: the block engine
extern const Engine dense_box_engine;     // dense_box.hip: the box-tiled engine for 8 heaps
extern const Engine dist_box_engine;      // dist_box.hip: the box engine split over G ranks
extern const Engine dist_sub_engine;      // dist_sub.hip: the block engine partitioned over ranks
extern const Engine sparse_engine;        // sparse.hip
extern const Engine dist_sparse_engine;   // dist_sparse.hip: the hash-sharded sparse engine

// the box engine's pieces shared with the split box engine (dist_box.hip)
uint64_t box_hilbert(uint32_t box);
int box_grid_cap(int device);
void box_launch_split_flow(uint32_t grid, const void *ranks, uint32_t nranks, uint32_t ep, uint32_t *err,
                           uint64_t timeout_ticks, bool sys, hipStream_t s);
int box_split_flow_resident(int device);
// the split dataflow launch's per-rank descriptor (dense_box.hip BxSplitFlow), filled by dist_box.hip
struct BxSplitFlowDesc {
    uint8_t *table;
    const uint32_t *boxes, *fills, *srcs, *dsts, *groups;
    uint32_t qbase[8], qlen[8];
    uint32_t *flag;
    uint8_t *ptab[3];
    uint32_t *pflag[3];
};
void box_launch_tier_split(uint32_t grid, uint8_t *table, const uint32_t *boxes, const uint32_t *fills,
                           const uint32_t *srcs, const uint32_t *dsts, uint8_t *msg, uint8_t *const *peers,
                           uint32_t nbox, bool fill, hipStream_t s);
void box_tier_counts(uint64_t root, std::vector<uint64_t> &acc);
void box_region_keys(uint64_t root, uint64_t *keys, uint64_t n);
constexpr uint64_t BOX_QUERY_CHUNK = 1ull << 26;   // keys on the device at a time in a byte-table query (byte_tables.hpp)
// the split box engine's per-rank figures (gm_rank_stats, gm_rank_op_ms) and its plan (gm_box_plan)
int dist_box_rank_stats(Ctx *c, double *kernel_ms, uint64_t *boxes, uint64_t *recv_bytes, int cap, int *n);
int dist_box_op_ms(Ctx *c, int rank, double *ms, int cap, int *n);
int dist_box_plan(uint64_t root, int world, int rank, const int32_t *opts, int what, int axis, uint32_t *out,
                  uint64_t cap, uint64_t *n);

// the dense tier kernel, shared with the partitioned (multi-GPU) driver
bool sub_kernel_exists(int low, int high, int nt);
void launch_sub_tier(int low, int high, int nt, uint32_t nblocks, uint8_t *table, const uint32_t *list,
                     const uint8_t *zero, hipStream_t s);
// the sharded solve's byte-image tier kernel with per-block extra destinations (LOW = 3)
bool sub_kernel_x_exists(int high);
void launch_sub_tier_x(int high, uint32_t nblocks, uint8_t *table, const uint32_t *list, const uint8_t *zero,
                       const uint32_t *xoff, const uint64_t *xdst, hipStream_t s, int kind);
int sub_kernel_threads(const Ctx *c, int low);   // 0 = the 4-block interleaved kernel
void sort_tiers_morton(std::vector<uint32_t> &order, const std::vector<uint32_t> &tier_off, int high, int mode);

// gm_dist_plan, gm_sparse_layout: host only
int dist_sub_plan(int heaps, int world, int rank, const int32_t *opts, int what, int axis, uint32_t *off,
                  uint64_t off_cap, uint64_t *n_off, uint32_t *data, uint64_t data_cap, uint64_t *n_data);
int dist_sparse_layout(int G, int S, const uint64_t *mat, int r, uint64_t *seg, uint64_t *send_off,
                       uint64_t *recv_off, uint64_t *recv_seg);
int graph_solve(Ctx *c, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid);

double now_ms();

// Device buffers of the per-solve tables, cached per context and reused by the
// next solve (dev_free keeps the buffer; gm_close releases them).  Buffers are
// only used on the context's stream, so reuse is stream-ordered.  GM_TRACE=1
// logs every hipMalloc with its host time.
int dev_alloc(Ctx *c, void **p, uint64_t bytes);
void dev_free(Ctx *c, void *p);
bool trace_on();
int ensure_comm(Ctx *c);   // the RCCL communicator of gm_set_comm's unique id (collective on first use)

// A temporary device buffer of the read paths: plain hipMalloc / hipFree (not the dev_alloc
// cache, which would change what a context holds on to), freed when it leaves scope, so a
// GM_HIP / GM_TRY that returns early does not leak it.
template <class T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int alloc(uint64_t n) {
        GM_HIP(hipMalloc(&p, n * sizeof(T)));
        return GM_OK;
    }
    operator T *() const { return p; }
};

// keys up, one launch over them, records down: the dense engines' queries.  launch(dk, dr, m)
// enqueues the kernel for m keys; `chunk` bounds the keys on the device at a time.
template <class L>
inline int query_keys(Ctx *c, const uint64_t *keys, uint16_t *recs, uint64_t n, uint64_t chunk, L &&launch) {
    if (!n) return GM_OK;
    chunk = std::min(n, chunk);
    DevBuf<uint64_t> dk;
    DevBuf<uint16_t> dr;
    GM_TRY(dk.alloc(chunk));
    GM_TRY(dr.alloc(chunk));
    for (uint64_t o = 0; o < n; o += chunk) {
        const uint64_t m = std::min(chunk, n - o);
        GM_HIP(hipMemcpyAsync(dk, keys + o, m * 8, hipMemcpyHostToDevice, c->stream));
        launch(dk.p, dr.p, m);
        GM_HIP(hipMemcpyAsync(recs + o, dr, m * 2, hipMemcpyDeviceToHost, c->stream));
    }
    GM_HIP(hipStreamSynchronize(c->stream));
    return GM_OK;
}

// call f with the context's game descriptor: the six games with 64-bit keys
template <class C, class F>
inline int with_desc(C *c, F &&f) {
    switch (c->game) {
    case GM_GAME_FOUR_TO_ONE: return f(c->f2o);
    case GM_GAME_TTT: return f(c->ttt);
    case GM_GAME_TOOT: return f(c->toot);
    case GM_GAME_OTHELLO: return f(c->oth);
    case GM_GAME_SUBTRACT: return f(c->sub);
    case GM_GAME_CONNECT: return f(c->con);
    }
    set_error("unknown game");
    return GM_E_GAME;
}
// as with_desc, and Othello 8x8 (K128 keys) for a wide context
template <class C, class F>
inline int with_desc_wide(C *c, F &&f) {
    if (c->wide) return f(c->oth8);
    return with_desc(c, f);
}

}  // namespace gm

struct gm_ctx {
    gm::Ctx c;
};
