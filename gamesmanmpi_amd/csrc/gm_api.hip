// gm_api.hip -- the C ABI (include/gmsolve.h): contexts, dispatch, errors.
#include "gm_internal.hpp"
#include "hist_common.hpp"
#include "verify_common.hpp"
#include "select_common.hpp"
#include "moves_common.hpp"
#include "reach_common.hpp"

#include <hipcub/hipcub.hpp>

#include <chrono>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace gm {

static thread_local char g_err[512];

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int dev_error_to_gm(uint32_t f) {
    if (f & DEV_ERR_DRAW) { set_error("a DRAW primitive was reached (unsupported)"); return GM_E_DRAW; }
    if (f & DEV_ERR_NOMOVES) { set_error("a non-primitive position has no moves"); return GM_E_NOMOVES; }
    if (f & DEV_ERR_TIER) { set_error("descriptor tier does not increase by 1..MAX_SKIP along a move"); return GM_E_GAME; }
    if (f & DEV_ERR_TABLE_FULL) { set_error("tier table overflow"); return GM_E_NOMEM; }
    if (f & DEV_ERR_MISSING_CHILD) { set_error("retrograde found a child missing from its tier table"); return GM_E_STATE; }
    if (f & DEV_ERR_OVERFLOW) { set_error("remoteness exceeds 14 bits"); return GM_E_CAP; }
    set_error("device error flags 0x%x", f);
    return GM_E_STATE;
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

bool trace_on() {
    static const bool on = getenv("GM_TRACE") && atoi(getenv("GM_TRACE"));
    return on;
}

// The communicator is made when a solve first needs it -- every rank's first sharded solve,
// so the call is collective as RCCL requires -- and not at all for a transport that needs none
// (the split box engine's IPC peer copies, which also run when the ranks share one GPU, where
// RCCL refuses to make a communicator).
int ensure_comm(Ctx *c) {
    if (c->comm) return GM_OK;
    if (!c->have_uid) {
        set_error("a %d-rank solve needs gm_set_comm with a unique id", c->world);
        return GM_E_COMM;
    }
    ncclUniqueId id;
    memcpy(&id, c->uid, sizeof id);
    GM_HIP(hipSetDevice(c->device));
    GM_NCCL(ncclCommInitRank(&c->comm, c->world, id, c->rank));
    return GM_OK;
}

// Best fit from the context's cache of released buffers (no more than 2x the
// request), else hipMalloc; if that fails, release the cache and retry once.
int dev_alloc(Ctx *c, void **p, uint64_t bytes) {
    bytes = std::max<uint64_t>(bytes, 256);
    size_t best = c->buf_cache.size();
    for (size_t i = 0; i < c->buf_cache.size(); i++) {
        const uint64_t sz = c->buf_cache[i].second;
        if (sz >= bytes && sz <= 2 * bytes && (best == c->buf_cache.size() || sz < c->buf_cache[best].second))
            best = i;
    }
    if (best < c->buf_cache.size()) {
        *p = c->buf_cache[best].first;
        c->buf_live.push_back(c->buf_cache[best]);
        c->buf_cache.erase(c->buf_cache.begin() + best);
        return GM_OK;
    }
    const double t0 = trace_on() ? now_ms() : 0;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(c->stream);
        for (auto &b : c->buf_cache) (void)hipFree(b.first);
        c->buf_cache.clear();
        e = hipMalloc(p, bytes);
    }
    if (trace_on()) fprintf(stderr, "[gm] hipMalloc %.3f GB in %.2f ms\n", bytes / 1e9, now_ms() - t0);
    if (e != hipSuccess) {
        *p = nullptr;
        set_error("out of device memory (%llu bytes): %s", (unsigned long long)bytes, hipGetErrorString(e));
        return GM_E_NOMEM;
    }
    c->buf_live.emplace_back(*p, bytes);
    return GM_OK;
}

// Return a buffer to the cache: a fresh multi-GB hipMalloc after a hipFree can
// stall for seconds (measured: 8.6 GB in 4.9 s on the second Toot 6x4 solve),
// so repeated solves reuse the previous solve's buffers instead.
void dev_free(Ctx *c, void *p) {
    if (!p) return;
    for (size_t i = 0; i < c->buf_live.size(); i++)
        if (c->buf_live[i].first == p) {
            c->buf_cache.push_back(c->buf_live[i]);
            c->buf_live.erase(c->buf_live.begin() + i);
            return;
        }
    (void)hipFree(p);   // not ours: plain free
}

// The engine of a gm_solve, from the context's options: dense (SUBTRACT, tic-tac-toe) or sparse,
// for the dense 8-heap game the box engine (GM_OPT_SUB_INTERLEAVE 20) or the block engine, and
// one GPU or -- `sharded` -- split / partitioned / hash-sharded over ranks.  GM_ENGINE_DIST_SPARSE
// forces the hash-sharded engine, e.g. over a one-rank communicator.
static const Engine *choose_engine(const Ctx *c, bool sharded) {
    const bool dense_game = c->game == GM_GAME_SUBTRACT || c->game == GM_GAME_TTT;
    // forced, or a wide game: the one engine that stores wide keys
    if (c->engine_opt == GM_ENGINE_DIST_SPARSE || c->wide) return &dist_sparse_engine;
    if (c->engine_opt == GM_ENGINE_SPARSE || !dense_game) return sharded ? &dist_sparse_engine : &sparse_engine;
    if (c->game == GM_GAME_TTT) return sharded ? &dist_sparse_engine : &small_dense_engine;
    // the 8-heap game on the box engine splits in dist_box.hip; other heap counts and
    // GM_OPT_SUB_INTERLEAVE != 20 keep the block engine and its partitioned path
    if (c->sub.heaps == 8 && c->sub_interleave == 20) return sharded ? &dist_box_engine : &dense_box_engine;
    return sharded ? &dist_sub_engine : &dense_sub_engine;
}

static bool key_valid(const Ctx *c, uint64_t k) {
    return with_desc(c, [&](const auto &d) { return (int)d.valid(k); }) > 0;
}

// ---------------------------------------------------------------- keys across the ABI
// The ABI speaks key words (gm_key_words() per key), the engines the context's device key type
// (gm_internal.hpp Engine).  The codec of a multi-word game is named here and nowhere below:
// Othello 8x8, whose 144-bit position string is three words and whose device key is a K128.
static int key_words(const Ctx *c) { return c->wide ? 3 : 1; }
static size_t key_bytes(const Ctx *c) { return c->wide ? sizeof(K128) : 8; }
static bool key_from_words(const Ctx *, const uint64_t *w, void *key) { return DescOthello8::from_words(w, (K128 *)key); }
static void key_to_words(const Ctx *, const void *key, uint64_t *w) { DescOthello8::to_words(*(const K128 *)key, w); }

static int refuse_wide(const Ctx *c, const char *call) {
    if (c->wide) { set_error("this game's keys have %d words: %s_key", key_words(c), call); return GM_E_ARG; }
    return GM_OK;
}

// what device_keys makes of words that are no position
enum class BadKey {
    Fails,     // GM_E_KEY, the error names the key's index
    Unsolved,  // the all-zero key, which no table holds; the index goes to DeviceKeys::bad (record 0xFFFF)
    Skipped    // the all-zero key, which the engines' moves and reach pass over
};
struct DeviceKeys {
    const void *p = nullptr;            // n keys of the context's device key type
    std::vector<unsigned char> held;    // ... held here on a wide context; a one-word context's are the caller's words
    std::vector<uint64_t> bad;
};
// ABI words to device keys.  A one-word context's words are its keys: no copy, and whether a key
// is a position is the engine's affair
static int device_keys(const Ctx *c, const uint64_t *words, uint64_t n, BadKey bad, const char *what, DeviceKeys *out) {
    out->p = words;
    if (!c->wide) return GM_OK;
    const size_t KB = key_bytes(c), W = key_words(c);
    out->held.assign(n * KB, 0);
    out->p = out->held.data();
    for (uint64_t i = 0; i < n; i++) {
        if (key_from_words(c, words + W * i, &out->held[i * KB])) continue;
        memset(&out->held[i * KB], 0, KB);
        if (bad == BadKey::Unsolved) out->bad.push_back(i);
        if (bad != BadKey::Fails) continue;
        std::string hex;
        char one[24];
        for (size_t j = 0; j < W; j++) { snprintf(one, sizeof one, " 0x%llx", (unsigned long long)words[W * i + j]); hex += one; }
        set_error("%s%s (index %llu) is not a valid position", what, hex.c_str(), (unsigned long long)i);
        return GM_E_KEY;
    }
    return GM_OK;
}

// Device keys to ABI words in ascending ABI order (a multi-word key: the position string as one
// integer, its last word the most significant).  Returns the permutation -- words of row i are
// those of keys[perm[i]] -- so that a caller can carry records and sides along.
static std::vector<uint64_t> abi_sorted(const Ctx *c, const void *keys, uint64_t n, uint64_t *words) {
    const size_t KB = key_bytes(c), W = key_words(c);
    std::vector<uint64_t> w(c->wide ? W * n : 0), perm(n);
    for (uint64_t i = 0; i < n; i++) {
        perm[i] = i;
        if (c->wide) key_to_words(c, (const unsigned char *)keys + i * KB, &w[W * i]);
    }
    const uint64_t *src = c->wide ? w.data() : (const uint64_t *)keys;
    std::sort(perm.begin(), perm.end(), [&](uint64_t a, uint64_t b) {
        for (size_t j = W; j-- > 0;)
            if (src[W * a + j] != src[W * b + j]) return src[W * a + j] < src[W * b + j];
        return false;
    });
    for (uint64_t i = 0; i < n; i++)
        for (size_t j = 0; j < W; j++) words[W * i + j] = src[W * perm[i] + j];
    return perm;
}

// keys per chunk of gm_moves: GM_MOVES_CHUNK (a development variable, as GM_SPARSE_BATCH) lets a
// test cross a chunk boundary with a small table
static uint64_t moves_chunk() {
    const char *e = getenv("GM_MOVES_CHUNK");
    const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? std::min<uint64_t>(v, 1ull << 30) : MOVES_CHUNK;   // the scan counts its items in an int
}

// The chunk loop of gm_moves (moves_common.hpp).  Per chunk: keys up, the engine's count pass,
// the exclusive sum of the counts (one slot past the chunk holds 0, so its sum is the chunk's
// total), the engine's fill pass into child buffers of exactly that total, heads and children
// down at the running offset.  The caller's child arrays must stay untouched when they are too
// small, and the total is known only after every chunk's count pass: a call of more than one
// chunk that wants children counts all chunks first.
int moves_run(Ctx *c, const MovesReq &r, const std::function<int(const MovesDev &)> &pass) {
    *r.n_children = 0;
    if (!r.n) return GM_OK;
    const uint64_t chunk = std::min(r.n, moves_chunk());
    const int W = r.words;
    bool want = r.child_words && r.cap;
    DevBuf<unsigned char> dk, dscan;
    DevBuf<uint64_t> dcount, dfirst, dcw;
    DevBuf<uint16_t> dcr;
    DevBuf<gm_moves_t> dh;
    GM_TRY(dk.alloc(chunk * r.key_bytes));
    GM_TRY(dcount.alloc(chunk + 1));
    GM_TRY(dfirst.alloc(chunk + 1));
    GM_TRY(dh.alloc(chunk));
    size_t scan_bytes = 0;
    GM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, dcount.p, dfirst.p, (int)(chunk + 1), c->stream));
    GM_TRY(dscan.alloc(std::max<size_t>(scan_bytes, 1)));
    // the count pass and the scan of keys [o, o + m): *ct = the chunk's children
    auto count_chunk = [&](uint64_t o, uint64_t m, MovesDev *mv, uint64_t *ct) -> int {
        GM_HIP(hipMemcpyAsync(dk, (const unsigned char *)r.keys + o * r.key_bytes, m * r.key_bytes, hipMemcpyHostToDevice,
                              c->stream));
        GM_HIP(hipMemsetAsync(dcount.p + m, 0, 8, c->stream));
        *mv = MovesDev{dk.p, m, dcount.p, dfirst.p, dh.p, nullptr, nullptr, 0, 0};
        GM_TRY(pass(*mv));
        GM_HIP(hipcub::DeviceScan::ExclusiveSum(dscan.p, scan_bytes, dcount.p, dfirst.p, (int)(m + 1), c->stream));
        GM_HIP(hipMemcpyAsync(ct, dfirst.p + m, 8, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        return GM_OK;
    };
    MovesDev mv;
    uint64_t ct = 0;
    if (want && r.n > chunk) {
        uint64_t total = 0;
        for (uint64_t o = 0; o < r.n; o += chunk) {
            GM_TRY(count_chunk(o, std::min(chunk, r.n - o), &mv, &ct));
            total += ct;
        }
        want = total <= r.cap;
    }
    uint64_t base = 0, have_w = 0, have_r = 0;
    for (uint64_t o = 0; o < r.n; o += chunk) {
        const uint64_t m = std::min(chunk, r.n - o);
        GM_TRY(count_chunk(o, m, &mv, &ct));
        if (want && base + ct > r.cap) want = false;   // one chunk: nothing has been written yet
        if (want && ct) {
            if (have_w < ct) {
                if (dcw.p) { (void)hipFree(dcw.p); dcw.p = nullptr; }
                GM_TRY(dcw.alloc(ct * W));
                have_w = ct;
            }
            if (r.child_records && have_r < ct) {
                if (dcr.p) { (void)hipFree(dcr.p); dcr.p = nullptr; }
                GM_TRY(dcr.alloc(ct));
                have_r = ct;
            }
            mv.child_words = dcw.p;
            mv.child_records = r.child_records ? dcr.p : nullptr;
        }
        mv.base = base;
        mv.fill = 1;
        GM_TRY(pass(mv));
        GM_HIP(hipMemcpyAsync(r.heads + o, dh.p, m * sizeof(gm_moves_t), hipMemcpyDeviceToHost, c->stream));
        if (mv.child_words) {
            GM_HIP(hipMemcpyAsync(r.child_words + base * W, dcw.p, ct * W * 8, hipMemcpyDeviceToHost, c->stream));
            if (mv.child_records)
                GM_HIP(hipMemcpyAsync(r.child_records + base, dcr.p, ct * 2, hipMemcpyDeviceToHost, c->stream));
        }
        GM_HIP(hipStreamSynchronize(c->stream));
        base += ct;
    }
    *r.n_children = base;
    if (r.child_words && r.cap && base > r.cap) {
        set_error("gm_moves: the child arrays hold %llu, need %llu", (unsigned long long)r.cap, (unsigned long long)base);
        return GM_E_CAP;
    }
    return GM_OK;
}

// frontier entries per launch of gm_reach: GM_REACH_CHUNK (a development variable, as
// GM_MOVES_CHUNK) lets a test cross chunk boundaries with a small table
static uint64_t reach_chunk() {
    const char *e = getenv("GM_REACH_CHUNK");
    const uint64_t v = e ? strtoull(e, nullptr, 10) : 0;
    return v ? std::min<uint64_t>(v, 1ull << 30) : REACH_CHUNK;
}

// The level loop of gm_reach (reach_common.hpp).  The starts are uploaded in chunks and marked
// at side 0 by a seed launch; then, per ply, the frontier is fed to the engine's level kernel
// in chunks, the accumulator read back (one synchronisation per level: the next frontier's
// size decides the next launches), and the two frontiers swapped.  The next frontier is sized
// from what can still be marked and from the frontier's size times the move count.
int reach_run(Ctx *c, const ReachReq &q, const ReachDims &dim, const std::function<int(const ReachDev &)> &level,
              const std::function<int(const ReachDev &)> &sweep) {
    const uint64_t KB = q.key_bytes, chunk = reach_chunk();
    gm_reach_out_t o{};
    q.ply_counts->clear();
    q.keys->clear();
    q.recs->clear();
    q.sides->clear();
    DevBuf<uint32_t> marks;
    DevBuf<unsigned long long> acc;
    const uint64_t words = std::max<uint64_t>(1, (dim.units + 15) / 16);
    GM_TRY(marks.alloc(words));
    GM_TRY(acc.alloc(RA_WORDS));
    GM_HIP(hipMemsetAsync(marks, 0, words * 4, c->stream));
    GM_HIP(hipMemsetAsync(acc, 0, RA_WORDS * 8, c->stream));
    DevBuf<unsigned char> fr[2];
    uint64_t have[2] = {0, 0};
    auto need = [&](int w, uint64_t n) -> int {
        if (have[w] >= n && fr[w].p) return GM_OK;
        if (fr[w].p) { (void)hipFree(fr[w].p); fr[w].p = nullptr; }
        GM_TRY(fr[w].alloc(std::max<uint64_t>(n, 1) * KB));
        have[w] = n;
        return GM_OK;
    };
    unsigned long long h[RA_WORDS];
    auto read_acc = [&]() -> int {
        GM_HIP(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        if (h[RA_OVER]) { set_error("gm_reach: a frontier outgrew its bound"); return GM_E_STATE; }
        return GM_OK;
    };
    ReachDev r{};
    r.marks = marks;
    r.acc = acc;
    // the starts: marked themselves, at side 0
    int cur = 0;
    {
        const uint64_t up = std::min(q.n_starts, chunk);
        DevBuf<unsigned char> in;
        GM_TRY(in.alloc(std::max<uint64_t>(up, 1) * KB));
        r.next_cap = std::min(q.n_starts, dim.positions);
        GM_TRY(need(cur, r.next_cap));
        r.next = fr[cur].p;
        r.seed = 1;
        r.side = 0;
        for (uint64_t s = 0; s < q.n_starts; s += up) {
            r.m = std::min(up, q.n_starts - s);
            GM_HIP(hipMemcpyAsync(in, (const unsigned char *)q.starts + s * KB, r.m * KB, hipMemcpyHostToDevice, c->stream));
            r.in = in.p;
            GM_TRY(level(r));
        }
        GM_TRY(read_acc());   // synchronised: `in` may leave scope
        r.seed = 0;
    }
    uint64_t f = h[RA_CURSOR], marked = f;
    if (f) q.ply_counts->push_back(h[RA_PAIRS]);
    for (uint32_t ply = 0; f; ply++) {
        if (q.how.max_plies && ply >= q.how.max_plies) break;
        uint64_t bound = 2 * dim.positions - marked;
        if (dim.max_moves) bound = std::min(bound, f * dim.max_moves);
        if (!bound) break;   // every (position, side) is marked
        GM_TRY(need(1 - cur, bound));
        GM_HIP(hipMemsetAsync(acc, 0, 16, c->stream));   // the cursor and the level's pairs
        r.next = fr[1 - cur].p;
        r.next_cap = bound;
        r.side = (ply + 1) & 1u;
        r.policy = ply & 1u ? q.how.other : q.how.mover;
        for (uint64_t s = 0; s < f; s += chunk) {
            r.in = fr[cur].p + s * KB;
            r.m = std::min(chunk, f - s);
            GM_TRY(level(r));
        }
        GM_TRY(read_acc());
        f = h[RA_CURSOR];
        marked += f;
        if (f) q.ply_counts->push_back(h[RA_PAIRS]);
        cur = 1 - cur;
    }
    o.n = h[RA_FRESH];
    for (size_t d = 0; d < q.ply_counts->size(); d++) (d & 1 ? o.n_other : o.n_mover) += (*q.ply_counts)[d];
    o.n_starts = h[RA_STARTS];
    o.edges = h[RA_EDGES];
    o.missing = h[RA_MISSING];
    o.plies = (int32_t)q.ply_counts->size();
    *q.out = o;
    const uint64_t want = std::min(q.cap, o.n);
    if (!want) return GM_OK;
    // the list: the frontiers go first, then one sweep over the marks
    for (auto &b : fr)
        if (b.p) { (void)hipFree(b.p); b.p = nullptr; }
    DevBuf<unsigned char> dk, ds;
    DevBuf<uint16_t> dr;
    GM_TRY(dk.alloc(want * KB));
    GM_TRY(dr.alloc(want));
    GM_TRY(ds.alloc(want));
    GM_HIP(hipMemsetAsync(acc, 0, 8, c->stream));
    r.keys = dk.p;
    r.recs = dr.p;
    r.sides = ds.p;
    r.cap = want;
    GM_TRY(sweep(r));
    GM_TRY(read_acc());
    const uint64_t m = std::min<uint64_t>(h[RA_CURSOR], want);
    q.keys->resize(m * KB);
    q.recs->resize(m);
    q.sides->resize(m);
    if (m) {
        GM_HIP(hipMemcpyAsync(q.keys->data(), dk, m * KB, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipMemcpyAsync(q.recs->data(), dr, m * 2, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipMemcpyAsync(q.sides->data(), ds, m, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
    }
    return GM_OK;
}

static void free_engines(Ctx *c) {
    for (const Engine *e : {&graph_engine, &dense_sub_engine, &dense_box_engine, &small_dense_engine, &sparse_engine,
                            &dist_sub_engine, &dist_box_engine, &dist_sparse_engine})
        e->free_(c);
}

// ---------------------------------------------------------------- around a solve or an import
// A root from ABI words: GM_E_KEY unless it is a position.  Checked before solve_begin, so that
// a refused root leaves the context's table alone (gm_solve) ...
struct Root {
    uint64_t one = 0;
    DeviceKeys wide;
};
static int parse_root(const Ctx *c, const uint64_t *words, const char *call, Root *r) {
    if (c->wide) return device_keys(c, words, 1, BadKey::Fails, call, &r->wide);
    if (!key_valid(c, words[0])) {
        set_error("%s 0x%llx is not a valid position", call, (unsigned long long)words[0]);
        return GM_E_KEY;
    }
    r->one = words[0];
    return GM_OK;
}
// ... and made the context's after it, with the symmetry reduction of a solve from it (games.hpp):
// Toot-and-Otto's and Connect's mirror when the root is its own mirror image, Othello's board symmetries that
// fix the root (DescOthello::sym)
static void set_root(Ctx *c, const Root &r) {
    c->root = r.one;
    if (c->wide) memcpy(&c->root_wide, r.wide.p, sizeof c->root_wide);
    if (c->game == GM_GAME_TOOT) c->toot.sym = (c->symmetry && c->toot.mirror(c->root) == c->root) ? 1u : 0u;
    if (c->game == GM_GAME_CONNECT) c->con.sym = (c->symmetry && c->con.mirror(c->root) == c->root) ? 1u : 0u;
    if (c->game == GM_GAME_OTHELLO && !c->wide) c->oth.sym = c->symmetry ? c->oth.stabilizer(c->root) : 0u;
}

// From here on the context no longer holds a table, so a failure leaves it unsolved; the stats
// are the coming solve's.  keep_launches: gm_solve under GM_OPT_TIMING accumulates them
static void solve_begin(Ctx *c, int world, bool keep_launches) {
    c->solved = false;
    c->solved_by = nullptr;
    c->hist_is_kept = false;
    c->n_draw = 0;
    const int32_t launches = keep_launches ? c->stats.kernel_launches : 0;
    c->stats = gm_stats_t{};
    c->stats.kernel_launches = launches;
    c->stats.world = world;
}

static int solve_finish(Ctx *c, const Engine *e, int world, uint64_t *n_positions, uint16_t *root_record) {
    if (!c->stats.n_stored) c->stats.n_stored = c->stats.n_positions;   // engines without a symmetry reduction
    c->stats.engine = e->id;
    c->stats.world = world;
    c->solved = true;
    c->solved_by = e;
    if (n_positions) *n_positions = c->n_positions;
    if (root_record) *root_record = c->root_record;
    return GM_OK;
}

// The communicator of a solve by engine e.  Virtual ranks run inside the context and need none.
// Otherwise two rules say whether the solve has ranks to connect:
//   one-word keys   `sharded`: more than one process, or GM_ENGINE_DIST_SPARSE forced (e.g. over
//                   a one-rank communicator); such a solve insists on a unique id
//   wide keys       the hash-sharded engine is the only engine, so one process without a unique
//                   id is simply G = 1; ranks are connected when there are several or an id was set
// A transport that needs no communicator (the split box engine's IPC stores, the sparse engine's
// IPC pulls; both also run with the ranks sharing one GPU, where RCCL refuses) still needs the
// unique id: it names the rendezvous.
static int solve_comm(Ctx *c, const Engine *e, bool sharded) {
    if (c->world > 1 && c->virtual_ranks > 1) {
        set_error("virtual ranks and a multi-process communicator are exclusive");
        return GM_E_ARG;
    }
    if (c->virtual_ranks > 1) return GM_OK;
    const bool ranks = c->wide ? (c->world > 1 || c->have_uid) : sharded;
    if (!ranks) return GM_OK;
    const bool no_comm = e == &dist_box_engine ? c->box_transport == 1
                                               : (e == &dist_sparse_engine && c->sparse_transport == 1);
    if (!c->have_uid) {
        if (no_comm) set_error("the IPC transport needs gm_set_comm with a unique id (it names the rendezvous)");
        else set_error("a %d-rank solve of this game needs an RCCL communicator (gm_set_comm with a unique id)", c->world);
        return GM_E_COMM;
    }
    return no_comm ? (int)GM_OK : ensure_comm(c);
}

// each dense SUBTRACT engine holds (or adopts) a whole table: choosing one releases the other two's
static void release_other_dense(Ctx *c, const Engine *e) {
    if (e == &dense_box_engine || e == &dist_box_engine || e == &dense_sub_engine)
        for (const Engine *o : {&dense_sub_engine, &dense_box_engine, &dist_box_engine})
            if (o != e) o->free_(c);
}

static int need_device(const Ctx *c) {
    if (c->device < 0) { set_error("no HIP device is visible: the solver needs an MI355X (gfx950)"); return GM_E_HIP; }
    return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" {

static int need_solved(gm_ctx *h);

int gm_version(void) { return GM_ABI_VERSION; }

const char *gm_last_error(void) { return g_err; }

int gm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int gm_open(int game, const int32_t *params, int nparams, int device, gm_ctx **out) {
    if (!out) { set_error("out is NULL"); return GM_E_ARG; }
    *out = nullptr;
    if (nparams < 0 || nparams > 4 || (nparams && !params)) { set_error("bad params"); return GM_E_ARG; }
    gm_ctx *h = new gm_ctx();
    Ctx *c = &h->c;
    c->game = game;
    for (int i = 0; i < nparams; i++) c->params[i] = params[i];
    bool ok = true;
    switch (game) {
    case GM_GAME_FOUR_TO_ONE: case GM_GAME_TTT: case GM_GAME_GRAPH: break;
    case GM_GAME_TOOT:
        ok = DescToot::make(nparams > 0 ? params[0] : 6, nparams > 1 ? params[1] : 4, &c->toot);
        break;
    case GM_GAME_OTHELLO:
        // 8x8 (the reference plugin's default board, othello_bit_new.py:8): 128-bit keys
        c->wide = nparams > 1 && params[0] == 8 && params[1] == 8;
        ok = c->wide || DescOthello::make(nparams > 0 ? params[0] : 4, nparams > 1 ? params[1] : 4, &c->oth);
        break;
    case GM_GAME_SUBTRACT:
        c->sub.heaps = nparams > 0 ? params[0] : 8;
        ok = c->sub.heaps >= 1 && c->sub.heaps <= 8;
        break;
    case GM_GAME_CONNECT:
        ok = DescConnect::make(nparams > 0 ? params[0] : 5, nparams > 1 ? params[1] : 4, nparams > 2 ? params[2] : 4,
                               &c->con);
        break;
    default:
        ok = false;
    }
    if (!ok) {
        set_error("game %d with these parameters is not supported", game);
        delete h;
        return GM_E_GAME;
    }
    int ndev = gm_device_count();
    if (ndev <= 0) {
        // Contexts can still be used for gm_pack_initial / gm_expand_host.
        c->device = -1;
        *out = h;
        return GM_OK;
    }
    if (device < 0) {
        if (hipGetDevice(&c->device) != hipSuccess) c->device = 0;
    } else {
        if (device >= ndev) { set_error("device %d out of range (%d visible)", device, ndev); delete h; return GM_E_ARG; }
        c->device = device;
    }
    if (hipSetDevice(c->device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("cannot initialise HIP device %d", c->device);
        delete h;
        return GM_E_HIP;
    }
    c->stream = c->own_stream;
    *out = h;
    return GM_OK;
}

int gm_set_stream(gm_ctx *h, void *s) {
    if (!h) return GM_E_ARG;
    h->c.stream = s ? (hipStream_t)s : h->c.own_stream;
    return GM_OK;
}

int gm_set_option(gm_ctx *h, int opt, int64_t v) {
    if (!h) return GM_E_ARG;
    Ctx *c = &h->c;
    switch (opt) {
    case GM_OPT_ENGINE:
        if (v < GM_ENGINE_AUTO || (v > GM_ENGINE_SPARSE && v != GM_ENGINE_DIST_SPARSE)) {
            set_error("bad engine");
            return GM_E_ARG;
        }
        c->engine_opt = (int)v;
        return GM_OK;
    case GM_OPT_SUB_LOW:
        if (v < 1 || v > 3) { set_error("sub_low must be 1..3"); return GM_E_ARG; }
        c->sub_low = (int)v;
        return GM_OK;
    case GM_OPT_GRAPH: c->use_graph = v != 0; return GM_OK;
    case GM_OPT_TIMING:
        if (v < 0 || v > 2) { set_error("timing must be 0, 1 or 2"); return GM_E_ARG; }
        c->timing = (int)v;
        return GM_OK;
    case GM_OPT_SUB_THREADS:
        if (v != 64 && v != 128 && v != 256) { set_error("sub_threads must be 64, 128 or 256"); return GM_E_ARG; }
        c->sub_threads = (int)v;
        return GM_OK;
    case GM_OPT_SUB_INTERLEAVE:
        if (v != 1 && v != 6 && v != 10 && v != 20) {
            set_error("sub_interleave must be 1 (one block per workgroup), 6 (four-block kernel), 10 (walker) "
                      "or 20 (box engine, 8 heaps)");
            return GM_E_ARG;
        }
        c->sub_interleave = (int)v;
        return GM_OK;
    case GM_OPT_SUB_ORDER:
        if (v < 0 || v > 2) { set_error("sub_order must be 0, 1 or 2"); return GM_E_ARG; }
        c->sub_order = (int)v;
        return GM_OK;
    case GM_OPT_DIST_BATCH:
        if (v < 1 || v > 128) { set_error("dist_batch must be 1..128"); return GM_E_ARG; }
        c->dist_batch = (int)v;
        return GM_OK;
    case GM_OPT_DIST_SLOTS:
        if (v < 1 || v > 128) { set_error("dist_slots must be 1..128"); return GM_E_ARG; }
        c->dist_slots = (int)v;
        return GM_OK;
    case GM_OPT_DIST_SYMMETRY:
        if (v < 0 || v > 1) { set_error("dist_symmetry must be 0 or 1"); return GM_E_ARG; }
        c->dist_symmetry = (int)v;
        return GM_OK;
    case GM_OPT_DIST_OWNER:
        if (v < 0 || v > 1) { set_error("dist_owner must be 0 or 1"); return GM_E_ARG; }
        c->dist_owner = (int)v;
        return GM_OK;
    case GM_OPT_DIST_SOLO:
        if (v < 0 || v > 64) { set_error("dist_solo must be 0..64"); return GM_E_ARG; }
        c->dist_solo = (int)v;
        return GM_OK;
    case GM_OPT_BOX_FLOW:
        if (v < -1 || v > 1) { set_error("box flow must be -1, 0 or 1"); return GM_E_ARG; }
        c->box_flow = (int)v;
        c->box_flow_failed = false;   // setting it again retries the dataflow launch
        return GM_OK;
    case GM_OPT_BOX_TRANSPORT:
        if (v < 0 || v > 1) { set_error("GM_OPT_BOX_TRANSPORT must be 0 (RCCL) or 1 (IPC peer copies)"); return GM_E_ARG; }
        c->box_transport = (int)v;
        return GM_OK;
    case GM_OPT_SPARSE_TRANSPORT:
        if (v < 0 || v > 1) { set_error("GM_OPT_SPARSE_TRANSPORT must be 0 (RCCL) or 1 (IPC pulls)"); return GM_E_ARG; }
        c->sparse_transport = (int)v;
        return GM_OK;
    case GM_OPT_POISON:
        if (v < 0 || v > 3) { set_error("GM_OPT_POISON must be 0..3"); return GM_E_ARG; }
        c->poison = (int)v;
        return GM_OK;
    case GM_OPT_BOX_SPLIT:
        if (v < 0 || v > 1) { set_error("box split must be 0 (halves) or 1 (comparisons)"); return GM_E_ARG; }
        c->box_split = (int)v;
        return GM_OK;
    case GM_OPT_SYMMETRY:
        if (v < 0 || v > 1) { set_error("symmetry must be 0 or 1"); return GM_E_ARG; }
        c->symmetry = (int)v;
        return GM_OK;
    case GM_OPT_VIRTUAL_RANKS:
        if (v < 1 || v > 64) { set_error("virtual ranks must be 1..64"); return GM_E_ARG; }
        c->virtual_ranks = (int)v;
        return GM_OK;
    case GM_OPT_LOOPY:
        if (c->game != GM_GAME_GRAPH) { set_error("GM_OPT_LOOPY is the graph engine's: a GM_GAME_GRAPH context"); return GM_E_ARG; }
        if (v < 0 || v > 1) { set_error("loopy must be 0 or 1"); return GM_E_ARG; }
        c->loopy = (int)v;
        return GM_OK;
    }
    set_error("unknown option %d", opt);
    return GM_E_ARG;
}

int gm_pack_initial(gm_ctx *h, uint64_t *key) {
    if (!h || !key) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_TRY(refuse_wide(c, "gm_pack_initial"));
    switch (c->game) {
    case GM_GAME_FOUR_TO_ONE: *key = 4; return GM_OK;   // four_to_one.py:8-10
    case GM_GAME_TTT: *key = 0; return GM_OK;           // empty board
    case GM_GAME_TOOT: *key = 0x6666; return GM_OK;     // empty planes, hands 6/6/6/6 (:36-44)
    case GM_GAME_OTHELLO: {                              // othello_bit_new.py:36-55
        const DescOthello &o = c->oth;
        int L = o.L, A = o.A;
        auto bit = [&](int x, int y) { return 1u << (A - 1 - (L * y + x)); };   // rotated plane bit
        uint32_t w = bit(L / 2 - 1, L / 2 - 1) | bit(L / 2, L / 2);
        uint32_t b = bit(L / 2 - 1, L / 2) | bit(L / 2, L / 2 - 1);
        *key = ((uint64_t)w << (A + 16)) | ((uint64_t)b << 16) | (2ull << 8);
        return GM_OK;
    }
    case GM_GAME_SUBTRACT: *key = (1ull << (4 * c->sub.heaps)) - 1; return GM_OK;
    case GM_GAME_CONNECT: *key = c->con.bottom; return GM_OK;   // every column's cap at row 0
    }
    return GM_E_GAME;
}

int gm_expand_host(gm_ctx *h, uint64_t key, uint64_t *children, int cap, int *n, int *prim, int64_t *tier) {
    if (!h || !n || !prim || !tier) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_TRY(refuse_wide(c, "gm_expand_host"));
    uint64_t kids[32];
    int p = UNDECIDED, k = 0;
    int64_t t = 0;
    if (!key_valid(c, key)) { set_error("key is not a valid position"); return GM_E_KEY; }
    GM_TRY(with_desc(c, [&](const auto &reduced) {
        const auto d = unreduced(reduced);   // the plugin's own moves: no symmetry reduction (Toot, Connect, Othello)
        p = d.primitive(key);
        t = d.tier(key);
        if (p == UNDECIDED) k = d.children(key, kids);
        return GM_OK;
    }));
    if (c->game == GM_GAME_OTHELLO && k > 1) {
        // the promised gen_moves order: squares x outer, y inner (othello_bit_new.py:137-143), where
        // visit() walks the rotated plane's lowest bit first.  The square played is the one bit
        // the occupied plane gains: plane bit A - 1 - (L y + x)  (as gm_expand_host_key, 8x8)
        const DescOthello &o = c->oth;
        auto occ = [&](uint64_t q) { return o.wplane(q) | o.bplane(q); };
        auto rank = [&](uint64_t ch) {
            const int j = o.A - 1 - __builtin_ctz(occ(ch) ^ occ(key));
            return o.L * (j % o.L) + j / o.L;
        };
        for (int i = 1; i < k; i++) {
            const uint64_t ch = kids[i];
            const int r = rank(ch);
            int at = i;
            for (; at > 0 && rank(kids[at - 1]) > r; at--) kids[at] = kids[at - 1];
            kids[at] = ch;
        }
    }
    *prim = p;
    *tier = t;
    *n = k;
    if (k > cap) { set_error("children buffer holds %d, need %d", cap, k); return GM_E_CAP; }
    if (children)
        for (int i = 0; i < k; i++) children[i] = kids[i];
    return GM_OK;
}

int gm_comm_unique_id(void *uid, int bytes) {
    if (!uid || bytes < (int)sizeof(ncclUniqueId)) { set_error("uid buffer must hold %d bytes", (int)sizeof(ncclUniqueId)); return GM_E_ARG; }
    ncclUniqueId id;
    GM_NCCL(ncclGetUniqueId(&id));
    memcpy(uid, &id, sizeof id);
    return GM_OK;
}

int gm_set_comm(gm_ctx *h, int rank, int world, const void *uid, int bytes) {
    if (!h || world < 1 || rank < 0 || rank >= world) { set_error("bad rank/world"); return GM_E_ARG; }
    Ctx *c = &h->c;
    // the sharded engines' transports (per-axis communicators split from c->comm, IPC
    // mappings) belong to the previous communicator: torn down first (dist_box_free
    // synchronises the device and destroys the split communicators), then the parent
    for (const Engine *e : {&dist_box_engine, &dist_sub_engine, &dist_sparse_engine}) e->free_(c);
    if (c->comm) { ncclCommDestroy(c->comm); c->comm = nullptr; }
    c->rank = rank;
    c->world = world;
    c->have_uid = false;
    // no uid: rank and world only; the sharded engines refuse to solve without one (gm_solve)
    if (!uid || bytes <= 0) return GM_OK;
    if (bytes < (int)sizeof(ncclUniqueId)) { set_error("uid must hold %d bytes", (int)sizeof(ncclUniqueId)); return GM_E_ARG; }
    if (c->device < 0) { set_error("no HIP device"); return GM_E_HIP; }
    static_assert(sizeof(ncclUniqueId) <= sizeof(c->uid), "unique id size");
    memcpy(c->uid, uid, sizeof(ncclUniqueId));
    c->have_uid = true;
    return GM_OK;
}

int gm_solve(gm_ctx *h, uint64_t root, uint64_t *n_positions, uint16_t *root_record) {
    if (!h) return GM_E_ARG;
    GM_TRY(refuse_wide(&h->c, "gm_solve"));
    return gm_solve_key(h, &root, n_positions, root_record);
}

// ---------------------------------------------------------------- multi-word keys
int gm_key_words(gm_ctx *h) {
    if (!h) return GM_E_ARG;
    return key_words(&h->c);
}

int gm_pack_initial_key(gm_ctx *h, uint64_t *words) {
    if (!h || !words) return GM_E_ARG;
    if (!h->c.wide) return gm_pack_initial(h, words);
    // othello_bit_new.py:36-55: white (3,3) (4,4), black (3,4) (4,3), turn 2, no pass
    auto bit = [](int x, int y) { return 1ull << (63 - (8 * y + x)); };
    const uint64_t w = bit(3, 3) | bit(4, 4), b = bit(3, 4) | bit(4, 3);
    DescOthello8::to_words(DescOthello8::pack(w, b, 2, 0), words);
    return GM_OK;
}

int gm_expand_host_key(gm_ctx *h, const uint64_t *words, uint64_t *children, int cap, int *n, int *prim,
                       int64_t *tier) {
    if (!h || !words || !n || !prim || !tier) return GM_E_ARG;
    Ctx *c = &h->c;
    if (!c->wide) return gm_expand_host(h, words[0], children, cap, n, prim, tier);
    K128 k;
    if (!DescOthello8::from_words(words, &k)) { set_error("key is not a valid position"); return GM_E_KEY; }
    K128 kids[64];
    const DescOthello8 &d = c->oth8;
    *prim = d.primitive(k);
    *tier = d.tier(k);
    *n = *prim == UNDECIDED ? d.children(k, kids) : 0;
    // the header promises the plugin's gen_moves order: squares x outer, y inner
    // (othello_bit_new.py:163-166), where visit() walks the plane's lowest bit first.  The
    // square played is the one bit the occupied plane gains: plane bit 63 - (8y + x).
    auto rank = [&](const K128 &ch) {
        const uint64_t placed = DescOthello8::occ(ch) ^ DescOthello8::occ(k);
        if (!placed) return 0;   // the pass: a single child
        const int j = 63 - __builtin_ctzll(placed);
        return 8 * (j % 8) + j / 8;
    };
    for (int i = 1; i < *n; i++) {
        const K128 ch = kids[i];
        const int r = rank(ch);
        int at = i;
        for (; at > 0 && rank(kids[at - 1]) > r; at--) kids[at] = kids[at - 1];
        kids[at] = ch;
    }
    if (*n > cap) { set_error("children buffer holds %d, need %d", cap, *n); return GM_E_CAP; }
    if (children)
        for (int i = 0; i < *n; i++) DescOthello8::to_words(kids[i], children + (size_t)key_words(c) * i);
    return GM_OK;
}

int gm_solve_key(gm_ctx *h, const uint64_t *words, uint64_t *n_positions, uint16_t *root_record) {
    if (!h || !words) return GM_E_ARG;
    Ctx *c = &h->c;
    if (c->game == GM_GAME_GRAPH) { set_error("a GM_GAME_GRAPH context is solved with gm_solve_graph"); return GM_E_GAME; }
    GM_TRY(need_device(c));
    Root root;
    GM_TRY(parse_root(c, words, "gm_solve: root key", &root));
    GM_HIP(hipSetDevice(c->device));
    solve_begin(c, c->world, c->timing && !c->wide);
    set_root(c, root);
    // a wide game's engine is the hash-sharded sparse engine: one GPU (G = 1), virtual ranks, or
    // one process per rank
    const bool sharded = c->wide || c->world > 1 || c->virtual_ranks > 1 || c->engine_opt == GM_ENGINE_DIST_SPARSE;
    const Engine *e = choose_engine(c, sharded);
    GM_TRY(solve_comm(c, e, sharded));
    release_other_dense(c, e);
    GM_TRY(e->solve(c, c->root_key()));
    return solve_finish(c, e, !sharded ? 1 : c->world > 1 ? c->world : c->virtual_ranks, n_positions, root_record);
}

int gm_export_key(gm_ctx *h, uint64_t *words, uint16_t *recs, uint64_t cap, uint64_t *n) {
    GM_TRY(need_solved(h));
    if (!n || (words && !recs)) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_HIP(hipSetDevice(c->device));
    // the engine's order is the device keys': a one-word context's are the ABI's
    if (!c->wide) return c->solved_by->export_(c, words, recs, cap, n);
    GM_TRY(c->solved_by->export_(c, nullptr, nullptr, 0, n));
    if (!words) return GM_OK;
    if (cap < *n) { set_error("export buffer too small"); return GM_E_CAP; }
    std::vector<unsigned char> k(*n * key_bytes(c));
    std::vector<uint16_t> r(*n);
    GM_TRY(c->solved_by->export_(c, k.data(), r.data(), *n, n));
    const std::vector<uint64_t> perm = abi_sorted(c, k.data(), *n, words);
    for (uint64_t i = 0; i < *n; i++) recs[i] = r[perm[i]];
    return GM_OK;
}

int gm_query_key(gm_ctx *h, const uint64_t *words, uint16_t *recs, uint64_t n) {
    GM_TRY(need_solved(h));
    if (n && (!words || !recs)) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_HIP(hipSetDevice(c->device));
    DeviceKeys k;
    GM_TRY(device_keys(c, words, n, BadKey::Unsolved, "gm_query_key: key", &k));
    GM_TRY(c->solved_by->query(c, k.p, recs, n));
    for (uint64_t i : k.bad) recs[i] = REC_UNSOLVED;
    return GM_OK;
}

int gm_solve_graph(gm_ctx *h, uint64_t n, const uint8_t *prim, const uint64_t *off, const uint32_t *kid,
                   uint16_t *root_record) {
    if (!h) return GM_E_ARG;
    Ctx *c = &h->c;
    if (c->game != GM_GAME_GRAPH) { set_error("gm_solve_graph needs a GM_GAME_GRAPH context"); return GM_E_GAME; }
    solve_begin(c, 1, false);   // the table the context held is not this graph's
    if (!prim || !off) { set_error("gm_solve_graph needs primitive and child_off"); return GM_E_ARG; }
    GM_TRY(need_device(c));
    if (n >= (1ull << 32)) { set_error("graphs are limited to 2^32 - 1 positions"); return GM_E_ARG; }
    for (uint64_t i = 0; i < n; i++)
        if (off[i + 1] < off[i]) { set_error("child_off is not monotone at %llu", (unsigned long long)i); return GM_E_ARG; }
    if (off[n] && !kid) { set_error("gm_solve_graph needs child_idx"); return GM_E_ARG; }
    GM_HIP(hipSetDevice(c->device));
    GM_TRY(graph_solve(c, n, prim, off, kid));
    return solve_finish(c, &graph_engine, 1, nullptr, root_record);
}

static int need_solved(gm_ctx *h) {
    if (!h) return GM_E_ARG;
    if (!h->c.solved) { set_error("call gm_solve first"); return GM_E_STATE; }
    return GM_OK;
}

int gm_import(gm_ctx *h, const uint64_t *root_words, const uint64_t *key_words, const uint16_t *records, uint64_t n,
              uint64_t *n_positions, uint16_t *root_record) {
    if (!h) return GM_E_ARG;
    Ctx *c = &h->c;
    solve_begin(c, 1, false);   // a refusal leaves the context without a table, as a failed solve does
    if (!root_words || !key_words || !records) { set_error("gm_import: root_words, key_words or records is NULL"); return GM_E_ARG; }
    if (!n) { set_error("gm_import: n is 0"); return GM_E_ARG; }
    if (c->game == GM_GAME_GRAPH) {
        set_error("gm_import: the keys of a GM_GAME_GRAPH table are the host walk's numbering, which a table does not carry");
        return GM_E_GAME;
    }
    GM_TRY(need_device(c));
    if (c->world > 1 || c->virtual_ranks > 1) {
        set_error("gm_import builds the whole table in one context: not for rank %d of %d processes or %d virtual ranks",
                  c->rank, c->world, c->virtual_ranks);
        return GM_E_ARG;
    }
    if (!c->wide && c->engine_opt == GM_ENGINE_DIST_SPARSE) {
        set_error("gm_import: GM_ENGINE_DIST_SPARSE on a one-word context; the one-GPU engines import its tables");
        return GM_E_ARG;
    }
    const Engine *e = choose_engine(c, false);
    if (e == &dense_box_engine) {
        set_error("gm_import: the box engine's tables are not imported; set GM_OPT_SUB_INTERLEAVE 10 for the block engine");
        return GM_E_GAME;
    }
    if (!e->import_) { set_error("gm_import: this engine's tables are not imported"); return GM_E_GAME; }
    Root root;
    GM_TRY(parse_root(c, root_words, "gm_import: root key", &root));
    GM_HIP(hipSetDevice(c->device));
    set_root(c, root);
    release_other_dense(c, e);
    DeviceKeys keys;
    GM_TRY(device_keys(c, key_words, n, BadKey::Fails, "gm_import: key", &keys));
    const double t0 = now_ms();
    const int rc = e->import_(c, keys.p, records, n);
    if (rc != GM_OK) {
        e->free_(c);
        return rc;
    }
    c->stats.solve_ms = now_ms() - t0;
    // the stored record of the root, 0xFFFF when the table does not hold it (gm_verify: root_ok = 0)
    // (read as every other read is, through solved_by: the byte-table readers take their view from it)
    uint16_t rr = REC_UNSOLVED;
    c->solved_by = e;
    const int rq = e->query(c, c->root_key(), &rr, 1);
    if (rq != GM_OK) {
        c->solved_by = nullptr;
        e->free_(c);
        return rq;
    }
    c->root_record = rr;
    return solve_finish(c, e, 1, n_positions, root_record);
}

int gm_export(gm_ctx *h, uint64_t *keys, uint16_t *recs, uint64_t cap, uint64_t *n) {
    GM_TRY(need_solved(h));
    GM_TRY(refuse_wide(&h->c, "gm_export"));
    return gm_export_key(h, keys, recs, cap, n);
}

int gm_query(gm_ctx *h, const uint64_t *keys, uint16_t *recs, uint64_t n) {
    GM_TRY(need_solved(h));
    GM_TRY(refuse_wide(&h->c, "gm_query"));
    return gm_query_key(h, keys, recs, n);
}

int gm_digest(gm_ctx *h, uint64_t *digest, uint64_t *n) {
    GM_TRY(need_solved(h));
    if (!digest || !n) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_HIP(hipSetDevice(c->device));
    return c->solved_by->digest(c, digest, n);
}

int gm_histogram(gm_ctx *h, uint64_t *counts, int cap, int *n_rem, uint64_t *n) {
    GM_TRY(need_solved(h));
    if (!n_rem || !n || (counts && cap < 0)) return GM_E_ARG;
    Ctx *c = &h->c;
    GM_HIP(hipSetDevice(c->device));
    Hist H;
    if (counts && c->hist_is_kept) {
        // the census of the counts == NULL query just before: one pass over the table per pair
        for (int v = 0; v < 3; v++) H.v[v].swap(c->hist_kept[v]);
        H.other = c->hist_kept_other;
    } else {
        GM_TRY(c->solved_by->histogram(c, &H));
    }
    c->hist_is_kept = false;
    const int nr = (int)H.n_rem();
    *n_rem = nr;
    *n = H.total();
    if (!counts) {
        for (int v = 0; v < 3; v++) c->hist_kept[v].swap(H.v[v]);
        c->hist_kept_other = H.other;
        c->hist_is_kept = true;
        return GM_OK;
    }
    if (cap < nr) { set_error("histogram buffer holds %d remoteness columns, need %d", cap, nr); return GM_E_CAP; }
    for (int v = 0; v < 3; v++)
        for (int r = 0; r < cap; r++) counts[(size_t)v * cap + r] = (size_t)r < H.v[v].size() ? H.v[v][r] : 0;
    return GM_OK;
}

// a rank of a multi-process solve holds its share of the table only
static int need_whole_table(Ctx *c, const char *what) {
    if (c->world > 1) {
        set_error("%s needs the whole table in one context: this is rank %d of a %d-process solve, which does not hold "
                  "the tables of its children's owners (virtual ranks are supported)", what, c->rank, c->world);
        return GM_E_STATE;
    }
    return GM_OK;
}

int gm_verify(gm_ctx *h, gm_verify_t *out, uint64_t *bad_key_words, uint64_t cap, uint64_t *n_bad) {
    GM_TRY(need_solved(h));
    if (!out) { set_error("out is NULL"); return GM_E_ARG; }
    Ctx *c = &h->c;
    GM_TRY(need_whole_table(c, "gm_verify"));
    GM_HIP(hipSetDevice(c->device));
    const uint64_t want = bad_key_words ? cap : 0;
    gm_verify_t r{};
    std::vector<unsigned char> raw;
    uint64_t nb = 0;
    // the list holds VF_FIRST_CAP keys at first; a table with more offenders, when the caller
    // has room for them, is checked again into a list of the right size
    for (uint64_t dev_cap = std::min(want, VF_FIRST_CAP);;) {
        VerifyRun run;
        GM_TRY(verify_begin(c, dev_cap, key_bytes(c), &run));
        const int rc = c->solved_by->verify(c, run.dev);
        const int rc2 = verify_end(c, &run, &r, &raw);
        if (rc != GM_OK) return rc;
        if (rc2 != GM_OK) return rc2;
        nb = r.bad_key + r.misplaced + r.bad_primitive + r.missing_child + r.bad_value;
        if (nb <= dev_cap || dev_cap >= want) break;
        dev_cap = std::min(want, nb);
    }
    // the root: stored, with the record the solve returned
    uint16_t rr = REC_UNSOLVED;
    GM_TRY(c->solved_by->query(c, c->root_key(), &rr, 1));
    r.root_ok = rr != REC_UNSOLVED && rr == c->root_record;
    *out = r;
    if (n_bad) *n_bad = nb;
    if (!want) return GM_OK;
    abi_sorted(c, raw.data(), raw.size() / key_bytes(c), bad_key_words);
    return GM_OK;
}

int gm_select(gm_ctx *h, const gm_select_t *what, uint64_t *key_words, uint16_t *records, uint64_t cap, uint64_t *n) {
    if (!h || !what || !n) { set_error("gm_select: a NULL argument"); return GM_E_ARG; }
    if (!what->values || (what->values & ~15u)) { set_error("gm_select: values is not an OR of GM_SEL_*"); return GM_E_ARG; }
    if (what->rem_lo > what->rem_hi) { set_error("gm_select: rem_lo exceeds rem_hi"); return GM_E_ARG; }
    if (what->reserved) { set_error("gm_select: reserved is not 0"); return GM_E_ARG; }
    GM_TRY(need_solved(h));
    Ctx *c = &h->c;
    if (!c->solved_by->select) { set_error("gm_select: this engine's tables are not selected from"); return GM_E_STATE; }
    GM_HIP(hipSetDevice(c->device));
    const uint64_t want = key_words ? cap : 0;
    std::vector<unsigned char> raw;
    std::vector<uint16_t> rr;
    uint64_t found = 0;
    // the list holds SEL_FIRST_CAP pairs at first; when more match and the caller has room for
    // them, the table is read again into a list of exactly that room
    for (uint64_t dev_cap = std::min(want, SEL_FIRST_CAP);;) {
        SelectRun run;
        GM_TRY(select_begin(c, *what, dev_cap, key_bytes(c), &run));
        const int rc = c->solved_by->select(c, run.dev);
        const int rc2 = select_end(c, &run, &found, &raw, &rr);
        if (rc != GM_OK) return rc;
        if (rc2 != GM_OK) return rc2;
        if (std::min(found, want) <= dev_cap) break;
        dev_cap = std::min(found, want);
    }
    *n = found;
    if (!want) return GM_OK;
    const std::vector<uint64_t> perm = abi_sorted(c, raw.data(), rr.size(), key_words);
    if (records)
        for (size_t i = 0; i < perm.size(); i++) records[i] = rr[perm[i]];
    return GM_OK;
}

int gm_moves(gm_ctx *h, const uint64_t *key_words, uint64_t n, gm_moves_t *heads, uint64_t *child_words,
             uint16_t *child_records, uint64_t cap, uint64_t *n_children) {
    if (!h || !n_children) { set_error("gm_moves: ctx or n_children is NULL"); return GM_E_ARG; }
    if (n && (!key_words || !heads)) { set_error("gm_moves: key_words or heads is NULL"); return GM_E_ARG; }
    GM_TRY(need_solved(h));
    Ctx *c = &h->c;
    GM_TRY(need_whole_table(c, "gm_moves"));
    if (!c->solved_by->moves) { set_error("gm_moves: this engine's tables do not answer moves"); return GM_E_STATE; }
    *n_children = 0;
    if (!n) return GM_OK;
    GM_HIP(hipSetDevice(c->device));
    DeviceKeys k;   // words that are no position: record 0xFFFF, no children
    GM_TRY(device_keys(c, key_words, n, BadKey::Skipped, "gm_moves: key", &k));
    const MovesReq r{k.p, key_bytes(c), gm::key_words(c), n, heads, child_words, child_records, cap, n_children};
    return c->solved_by->moves(c, r);
}

int gm_reach(gm_ctx *h, const gm_reach_t *how, const uint64_t *start_words, uint64_t n_starts, gm_reach_out_t *out,
             uint64_t *ply_counts, int ply_cap, uint64_t *key_words, uint16_t *records, uint8_t *sides, uint64_t cap) {
    if (!h || !how || !out) { set_error("gm_reach: ctx, how or out is NULL"); return GM_E_ARG; }
    if (how->mover > GM_REACH_FIRST || how->other > GM_REACH_FIRST) { set_error("gm_reach: a policy is not a GM_REACH_*"); return GM_E_ARG; }
    if (how->reserved) { set_error("gm_reach: reserved is not 0"); return GM_E_ARG; }
    if (n_starts && !start_words) { set_error("gm_reach: start_words is NULL"); return GM_E_ARG; }
    GM_TRY(need_solved(h));
    Ctx *c = &h->c;
    GM_TRY(need_whole_table(c, "gm_reach"));
    if (!c->solved_by->reach) { set_error("gm_reach: this engine's tables are not walked"); return GM_E_STATE; }
    *out = gm_reach_out_t{};
    std::vector<uint64_t> pc;
    std::vector<unsigned char> raw;
    std::vector<uint16_t> rr;
    std::vector<uint8_t> ss;
    if (n_starts) {
        GM_HIP(hipSetDevice(c->device));
        DeviceKeys k;
        GM_TRY(device_keys(c, start_words, n_starts, BadKey::Skipped, "gm_reach: start", &k));
        const ReachReq q{*how, k.p, key_bytes(c), n_starts, key_words ? cap : 0, out, &pc, &raw, &rr, &ss};
        GM_TRY(c->solved_by->reach(c, q));
    }
    if (ply_counts && ply_cap > 0) {
        if ((size_t)ply_cap < pc.size()) {
            set_error("gm_reach: ply_counts holds %d plies, need %d", ply_cap, out->plies);
            return GM_E_CAP;
        }
        for (int d = 0; d < ply_cap; d++) ply_counts[d] = (size_t)d < pc.size() ? pc[d] : 0;
    }
    if (rr.empty()) return GM_OK;
    const std::vector<uint64_t> perm = abi_sorted(c, raw.data(), rr.size(), key_words);
    for (size_t i = 0; i < perm.size(); i++) {
        if (records) records[i] = rr[perm[i]];
        if (sides) sides[i] = ss[perm[i]];
    }
    return GM_OK;
}

int gm_poke(gm_ctx *h, const uint64_t *key_words, uint16_t record) {
    GM_TRY(need_solved(h));
    if (!key_words) { set_error("key_words is NULL"); return GM_E_ARG; }
    Ctx *c = &h->c;
    // (DRAW, 0) is a record of the graph engine's loopy tables only (graph_poke refuses it on the others)
    const bool draw = record == 0xC000 && c->solved_by == &graph_engine;
    if (record != REC_UNSOLVED && (record >> 14) > TIE && !draw) { set_error("gm_poke: not a record"); return GM_E_ARG; }
    GM_TRY(need_whole_table(c, "gm_poke"));
    GM_HIP(hipSetDevice(c->device));
    c->hist_is_kept = false;
    DeviceKeys k;
    GM_TRY(device_keys(c, key_words, 1, BadKey::Fails, "gm_poke: key", &k));
    return c->solved_by->poke(c, k.p, record);
}

int gm_draw_count(gm_ctx *h, uint64_t *n_draw) {
    GM_TRY(need_solved(h));
    if (!n_draw) { set_error("n_draw is NULL"); return GM_E_ARG; }
    *n_draw = h->c.n_draw;
    return GM_OK;
}

int gm_stats(gm_ctx *h, gm_stats_t *out) {
    if (!h || !out) return GM_E_ARG;
    *out = h->c.stats;
    return GM_OK;
}

int gm_tier_counts(gm_ctx *h, uint64_t *counts, int cap, int *n) {
    GM_TRY(need_solved(h));
    if (!n) return GM_E_ARG;
    Ctx *c = &h->c;
    *n = (int)c->tier_counts.size();
    if (!counts) return GM_OK;
    if (cap < *n) { set_error("tier buffer too small"); return GM_E_CAP; }
    for (int i = 0; i < *n; i++) counts[i] = c->tier_counts[i];
    return GM_OK;
}

int gm_adopt_buffer(gm_ctx *h, int role, void *p, uint64_t bytes) {
    if (!h || !p) return GM_E_ARG;
    if (role != GM_BUF_DENSE_TABLE) { set_error("unknown buffer role %d", role); return GM_E_ARG; }
    h->c.adopted_dense = p;
    h->c.adopted_dense_bytes = bytes;
    return GM_OK;
}

int gm_dense_table(gm_ctx *h, void **p, uint64_t *bytes) {
    GM_TRY(need_solved(h));
    if (!p || !bytes) return GM_E_ARG;
    if (!h->c.solved_by->table) {
        set_error("only the SUBTRACT dense path has a dense table");
        return GM_E_STATE;
    }
    return h->c.solved_by->table(&h->c, p, bytes);
}

int gm_dist_plan(int heaps, int world, int rank, const int32_t *opts, int what, int axis, uint32_t *off,
                 uint64_t off_cap, uint64_t *n_off, uint32_t *data, uint64_t data_cap, uint64_t *n_data) {
    return dist_sub_plan(heaps, world, rank, opts, what, axis, off, off_cap, n_off, data, data_cap, n_data);
}

int gm_box_plan(uint64_t root, int world, int rank, const int32_t *opts, int what, int axis, uint32_t *out,
                uint64_t cap, uint64_t *n) {
    if (!n) return GM_E_ARG;
    return dist_box_plan(root, world, rank, opts, what, axis, out, cap, n);
}

int gm_sparse_layout(int world, int steps, const uint64_t *counts, int rank, uint64_t *seg, uint64_t *send_off,
                     uint64_t *recv_off, uint64_t *recv_seg) {
    return dist_sparse_layout(world, steps, counts, rank, seg, send_off, recv_off, recv_seg);
}

int gm_rank_stats(gm_ctx *h, double *kernel_ms, uint64_t *boxes, uint64_t *recv_bytes, int cap, int *n) {
    GM_TRY(need_solved(h));
    if (!n) return GM_E_ARG;
    Ctx *c = &h->c;
    if (c->solved_by != &dist_box_engine) { *n = 0; return GM_OK; }   // ranks: the split box engine's
    return dist_box_rank_stats(c, kernel_ms, boxes, recv_bytes, cap, n);
}

int gm_rank_op_ms(gm_ctx *h, int rank, double *ms, int cap, int *n) {
    GM_TRY(need_solved(h));
    if (!n) return GM_E_ARG;
    Ctx *c = &h->c;
    if (c->solved_by != &dist_box_engine) { *n = 0; return GM_OK; }   // ranks: the split box engine's
    return dist_box_op_ms(c, rank, ms, cap, n);
}

void gm_close(gm_ctx *h) {
    if (!h) return;
    Ctx *c = &h->c;
    if (c->device >= 0) hipSetDevice(c->device);
    free_engines(c);
    if (c->device >= 0) (void)hipDeviceSynchronize();
    for (auto &b : c->buf_cache) (void)hipFree(b.first);
    for (auto &b : c->buf_live) (void)hipFree(b.first);
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    if (c->comm_stream) hipStreamDestroy(c->comm_stream);
    delete h;
}

}  // extern "C"
