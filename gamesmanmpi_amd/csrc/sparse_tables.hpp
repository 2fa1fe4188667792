// sparse_tables.hpp -- per-tier tables and the kernels shared by the single-GPU
// sparse engine (sparse.hip) and its hash-sharded twin (dist_sparse.hip).
//
//   tier table     16-byte slots {u64 key, u64 score}, linear probing from
//                  home = mixed key * cap >> 64 (any capacity, no power-of-two
//                  rounding).  Sized for load <= 0.7 from the edges into the
//                  tier times a predicted distinct fraction (sparse.hip); an
//                  insert that probes past MAX_PROBE slots flags the table full
//                  and the insert pass is re-run into a larger table (inserts are
//                  idempotent).  The tiers above atomicCAS-insert their
//                  children's keys (deduplication); classify_kernel then streams
//                  it once, scoring every position in place; retrograde lookups
//                  read key and score with one 16-byte load.
//   interior list  dense (key, slot) of the tier's undecided positions.
// These replace the reference's CacheDict tables (src/cache_dict.py:7-82) and
// the per-edge LOOK_UP / primitive test of Process.lookup (src/new_process.py:102-133).
#pragma once
#include "sparse_common.hpp"
#include "verify_common.hpp"
#include "moves_common.hpp"
#include "reach_common.hpp"
#include "select_common.hpp"

namespace gm {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct alignas(16) RSlot {
    uint64_t key;
    uint64_t score;   // u16 preference score in the low bits
};

// loc: the table's home function (home_slot): 0 = a hash of the whole key; else
// gshift | wlog << 8 = the key's group (key >> gshift) picks a base slot and a hash of the
// key one of the 2^wlog slots from it (GM_SPARSE_HOME_W, sparse.hip)
struct FrontRef {           // inserting into a tier table
    RSlot *s;
    uint64_t cap;
    unsigned long long *count;
    uint32_t loc = 0;
};
struct ResRef {             // looking up in a tier table
    RSlot *s;
    uint64_t cap;
    uint32_t loc = 0;
};
// the home function a table of `cap` slots uses: a locality home only when the table
// holds at least two windows (the same rule for inserts, lookups and rehashes)
inline GM_HD uint32_t eff_loc(uint32_t loc, uint64_t cap) {
    return (loc >> 8) && cap >= (2ull << (loc >> 8)) ? loc : 0u;
}

// 128-bit keys (gm_common.hpp K128): 32-byte slots.  An insert claims a slot by atomicCAS of
// hi from EMPTY_HI to the key's hi without its publish bit, stores lo, then publishes hi
// (coherent stores, ordered by a wait: front_insert below); a probe that meets a claimed but
// unpublished slot with its own hi re-reads that slot (the claiming lane publishes in the same iteration of the probe loop, so lanes of
// one wave never wait on each other across iterations).  Lookups run after the tier is
// complete and read (hi, lo) with one 16-byte load.
struct alignas(32) WSlot {
    uint64_t hi, lo;
    uint64_t score;   // u16 preference score in the low bits
    uint64_t pad;
};
struct WFrontRef {
    WSlot *s;
    uint64_t cap;
    unsigned long long *count;
    uint32_t loc = 0;
};
struct WResRef {
    WSlot *s;
    uint64_t cap;
    uint32_t loc = 0;
};

// the table types of a key type
template <class K>
struct KT;
template <>
struct KT<uint64_t> {
    using Slot = RSlot;
    using Front = FrontRef;
    using Res = ResRef;
};
template <>
struct KT<K128> {
    using Slot = WSlot;
    using Front = WFrontRef;
    using Res = WResRef;
};

constexpr uint64_t MAX_PROBE = 2048;   // an insert probing further marks the table full
constexpr double TABLE_LOAD = 0.7;     // planned load of a tier table
template <int S>
struct Fronts {
    FrontRef t[S];
};
template <int S>
struct Ress {
    ResRef t[S];
};

template <class K>
struct SpTierT {
    typename KT<K>::Slot *slots = nullptr;
    uint64_t cap = 0;
    uint64_t fcount = 0;         // keys inserted so far (host mirror of the device counter)
    uint64_t count = 0;          // positions of the tier once classified (stored representatives)
    uint64_t count_all = 0;      // positions they stand for (orbits expanded, games.hpp NoSym)
    K *ikeys = nullptr;          // interior (undecided) positions and their slots
    uint32_t *islot = nullptr;
    uint8_t *iwon = nullptr;     // per interior position: 1 = has a LOSS-in-0 child (set by expand)
    uint64_t ni = 0;
    // single-GPU engine, large tiers: the interior list sorted by the key's top bits
    // (sparse.hip, batch kernels); expand, retro and iwon then follow this order
    K *skeys = nullptr;
    uint32_t *sslot = nullptr;
    int64_t tier = 0;            // the descriptor tier of the positions (root tier + index)
    uint32_t loc = 0;            // home function (FrontRef::loc) requested for this tier's table
    // GM_SPARSE_CSR (sparse.hip, one-step games on the plain kernels): per interior position
    // in the order expand / retro walk it, its undecided children's slots in the next tier's
    // table (cslot[coff .. coff + ccnt)) and the best score of its primitive children
    uint32_t *coff = nullptr, *cslot = nullptr;
    uint8_t *ccnt = nullptr;
    uint16_t *pbest = nullptr;
};
using SpTier = SpTierT<uint64_t>;

namespace {

// home slot: the low half of mix64 scaled to cap (the high half picks the owner
// rank in the sharded engine, so the two stay independent).  With a locality home
// (loc != 0) the keys of one group -- one value of the key's top bits, which the sorted
// interior lists walk together -- share a window of 2^wlog slots at a hashed base.
__device__ __forceinline__ uint64_t home_slot(uint64_t key, uint64_t cap, uint32_t loc) {
    const uint64_t m = mix64(key);
    if (!loc) return __umul64hi((m << 32) | (m >> 32), cap);
    const uint64_t g = mix64((key >> (loc & 63u)) ^ 0x5851F42D4C957F2Dull);
    const uint64_t h = __umul64hi(g, cap) + (m & ((1ull << (loc >> 8)) - 1ull));
    return h >= cap ? h - cap : h;
}

__device__ __forceinline__ bool front_insert(const FrontRef &t, uint64_t key, uint32_t *err) {
    uint64_t h = home_slot(key, t.cap, t.loc);
    const uint64_t lim = t.cap < MAX_PROBE ? t.cap : MAX_PROBE;
    for (uint64_t probe = 0; probe < lim; probe++) {
        const uint64_t cur = t.s[h].key;
        if (cur == key) return false;
        if (cur == EMPTY_KEY) {
            const unsigned long long prev = atomicCAS((unsigned long long *)&t.s[h].key,
                                                      (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (prev == EMPTY_KEY) return true;
            if (prev == key) return false;
        }
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    atomicOr(err, DEV_ERR_TABLE_FULL);
    return false;
}

// as front_insert, and the key's slot (new or found) in *slot (~0u when the table is full)
__device__ __forceinline__ bool front_insert_slot(const FrontRef &t, uint64_t key, uint32_t *err, uint32_t *slot) {
    uint64_t h = home_slot(key, t.cap, t.loc);
    const uint64_t lim = t.cap < MAX_PROBE ? t.cap : MAX_PROBE;
    for (uint64_t probe = 0; probe < lim; probe++) {
        const uint64_t cur = t.s[h].key;
        if (cur == key) { *slot = (uint32_t)h; return false; }
        if (cur == EMPTY_KEY) {
            const unsigned long long prev = atomicCAS((unsigned long long *)&t.s[h].key,
                                                      (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (prev == EMPTY_KEY || prev == key) { *slot = (uint32_t)h; return prev == EMPTY_KEY; }
        }
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    atomicOr(err, DEV_ERR_TABLE_FULL);
    *slot = ~0u;
    return false;
}

// score of key, or -1 when absent; each probe is one 16-byte load
__device__ __forceinline__ int res_find(const ResRef &t, uint64_t key) {
    if (!t.s) return -1;
    uint64_t h = home_slot(key, t.cap, t.loc);
    for (uint64_t probe = 0; probe < t.cap; probe++) {
        const u64x2 v = *(const u64x2 *)&t.s[h];
        if (v[0] == key) return (int)(v[1] & 0xFFFFu);
        if (v[0] == EMPTY_KEY) return -1;
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    return -1;
}

__device__ __forceinline__ uint64_t home_slot(const K128 &key, uint64_t cap, uint32_t) {
    const uint64_t m = mix_key(key);
    return __umul64hi((m << 32) | (m >> 32), cap);
}

__device__ __forceinline__ bool front_insert(const WFrontRef &t, const K128 &key, uint32_t *err) {
    // No acquire / release here: on this chip an agent-scope acquire invalidates the XCD's L2
    // (buffer_inv sc1) and a release writes it back (buffer_wbl2 sc1) -- per probe, that made
    // the 8x8 forward pass ~10x slower.  Instead lo is stored with a coherent (sc1) atomic
    // store that the wave waits for before it publishes hi with another; a reader that sees
    // the published hi reads lo with a coherent load.  The first read of a slot is a plain
    // load: a stale view can only show the slot emptier than it is (EMPTY for claimed, claimed
    // for published -- the CAS, or a coherent re-read, settles it), never another key.
    const uint64_t claim = key.hi & ~K128_PUB;
    uint64_t h = home_slot(key, t.cap, t.loc);
    const uint64_t lim = t.cap < MAX_PROBE ? t.cap : MAX_PROBE;
    uint32_t spins = 0;
    bool coherent = false;   // this slot was seen claimed but unpublished: re-read it coherently
    for (uint64_t probe = 0; probe < lim;) {
        uint64_t cur = coherent ? __hip_atomic_load(&t.s[h].hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : t.s[h].hi;
        if (cur == EMPTY_HI) {
            const unsigned long long prev =
                atomicCAS((unsigned long long *)&t.s[h].hi, (unsigned long long)EMPTY_HI, (unsigned long long)claim);
            if (prev == EMPTY_HI) {
                __hip_atomic_store(&t.s[h].lo, key.lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // lo has reached the coherent level
                __hip_atomic_store(&t.s[h].hi, key.hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return true;
            }
            cur = prev;
        }
        if ((cur | K128_PUB) == key.hi) {
            if (!(cur & K128_PUB)) {   // claimed with this hi, lo not published yet: read the slot again
                if (++spins > (1u << 24)) {
                    atomicOr(err, DEV_ERR_TABLE_FULL);
                    return false;
                }
                coherent = true;
                continue;
            }
            if (__hip_atomic_load(&t.s[h].lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == key.lo) return false;
        }
        coherent = false;
        h = h + 1 == t.cap ? 0 : h + 1;
        probe++;
    }
    atomicOr(err, DEV_ERR_TABLE_FULL);
    return false;
}

__device__ __forceinline__ int res_find(const WResRef &t, const K128 &key) {
    if (!t.s) return -1;
    uint64_t h = home_slot(key, t.cap, t.loc);
    for (uint64_t probe = 0; probe < t.cap; probe++) {
        const u64x2 v = *(const u64x2 *)&t.s[h];
        if (v[0] == key.hi && v[1] == key.lo) return (int)(t.s[h].score & 0xFFFFu);
        if (v[0] == EMPTY_HI) return -1;
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    return -1;
}

// the slot a lookup of key ends at, or -1 when absent (gm_verify, gm_poke)
__device__ __forceinline__ int64_t res_find_slot(const ResRef &t, uint64_t key) {
    if (!t.s) return -1;
    uint64_t h = home_slot(key, t.cap, t.loc);
    for (uint64_t probe = 0; probe < t.cap; probe++) {
        const uint64_t cur = t.s[h].key;
        if (cur == key) return (int64_t)h;
        if (cur == EMPTY_KEY) return -1;
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    return -1;
}
__device__ __forceinline__ int64_t res_find_slot(const WResRef &t, const K128 &key) {
    if (!t.s) return -1;
    uint64_t h = home_slot(key, t.cap, t.loc);
    for (uint64_t probe = 0; probe < t.cap; probe++) {
        const u64x2 v = *(const u64x2 *)&t.s[h];
        if (v[0] == key.hi && v[1] == key.lo) return (int64_t)h;
        if (v[0] == EMPTY_HI) return -1;
        h = h + 1 == t.cap ? 0 : h + 1;
    }
    return -1;
}

// slot access shared by the two slot types
__device__ __forceinline__ void slot_clear_key(uint64_t &k) { k = EMPTY_KEY; }
__device__ __forceinline__ void slot_clear_key(K128 &k) { k = K128{0, EMPTY_HI}; }
__device__ __forceinline__ uint64_t slot_key(const RSlot &s) { return s.key; }
__device__ __forceinline__ K128 slot_key(const WSlot &s) {
    const u64x2 v = *(const u64x2 *)&s;
    return K128{v[1], v[0]};
}
__device__ __forceinline__ uint64_t slot_score(const RSlot &s) { return s.score; }
__device__ __forceinline__ uint64_t slot_score(const WSlot &s) { return s.score; }
__device__ __forceinline__ void slot_set(RSlot &s, uint64_t k, uint64_t score) { *(u64x2 *)&s = u64x2{k, score}; }
__device__ __forceinline__ void slot_set(WSlot &s, const K128 &, uint64_t score) { s.score = score; }
__device__ __forceinline__ void slot_clear(RSlot &s) { *(u64x2 *)&s = u64x2{EMPTY_KEY, 0}; }
__device__ __forceinline__ void slot_clear(WSlot &s) {
    *(u64x2 *)&s = u64x2{EMPTY_HI, 0};
    *((u64x2 *)&s + 1) = u64x2{0, 0};
}

template <class Slot>
__global__ void slot_fill_kernel(Slot *s, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        slot_clear(s[i]);
}

// every table of a replay in one launch: blockIdx.y = table, x strides inside it
__global__ void slot_fill_many_kernel(const ResRef *__restrict__ t) {
    const ResRef r = t[blockIdx.y];
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < r.cap; i += (uint64_t)gridDim.x * blockDim.x)
        *(u64x2 *)&r.s[i] = u64x2{EMPTY_KEY, 0};
}

template <class K>
__global__ void front_rehash_kernel(const typename KT<K>::Slot *__restrict__ old, uint64_t ocap,
                                    typename KT<K>::Front dst, uint32_t *err) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < ocap;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const K k = slot_key(old[i]);
        if (!key_empty(k)) front_insert(dst, k, err);
    }
}

// the record of one key of a resolved table (0 = not found) -> *out
__global__ void res_lookup_one_kernel(ResRef t, uint64_t key, unsigned long long *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int s = res_find(t, key);
        *out = s < 0 ? 0ull : (unsigned long long)record_of_score((uint16_t)s) | (1ull << 32);
    }
}

__global__ void front_insert_one_kernel(FrontRef t, uint64_t key, uint32_t *err) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && front_insert(t, key, err)) atomicAdd(t.count, 1ull);
}
__global__ void front_insert_one_wkernel(WFrontRef t, K128 key, uint32_t *err) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && front_insert(t, key, err)) atomicAdd(t.count, 1ull);
}

// One streaming pass over a finished tier table: primitive() once per position,
// its score stored in place (whole 16-B slots, coalesced), the undecided ones
// appended to the interior list with their edge counts per tier step.  A
// workgroup takes CROWS rows of 256 slots and reserves its part of the interior
// list with ONE atomic (a per-wave atomic on one counter serialises at ~90 per
// microsecond).  seen = positions found (a check against the insert count);
// seen[1] = the positions they stand for (each representative's orbit, games.hpp).
// Tables below CLASSIFY_ROWS_MIN slots take one row per workgroup: with CROWS rows a
// small tier ran on one or two workgroups whose threads each walked 16 positions in
// turn (Othello 4x4: classify 0.1-0.4 ms per tier, most of the solve).
constexpr int CROWS = 16;
constexpr uint64_t CLASSIFY_ROWS_MIN = 1ull << 22;
template <class D, int ROWS, bool COUNT = true, bool EDGES = COUNT>
__global__ __launch_bounds__(256) void classify_kernel(D d, typename KT<key_t<D>>::Slot *__restrict__ slots, uint64_t cap,
                                                       key_t<D> *__restrict__ ikeys, uint32_t *__restrict__ islot,
                                                       unsigned long long *icount, unsigned long long *edges,
                                                       unsigned long long *seen, uint32_t *err) {
    constexpr int S = D::MAX_SKIP;
    __shared__ uint32_t woff[ROWS * 4];
    __shared__ unsigned long long sbase;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t cnt[S];
#pragma unroll
    for (int s = 0; s < S; s++) cnt[s] = 0;
    uint64_t nseen = 0, nall = 0;
    for (uint64_t chunk = blockIdx.x * (256ull * ROWS); chunk < cap; chunk += (uint64_t)gridDim.x * 256ull * ROWS) {
        using K = key_t<D>;
        K k[ROWS];
        uint64_t m[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            const uint64_t i = chunk + 256ull * r + threadIdx.x;
            if (i < cap) k[r] = slot_key(slots[i]);
            else slot_clear_key(k[r]);
        }
#pragma unroll
        for (int r = 0; r < ROWS; r++) {
            bool interior = false;
            if (!key_empty(k[r])) {
                nseen++;
                if (COUNT) d.orbit(k[r], [&](const K &) { nall++; });   // a replay knows its orbit counts
                const uint64_t i = chunk + 256ull * r + threadIdx.x;
                const int p = d.primitive(k[r]);
                if (p == DRAW) atomicOr(err, DEV_ERR_DRAW);
                interior = p == UNDECIDED;
                if (!interior) {
                    slot_set(slots[i], k[r], (uint64_t)score_of_primitive(p));
                } else if (EDGES) {   // a replay knows its sizes, the sharded path counts bins: no edge counts
                    if constexpr (step_count_t<D>::value) {
                        int dt = 0;
                        const int nk = d.count_children(k[r], &dt);
                        if (dt < 1 || dt > S) atomicOr(err, DEV_ERR_TIER);
#pragma unroll
                        for (int s = 0; s < S; s++) cnt[s] += dt == s + 1 ? (uint64_t)nk : 0ull;
                    } else {
                        const int64_t tk = d.tier(k[r]);
                        int nk = 0;
                        unreduced(d).visit(k[r], [&](const K &c) {   // tiers only: no canonical children
                            const int64_t dt = d.tier(c) - tk;
                            nk++;
                            if (dt < 1 || dt > S) atomicOr(err, DEV_ERR_TIER);
#pragma unroll
                            for (int s = 0; s < S; s++) cnt[s] += dt == s + 1;
                            return true;
                        });
                        if (!nk) atomicOr(err, DEV_ERR_NOMOVES);
                    }
                }
            }
            m[r] = __ballot(interior);
            if (lane == 0) woff[r * 4 + w] = (uint32_t)__popcll(m[r]);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (int j = 0; j < ROWS * 4; j++) {
                const uint32_t c = woff[j];
                woff[j] = acc;
                acc += c;
            }
            sbase = acc ? atomicAdd(icount, (unsigned long long)acc) : 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < ROWS; r++)
            if ((m[r] >> lane) & 1ull) {
                const uint64_t at = sbase + woff[r * 4 + w] + __popcll(m[r] & below);
                ikeys[at] = k[r];
                islot[at] = (uint32_t)(chunk + 256ull * r + threadIdx.x);
            }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < S; s++) block_add(edges + s, cnt[s]);
    block_add(seen, nseen);
    block_add(seen + 1, nall);
}

template <class D>
__global__ void query_kernel(D d, int64_t t_root, const typename KT<key_t<D>>::Res *tabs, int ntabs,
                             const key_t<D> *__restrict__ keys, uint16_t *__restrict__ out, uint64_t n) {
    uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const key_t<D> k = keys[i];
    int64_t t = d.valid(k) ? d.tier(k) - t_root : -1;
    uint16_t r = REC_UNSOLVED;
    if (t >= 0 && t < ntabs) {
        int s = res_find(tabs[t], d.canon(k));
        if (s >= 0) r = record_of_score((uint16_t)s);
    }
    out[i] = r;
}

// digest and export expand every stored representative's orbit (games.hpp)
template <class D>
__global__ void res_digest_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ s, uint64_t cap,
                                  unsigned long long *acc) {
    using K = key_t<D>;
    uint64_t sum = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const K key = slot_key(s[i]);
        if (!key_empty(key)) {
            const uint16_t rec = record_of_score((uint16_t)slot_score(s[i]));
            d.orbit(key, [&](const K &k) { sum += digest_term(k, rec); });
        }
    }
    block_add(acc, sum);
}

// census of a tier table: every stored representative counts once per member of its orbit
template <class D>
__global__ void res_hist_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ s, uint64_t cap,
                                unsigned long long *bins, uint32_t nbin, int use_lds) {
    using K = key_t<D>;
    uint32_t *lds = score_bins_open(nbin, use_lds);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const K key = slot_key(s[i]);
        if (key_empty(key)) continue;
        uint32_t w = 0;
        d.orbit(key, [&](const K &) { w++; });
        score_bin_add(lds, bins, nbin, (uint16_t)slot_score(s[i]), w);
    }
    score_bins_flush(lds, bins, nbin);
}

// gm_select over a tier table (select_common.hpp): every matching representative emits each
// member of its orbit with the representative's record, as res_gather_kernel does.  The loop
// runs per wave; the orbit walks diverge, which select_note allows.
template <class D>
__global__ __launch_bounds__(256) void res_select_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ sl,
                                                         uint64_t cap, SelectDev s) {
    using K = key_t<D>;
    SelectTally t;
    for (uint64_t w0 = blockIdx.x * 256ull + (threadIdx.x & ~63u); w0 < cap; w0 += (uint64_t)gridDim.x * 256ull) {
        const uint64_t i = w0 + (threadIdx.x & 63u);
        if (i >= cap) continue;
        const K key = slot_key(sl[i]);
        if (key_empty(key)) continue;
        const uint16_t rec = record_of_score((uint16_t)slot_score(sl[i]));
        if (!select_match(s.values, s.rem_lo, s.rem_hi, rec)) continue;
        d.orbit(key, [&](const K &k) { select_note(s, t, true, k, rec); });
    }
    select_flush(s, t);
}

// gm_verify over one tier table (verify_common.hpp): table `t` of group `g` of the G x ntabs
// matrix `tabs` (row = owner rank, one row for the one-GPU engine; column = tier from the
// root's, t_root).  Every occupied slot: its key (valid, its own representative, of this tier
// and this owner), its place (a lookup ends at this slot), then its score against primitive()
// or against the best of ALL its children -- made as retro_kernel makes them, looked up in
// their owner's table of tiers t + 1 .. t + MAX_SKIP.
template <class D>
__global__ __launch_bounds__(256) void res_verify_kernel(D d, const typename KT<key_t<D>>::Res *__restrict__ tabs,
                                                         int G, int ntabs, int g, int t, int64_t t_root, VerifyDev v) {
    using K = key_t<D>;
    constexpr int S = D::MAX_SKIP;
    const typename KT<K>::Res self = tabs[(size_t)g * ntabs + t];
    const auto plain = unreduced(d);
    VerifyTally tally;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < self.cap; i += (uint64_t)gridDim.x * 256ull) {
        const K k = slot_key(self.s[i]);
        if (key_empty(k)) continue;
        int cls;
        if (!d.valid(k) || d.canon(k) != k || d.tier(k) - t_root != t || (int)owner_rank(k, (uint32_t)G) != g) {
            cls = VF_BAD_KEY;
        } else if (res_find_slot(self, k) != (int64_t)i) {
            cls = VF_MISPLACED;
        } else {
            const uint32_t stored = (uint32_t)(slot_score(self.s[i]) & 0xFFFFu);
            const int prim = d.primitive(k);
            uint32_t best = 0;
            bool missing = false;
            if (prim == UNDECIDED) {
                const int64_t tk = d.tier(k);
                plain.visit(k, [&](const K &ch) {
                    const int p = d.primitive(ch);
                    uint32_t sc;
                    if (p != UNDECIDED) {
                        sc = score_of_primitive(p);
                    } else {
                        const int64_t dt = d.tier(ch) - tk;
                        int f = -1;
                        if (dt >= 1 && dt <= S && t + dt < ntabs) {
                            const K cc = d.canon(ch);
                            f = res_find(tabs[(size_t)owner_rank(cc, (uint32_t)G) * ntabs + (t + dt)], cc);
                            tally.n[6]++;
                        }
                        missing |= f <= 0;
                        sc = f > 0 ? (uint32_t)f : 0u;
                    }
                    best = max(best, sc);
                    return true;
                });
            }
            cls = verify_class(stored, prim, best, missing);
        }
        verify_note(v, tally, cls, k);
    }
    verify_flush(v, tally);
}

// gm_moves over tier tables (moves_common.hpp).  The G x ntabs matrix of res_verify_kernel; a
// key's record is query_kernel's answer: valid, its tier one of the tables', its representative
// found in its owner's table of that tier.
template <class K>
struct TierTabs {
    const typename KT<K>::Res *tabs;
    int G, ntabs;
    int64_t t_root;
    template <class D>
    __device__ __forceinline__ uint16_t record(const D &d, const K &k) const {
        if (!d.valid(k)) return REC_UNSOLVED;
        const int64_t t = d.tier(k) - t_root;
        if (t < 0 || t >= ntabs) return REC_UNSOLVED;
        const K cc = d.canon(k);
        const int s = res_find(tabs[(size_t)owner_rank(cc, (uint32_t)G) * ntabs + t], cc);
        return s >= 0 ? record_of_score((uint16_t)s) : REC_UNSOLVED;
    }
};
template <class D>
__global__ __launch_bounds__(256) void res_moves_kernel(D d, TierTabs<key_t<D>> tab, MovesDev mv) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < mv.m; i += (uint64_t)gridDim.x * 256ull)
        moves_of_key(d, tab, mv, i);
}

// gm_reach over tier tables (reach_common.hpp): the accessor of reach_level_kernel.  The mark
// index of a key is the slot of its representative in its owner's table of its tier plus that
// table's base, a prefix sum of the capacities over the G x ntabs matrix.  The children are the
// plugin's own (the unreduced descriptor, as gm_moves), each brought to its representative by
// the lookup; a frontier holds representatives.
template <class D>
struct ReachTiers {
    using Key = key_t<D>;
    D d;
    const typename KT<Key>::Res *tabs;
    const uint64_t *base;
    int G, ntabs;
    int64_t t_root;
    __device__ __forceinline__ int64_t find(const Key &k, uint16_t &rec, Key &st) const {
        rec = REC_UNSOLVED;
        st = k;
        if (!d.valid(k)) return -1;
        const int64_t t = d.tier(k) - t_root;
        if (t < 0 || t >= ntabs) return -1;
        st = d.canon(k);
        const size_t tb = (size_t)owner_rank(st, (uint32_t)G) * ntabs + (size_t)t;
        const typename KT<Key>::Res T = tabs[tb];
        const int64_t at = res_find_slot(T, st);
        if (at < 0) return -1;
        rec = record_of_score((uint16_t)slot_score(T.s[at]));
        return rec == REC_UNSOLVED ? -1 : (int64_t)(base[tb] + (uint64_t)at);
    }
    __device__ __forceinline__ bool interior(const Key &k) const { return d.primitive(k) == UNDECIDED; }
    template <class F>
    __device__ __forceinline__ void visit(const Key &k, F &&f) const {
        const auto plain = unreduced(d);
        uint32_t seq = 0;
        plain.visit(k, [&](const Key &ch) {
            uint32_t pos = seq++;
            if constexpr (slot_order_t<D>::value) pos = (uint32_t)move_slot(plain, k, ch);
            f(ch, pos);
            return true;
        });
    }
    __device__ __forceinline__ uint32_t weight(const Key &st) const {
        uint32_t w = 0;
        d.orbit(st, [&](const Key &) { w++; });
        return w;
    }
};

// the sweep over one table: every marked representative emits each member of its orbit with
// the representative's record and side bits, as res_select_kernel emits a match
template <class D>
__global__ __launch_bounds__(256) void res_reach_sweep_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ sl,
                                                              uint64_t cap, uint64_t base, ReachDev r) {
    using K = key_t<D>;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256ull) {
        const K key = slot_key(sl[i]);
        if (key_empty(key)) continue;
        const uint32_t bits = reach_bits(r, base + i);
        if (!bits) continue;
        const uint16_t rec = record_of_score((uint16_t)slot_score(sl[i]));
        d.orbit(key, [&](const K &k) { reach_emit(r, k, rec, bits); });
    }
}

// gm_poke: the score of key's slot overwritten, or (remove) the slot emptied; *found = 1 if held
template <class K>
__global__ void res_poke_kernel(typename KT<K>::Res t, K key, uint64_t score, int remove, uint32_t *found) {
    if (threadIdx.x || blockIdx.x) return;
    const int64_t at = res_find_slot(t, key);
    *found = at >= 0;
    if (at < 0) return;
    if (remove) slot_clear(t.s[at]);
    else t.s[at].score = score;
}

template <class D>
__global__ void res_gather_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ s, uint64_t cap,
                                  key_t<D> *okeys, uint16_t *orec, unsigned long long *cursor) {
    using K = key_t<D>;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < cap;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const K key = slot_key(s[i]);
        if (key_empty(key)) continue;
        const uint16_t rec = record_of_score((uint16_t)slot_score(s[i]));
        d.orbit(key, [&](const K &k) {
            const unsigned long long at = atomicAdd(cursor, 1ull);
            okeys[at] = k;
            orec[at] = rec;
        });
    }
}

}  // namespace

template <class Slot>
inline int tier_alloc(Ctx *c, Slot **slots, uint64_t cap) {
    GM_TRY(dev_alloc(c, (void **)slots, cap * sizeof(Slot)));
    hipLaunchKernelGGL(slot_fill_kernel<Slot>, dim3(grid_for(cap)), dim3(256), 0, c->stream, *slots, cap);
    return GM_OK;
}

// grow a tier table to `cap` slots, re-inserting the keys it holds
template <class K>
inline int tier_grow(Ctx *c, SpTierT<K> &T, uint64_t cap, uint32_t *d_err) {
    typename KT<K>::Slot *ns;
    GM_TRY(tier_alloc(c, &ns, cap));
    if (T.cap) {
        typename KT<K>::Front dst{ns, cap, nullptr, eff_loc(T.loc, cap)};
        hipLaunchKernelGGL(front_rehash_kernel<K>, dim3(grid_for(T.cap)), dim3(256), 0, c->stream, T.slots, T.cap, dst,
                           d_err);
        dev_free(c, T.slots);
    }
    T.slots = ns;
    T.cap = cap;
    return GM_OK;
}

template <class K>
inline typename KT<K>::Res res_ref_of(const SpTierT<K> &T) {
    return typename KT<K>::Res{T.slots, T.cap, eff_loc(T.loc, T.cap)};
}

// capacity for `n` keys at the planned load (multiple of 1024)
inline uint64_t table_cap_for(uint64_t n) {
    const uint64_t c = (uint64_t)((double)n / TABLE_LOAD) + 1;
    return std::max<uint64_t>(1024, (c + 1023) & ~1023ull);
}

// Distinct fraction of a tier's incoming edges, predicted from the last insert
// pass (fresh keys / keys offered) with a margin; 1 (the exact upper bound)
// until a pass of some size has been seen.  GM_TEST_DEDUP_RATIO pins the
// ratio (tests use a tiny one to drive the full-table re-run path).
struct DedupEstimate {
    double ratio = 1.0;
    bool pinned = false;
    DedupEstimate() {
        if (const char *e = getenv("GM_TEST_DEDUP_RATIO")) {
            ratio = atof(e);
            pinned = true;
        }
    }
    void observe(uint64_t fresh, uint64_t offered) {
        if (pinned || offered < (1u << 20)) return;
        ratio = std::min(1.0, 1.25 * (double)fresh / (double)offered + 0.05);
    }
    void missed() {
        if (!pinned) ratio = 1.0;
    }
    uint64_t distinct(uint64_t offered) const { return (uint64_t)(ratio * (double)offered) + 1; }
};

// classify a finished tier table: scores in place, interior list, edge counts
// (scr[0, S) edges by step, scr[9] interior count, scr[10] positions seen)
// scr: [0, S) edges per tier step, [9] interior count, [10] positions, [11] positions with orbits
template <class D, bool COUNT = true, bool EDGES = COUNT>
inline void launch_classify(hipStream_t st, const D &d, typename KT<key_t<D>>::Slot *slots, uint64_t cap,
                            key_t<D> *ikeys, uint32_t *islot, unsigned long long *scr, uint32_t *err) {
    // a replay's classify (no edge or orbit counts) does less per row: 32 rows
    // per thread there (Toot 6x4 replay: 8.8 vs 9.5 ms; rows 8 / 4: 12.6 / 19.6 ms -- each
    // chunk's barriers and reservation atomic are paid fewer times)
    constexpr int rows = COUNT ? CROWS : 32;
    if (cap >= CLASSIFY_ROWS_MIN)
        hipLaunchKernelGGL((classify_kernel<D, rows, COUNT, EDGES>), dim3(grid_counted(cap / rows + 1)), dim3(256), 0,
                           st, d, slots, cap, ikeys, islot, scr + 9, scr, scr + 10, err);
    else
        hipLaunchKernelGGL((classify_kernel<D, 1, COUNT, EDGES>), dim3(grid_counted(cap)), dim3(256), 0, st, d, slots,
                           cap, ikeys, islot, scr + 9, scr, scr + 10, err);
}

// edges = false (the sharded path, whose bucket pass counts the children per bin): no edge counts
template <class D>
inline int classify_tier_table(Ctx *c, const D &d, SpTierT<key_t<D>> &T, unsigned long long *scr, uint32_t *d_err,
                               bool edges = true) {
    const uint64_t n = T.fcount;
    GM_TRY(dev_alloc(c, (void **)&T.ikeys, std::max<uint64_t>(n, 1) * sizeof(key_t<D>)));
    GM_TRY(dev_alloc(c, (void **)&T.islot, std::max<uint64_t>(n, 1) * 4));
    GM_TRY(dev_alloc(c, (void **)&T.iwon, std::max<uint64_t>(n, 1)));
    GM_HIP(hipMemsetAsync(scr, 0, 16 * sizeof(unsigned long long), c->stream));
    if (edges)
        launch_classify(c->stream, d, T.slots, T.cap, T.ikeys, T.islot, scr, d_err);
    else
        launch_classify<D, true, false>(c->stream, d, T.slots, T.cap, T.ikeys, T.islot, scr, d_err);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

template <class K>
inline void free_tier(Ctx *c, SpTierT<K> &T) {
    for (void *p : {(void *)T.slots, (void *)T.ikeys, (void *)T.islot, (void *)T.iwon, (void *)T.skeys, (void *)T.sslot,
                    (void *)T.coff, (void *)T.cslot, (void *)T.ccnt, (void *)T.pbest})
        dev_free(c, p);
    T = SpTierT<K>{};
}

// ----------------------------------------------------------------- readers
// The host side of export, query, digest and histogram over tier tables: the one-GPU engine
// passes its tiers, the sharded engine those of every rank it runs.
template <class K>
using TierList = std::vector<const SpTierT<K> *>;

// every position of the tables (each representative's orbit expanded), sorted by key
template <class D>
inline int tiers_export(Ctx *c, const D &d, const TierList<key_t<D>> &tiers, key_t<D> *keys, uint16_t *recs,
                        uint64_t cap, uint64_t *n) {
    using K = key_t<D>;
    uint64_t total = 0;
    for (auto *T : tiers) total += T->count_all;
    *n = total;
    if (!keys) return GM_OK;
    if (cap < total) {
        set_error("export buffer holds %llu, need %llu", (unsigned long long)cap, (unsigned long long)total);
        return GM_E_CAP;
    }
    DevBuf<K> dk;
    DevBuf<uint16_t> dr;
    DevBuf<unsigned long long> cur;
    GM_TRY(dk.alloc(std::max<uint64_t>(1, total)));
    GM_TRY(dr.alloc(std::max<uint64_t>(1, total)));
    GM_TRY(cur.alloc(1));
    GM_HIP(hipMemsetAsync(cur, 0, 8, c->stream));
    for (auto *T : tiers)
        if (T->count)
            hipLaunchKernelGGL(res_gather_kernel<D>, dim3(grid_for(T->cap)), dim3(256), 0, c->stream, d, T->slots, T->cap,
                               dk.p, dr.p, cur.p);
    std::vector<K> hk(total);
    std::vector<uint16_t> hr(total);
    GM_HIP(hipMemcpyAsync(hk.data(), dk, total * sizeof(K), hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipMemcpyAsync(hr.data(), dr, total * 2, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    std::vector<uint64_t> idx(total);
    for (uint64_t i = 0; i < total; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) { return hk[a] < hk[b]; });
    for (uint64_t i = 0; i < total; i++) {
        keys[i] = hk[idx[i]];
        recs[i] = hr[idx[i]];
    }
    return GM_OK;
}

template <class D>
inline int tiers_digest(Ctx *c, const D &d, const TierList<key_t<D>> &tiers, uint64_t *digest, uint64_t *n) {
    DevBuf<unsigned long long> acc;
    GM_TRY(acc.alloc(1));
    GM_HIP(hipMemsetAsync(acc, 0, 8, c->stream));
    uint64_t total = 0;
    for (auto *T : tiers) {
        total += T->count_all;
        if (T->count)
            hipLaunchKernelGGL(res_digest_kernel<D>, dim3(grid_counted(T->cap)), dim3(256), 0, c->stream, d, T->slots,
                               T->cap, acc.p);
    }
    unsigned long long h;
    GM_HIP(hipMemcpyAsync(&h, acc, 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    *digest = h;
    *n = total;
    return GM_OK;
}

// census of the tables; remoteness is below the number of tiers walked (`depth`): 3 x (depth + 1)
// bins (hist_common.hpp)
template <class D>
inline int tiers_histogram(Ctx *c, const D &d, const TierList<key_t<D>> &tiers, size_t depth, Hist *out) {
    ScoreBins b;
    GM_TRY(score_bins_begin(c, (uint32_t)depth + 1, &b));
    for (auto *T : tiers)
        if (T->count)
            hipLaunchKernelGGL(res_hist_kernel<D>, dim3(grid_counted(T->cap)), dim3(256), b.lds_bytes, c->stream, d,
                               T->slots, T->cap, b.d, b.nbin, b.use_lds);
    return score_bins_end(c, &b, out);
}

// gm_select over the tables (select_common.hpp)
template <class D>
inline int tiers_select(Ctx *c, const D &d, const TierList<key_t<D>> &tiers, const SelectDev &s) {
    for (auto *T : tiers)
        if (T->count)
            hipLaunchKernelGGL(res_select_kernel<D>, dim3(grid_counted(T->cap)), dim3(256), 0, c->stream, d, T->slots,
                               T->cap, s);
    GM_HIP(hipGetLastError());
    return GM_OK;
}

// One group of tier tables a query looks in: a tier per table from the root's (t_root) on.  A
// key is in at most one group (the sharded engine: one per rank); keys in none stay REC_UNSOLVED.
template <class K>
struct TierGroup {
    const std::vector<SpTierT<K>> *tiers;
    int64_t t_root;
};

template <class D>
inline int tiers_query(Ctx *c, const D &d, const std::vector<TierGroup<key_t<D>>> &groups, const key_t<D> *keys,
                       uint16_t *recs, uint64_t n) {
    using K = key_t<D>;
    using Res = typename KT<K>::Res;
    if (!n) return GM_OK;
    DevBuf<K> dk;
    DevBuf<uint16_t> dr;
    GM_TRY(dk.alloc(n));
    GM_TRY(dr.alloc(n));
    GM_HIP(hipMemcpyAsync(dk, keys, n * sizeof(K), hipMemcpyHostToDevice, c->stream));
    std::vector<uint16_t> part(n);
    for (uint64_t i = 0; i < n; i++) recs[i] = REC_UNSOLVED;
    for (auto &g : groups) {
        std::vector<Res> h(g.tiers->size());
        for (size_t t = 0; t < h.size(); t++) h[t] = res_ref_of((*g.tiers)[t]);
        DevBuf<Res> tabs;
        GM_TRY(tabs.alloc(std::max<size_t>(1, h.size())));
        if (!h.empty()) GM_HIP(hipMemcpyAsync(tabs, h.data(), h.size() * sizeof(Res), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(query_kernel<D>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, d, g.t_root,
                           tabs.p, (int)h.size(), dk.p, dr.p, n);
        GM_HIP(hipMemcpyAsync(part.data(), dr, n * 2, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < n; i++)
            if (part[i] != REC_UNSOLVED) recs[i] = part[i];
    }
    return GM_OK;
}

// the groups x tiers matrix of table references on the device (a group without a tier: no table)
template <class K>
inline int tiers_matrix(Ctx *c, const std::vector<TierGroup<K>> &groups, DevBuf<typename KT<K>::Res> *tabs,
                        int *ntabs) {
    using Res = typename KT<K>::Res;
    size_t nt = 0;
    for (auto &g : groups) nt = std::max(nt, g.tiers->size());
    std::vector<Res> h(std::max<size_t>(1, groups.size() * nt), Res{nullptr, 0, 0});
    for (size_t g = 0; g < groups.size(); g++)
        for (size_t t = 0; t < groups[g].tiers->size(); t++) h[g * nt + t] = res_ref_of((*groups[g].tiers)[t]);
    GM_TRY(tabs->alloc(h.size()));
    GM_HIP(hipMemcpyAsync(*tabs, h.data(), h.size() * sizeof(Res), hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));   // h leaves scope
    *ntabs = (int)nt;
    return GM_OK;
}

// gm_verify over tier tables: group g holds the keys of owner rank g (one group: the one-GPU engine)
template <class D>
inline int tiers_verify(Ctx *c, const D &d, const std::vector<TierGroup<key_t<D>>> &groups, const VerifyDev &v) {
    using K = key_t<D>;
    DevBuf<typename KT<K>::Res> tabs;
    int ntabs = 0;
    GM_TRY(tiers_matrix<K>(c, groups, &tabs, &ntabs));
    for (size_t g = 0; g < groups.size(); g++)
        for (size_t t = 0; t < groups[g].tiers->size(); t++) {
            const SpTierT<K> &T = (*groups[g].tiers)[t];
            if (!T.slots || !T.cap) continue;
            hipLaunchKernelGGL(res_verify_kernel<D>, dim3(grid_counted(T.cap)), dim3(256), 0, c->stream, d, tabs.p,
                               (int)groups.size(), ntabs, (int)g, (int)t, groups[g].t_root, v);
        }
    GM_HIP(hipGetLastError());
    GM_HIP(hipStreamSynchronize(c->stream));   // tabs leaves scope
    return GM_OK;
}

// gm_moves over tier tables: group g holds the keys of owner rank g (one group: the one-GPU engine)
template <class D>
inline int tiers_moves(Ctx *c, const D &d, const std::vector<TierGroup<key_t<D>>> &groups, const MovesReq &r) {
    using K = key_t<D>;
    DevBuf<typename KT<K>::Res> tabs;
    int ntabs = 0;
    GM_TRY(tiers_matrix<K>(c, groups, &tabs, &ntabs));
    const TierTabs<K> tab{tabs.p, (int)groups.size(), ntabs, groups.empty() ? 0 : groups[0].t_root};
    return moves_run(c, r, [&](const MovesDev &mv) {
        // random probes whose workgroups finish unevenly: grid_for's 8,192, as the insert kernels
        hipLaunchKernelGGL(res_moves_kernel<D>, dim3(grid_for(mv.m)), dim3(256), 0, c->stream, d, tab, mv);
        GM_HIP(hipGetLastError());
        return GM_OK;
    });   // moves_run ends synchronised: tabs may leave scope
}

// whether the tables hold one representative per orbit (games.hpp: the descriptor's sym, set per solve)
template <class D>
inline bool tables_reduced(const D &) { return false; }
inline bool tables_reduced(const DescToot &d) { return d.sym != 0; }
inline bool tables_reduced(const DescConnect &d) { return d.sym != 0; }
inline bool tables_reduced(const DescOthello &d) { return d.sym != 0; }

// gm_reach over tier tables: group g holds the keys of owner rank g (one group: the one-GPU engine)
template <class D>
inline int tiers_reach(Ctx *c, const D &d, const std::vector<TierGroup<key_t<D>>> &groups, const ReachReq &q) {
    using K = key_t<D>;
    if (reach_wants_first(q) && tables_reduced(d)) {
        set_error("gm_reach: GM_REACH_FIRST does not commute with the symmetries and this table holds one "
                  "representative per orbit: solve with GM_OPT_SYMMETRY 0");
        return GM_E_ARG;
    }
    DevBuf<typename KT<K>::Res> tabs;
    int ntabs = 0;
    GM_TRY(tiers_matrix<K>(c, groups, &tabs, &ntabs));
    // every table's first mark index
    std::vector<uint64_t> base(std::max<size_t>(1, groups.size() * (size_t)ntabs), 0);
    uint64_t units = 0;
    for (size_t g = 0; g < groups.size(); g++)
        for (size_t t = 0; t < (size_t)ntabs; t++) {
            base[g * ntabs + t] = units;
            if (t < groups[g].tiers->size() && (*groups[g].tiers)[t].slots) units += (*groups[g].tiers)[t].cap;
        }
    DevBuf<uint64_t> dbase;
    GM_TRY(dbase.alloc(base.size()));
    GM_HIP(hipMemcpyAsync(dbase, base.data(), base.size() * 8, hipMemcpyHostToDevice, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    const ReachTiers<D> acc{d, tabs.p, dbase.p, (int)groups.size(), ntabs, groups.empty() ? 0 : groups[0].t_root};
    // the capacities bound what can be marked
    return reach_run(
        c, q, ReachDims{units, units, (uint64_t)D::MAXC},
        [&](const ReachDev &r) {
            // random probes whose workgroups finish unevenly: grid_for's 8,192, as res_moves_kernel
            hipLaunchKernelGGL(reach_level_kernel<ReachTiers<D>>, dim3(grid_for(r.m)), dim3(256), 0, c->stream, acc, r);
            GM_HIP(hipGetLastError());
            return GM_OK;
        },
        [&](const ReachDev &r) {
            for (size_t g = 0; g < groups.size(); g++)
                for (size_t t = 0; t < groups[g].tiers->size(); t++) {
                    const SpTierT<K> &T = (*groups[g].tiers)[t];
                    if (!T.slots || !T.cap) continue;
                    hipLaunchKernelGGL(res_reach_sweep_kernel<D>, dim3(grid_counted(T.cap)), dim3(256), 0, c->stream, d,
                                       T.slots, T.cap, base[g * ntabs + t], r);
                }
            GM_HIP(hipGetLastError());
            return GM_OK;
        });   // reach_run ends synchronised: tabs and dbase may leave scope
}

// gm_poke in tier tables: the representative's slot in its owner's table of its tier
template <class D>
inline int tiers_poke(Ctx *c, const D &d, const std::vector<TierGroup<key_t<D>>> &groups, const key_t<D> &key,
                      uint16_t rec) {
    using K = key_t<D>;
    uint32_t found = 0;
    if (d.valid(key)) {
        const K k = d.canon(key);
        const auto &g = groups[owner_rank(k, (uint32_t)groups.size())];
        const int64_t t = d.tier(k) - g.t_root;
        if (t >= 0 && t < (int64_t)g.tiers->size() && (*g.tiers)[t].slots) {
            DevBuf<uint32_t> df;
            GM_TRY(df.alloc(1));
            hipLaunchKernelGGL(res_poke_kernel<K>, dim3(1), dim3(64), 0, c->stream, res_ref_of((*g.tiers)[t]), k,
                               (uint64_t)score_of_record(rec), rec == REC_UNSOLVED ? 1 : 0, df.p);
            GM_HIP(hipMemcpyAsync(&found, df, 4, hipMemcpyDeviceToHost, c->stream));
            GM_HIP(hipStreamSynchronize(c->stream));
        }
    }
    if (!found) { set_error("gm_poke: the key is not a stored position"); return GM_E_KEY; }
    return GM_OK;
}

// ----------------------------------------------------------------- record entries
// The nine read entries of an engine record (gm_internal.hpp Engine) over tier tables, once for
// both sparse engines.  E says how an engine names its tables:
//   E::desc(c, f)      f with the context's descriptor (with_desc, or with_desc_wide)
//   E::groups<K>(c)    its groups of tier tables: one, or one per rank it runs (a rank of a
//                      multi-process solve holds its hash share; gm_api.hip refuses it the reads
//                      that need the whole table)
// A translation unit instantiates TierReads<E> explicitly, so that its device pass, which sees
// no record (GM_ENGINE_RECORD), emits the kernels too.
template <class D>
struct TierView {
    using K = key_t<D>;
    const D &d;
    std::vector<TierGroup<K>> groups;
    TierList<K> tiers;   // every tier of every group
    size_t depth = 0;    // the most tiers a group holds
    static K *keys(void *p) { return (K *)p; }   // the record's keys: K is the context's device key type
    static const K *keys(const void *p) { return (const K *)p; }
};

template <class E>
struct TierReads {
    template <class F>
    static int with_tables(Ctx *c, F &&f) {
        return E::desc(c, [&](const auto &d) {
            using D = std::decay_t<decltype(d)>;
            TierView<D> v{d, E::template groups<key_t<D>>(c), {}, 0};
            for (auto &g : v.groups) {
                v.depth = std::max(v.depth, g.tiers->size());
                for (auto &T : *g.tiers) v.tiers.push_back(&T);
            }
            return f(v);
        });
    }
    static int export_(Ctx *c, void *keys, uint16_t *recs, uint64_t cap, uint64_t *n) {
        return with_tables(c, [&](const auto &v) { return tiers_export(c, v.d, v.tiers, v.keys(keys), recs, cap, n); });
    }
    static int query(Ctx *c, const void *keys, uint16_t *recs, uint64_t n) {
        return with_tables(c, [&](const auto &v) { return tiers_query(c, v.d, v.groups, v.keys(keys), recs, n); });
    }
    static int digest(Ctx *c, uint64_t *digest, uint64_t *n) {
        return with_tables(c, [&](const auto &v) { return tiers_digest(c, v.d, v.tiers, digest, n); });
    }
    static int histogram(Ctx *c, Hist *out) {
        return with_tables(c, [&](const auto &v) { return tiers_histogram(c, v.d, v.tiers, v.depth, out); });
    }
    static int select(Ctx *c, const SelectDev &s) {
        return with_tables(c, [&](const auto &v) { return tiers_select(c, v.d, v.tiers, s); });
    }
    static int verify(Ctx *c, const VerifyDev &vf) {
        return with_tables(c, [&](const auto &v) { return tiers_verify(c, v.d, v.groups, vf); });
    }
    static int moves(Ctx *c, const MovesReq &r) {
        return with_tables(c, [&](const auto &v) { return tiers_moves(c, v.d, v.groups, r); });
    }
    static int reach(Ctx *c, const ReachReq &q) {
        return with_tables(c, [&](const auto &v) { return tiers_reach(c, v.d, v.groups, q); });
    }
    static int poke(Ctx *c, const void *key, uint16_t rec) {
        return with_tables(c, [&](const auto &v) { return tiers_poke(c, v.d, v.groups, *v.keys(key), rec); });
    }
};

// ------------------------------------------------------------------ import
// gm_import: the tier tables a solve from the root would hold had it produced exactly the given
// (key, record) pairs -- what the readers above look at, built without a solve.  Four passes
// over the input, which stays on the device in chunks of at most IMPORT_CHUNK keys (a table of
// more is uploaded again by each pass):
//   scan     one lane per key: valid(), tier - t_root in [0, IMPORT_MAX_TIERS), the record a
//            WIN / LOSS / TIE one; keys counted per tier -- an exact upper bound of the tier's
//            table, so nothing is predicted
//   insert   canon(key) into its tier's table (front_insert), fresh inserts counted per tier
//   score    after the insert kernel: the slot's score word goes 0 -> score_of_record by
//            atomicCAS; an old value that is neither 0 nor the same score is a conflict (two
//            members of one orbit, or one key twice, with different records)
//   census   per table: stored keys and the positions their orbits stand for (count, count_all)
// A key that breaks a rule is reported as index << 3 | reason through one atomicMin word, so the
// host names the first offender.  The per-tier counters are LDS bins, flushed with one global
// atomic per non-empty bin per workgroup.  No kernel waits on another: every loop ends at the
// list's length or a probe limit.
constexpr int IMPORT_MAX_TIERS = 1024;
constexpr uint64_t IMPORT_CHUNK = 1ull << 24;
enum : uint32_t { IMP_INVALID = 1, IMP_TIER = 2, IMP_DEPTH = 3, IMP_RECORD = 4, IMP_CONFLICT = 5, IMP_LOST = 6 };

namespace {

__device__ __forceinline__ void import_note(unsigned long long *first, uint64_t index, uint32_t why) {
    atomicMin(first, (unsigned long long)(index << 3 | why));
}

__device__ __forceinline__ void tier_bins_clear(uint32_t *bins) {
    for (int i = threadIdx.x; i < IMPORT_MAX_TIERS; i += blockDim.x) bins[i] = 0;
    __syncthreads();
}
__device__ __forceinline__ void tier_bins_flush(const uint32_t *bins, unsigned long long *out) {
    __syncthreads();
    for (int i = threadIdx.x; i < IMPORT_MAX_TIERS; i += blockDim.x)
        if (bins[i]) atomicAdd(out + i, (unsigned long long)bins[i]);
}

template <class D>
__global__ __launch_bounds__(256) void import_scan_kernel(D d, int64_t t_root, const key_t<D> *__restrict__ keys,
                                                          const uint16_t *__restrict__ recs, uint64_t n, uint64_t base,
                                                          unsigned long long *per_tier, unsigned long long *first) {
    __shared__ uint32_t bins[IMPORT_MAX_TIERS];
    tier_bins_clear(bins);
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
        const key_t<D> k = keys[i];
        const uint16_t rec = recs[i];
        uint32_t why = 0;
        int64_t t = 0;
        if (!d.valid(k)) {
            why = IMP_INVALID;
        } else {
            t = d.tier(k) - t_root;
            if (t < 0) why = IMP_TIER;
            else if (t >= IMPORT_MAX_TIERS) why = IMP_DEPTH;
            else if (rec == REC_UNSOLVED || (rec >> 14) > TIE) why = IMP_RECORD;
        }
        if (why) import_note(first, base + i, why);
        else atomicAdd(&bins[t], 1u);
    }
    tier_bins_flush(bins, per_tier);
}

template <class D>
__global__ __launch_bounds__(256) void import_insert_kernel(D d, int64_t t_root, const key_t<D> *__restrict__ keys,
                                                            uint64_t n,
                                                            const typename KT<key_t<D>>::Front *__restrict__ fronts,
                                                            unsigned long long *fresh, uint32_t *err) {
    __shared__ uint32_t bins[IMPORT_MAX_TIERS];
    tier_bins_clear(bins);
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
        if (*(volatile uint32_t *)err & DEV_ERR_TABLE_FULL) break;   // the pass is re-run into larger tables
        const key_t<D> k = d.canon(keys[i]);
        const int64_t t = d.tier(k) - t_root;   // in range: the scan passed
        if (front_insert(fronts[t], k, err)) atomicAdd(&bins[t], 1u);
    }
    tier_bins_flush(bins, fresh);
}

template <class D>
__global__ __launch_bounds__(256) void import_score_kernel(D d, int64_t t_root, const key_t<D> *__restrict__ keys,
                                                           const uint16_t *__restrict__ recs, uint64_t n, uint64_t base,
                                                           const typename KT<key_t<D>>::Res *__restrict__ tabs,
                                                           unsigned long long *first) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256ull) {
        const key_t<D> k = d.canon(keys[i]);
        const typename KT<key_t<D>>::Res r = tabs[d.tier(k) - t_root];
        const int64_t at = res_find_slot(r, k);
        if (at < 0) { import_note(first, base + i, IMP_LOST); continue; }
        const unsigned long long sc = score_of_record(recs[i]);
        const unsigned long long old = atomicCAS((unsigned long long *)&r.s[at].score, 0ull, sc);
        if (old != 0ull && old != sc) import_note(first, base + i, IMP_CONFLICT);
    }
}

// out[0] += stored keys, out[1] += the positions their orbits stand for
template <class D>
__global__ __launch_bounds__(256) void import_census_kernel(D d, const typename KT<key_t<D>>::Slot *__restrict__ s,
                                                            uint64_t cap, unsigned long long *out) {
    using K = key_t<D>;
    uint64_t cnt = 0, all = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * 256ull) {
        const K key = slot_key(s[i]);
        if (key_empty(key)) continue;
        cnt++;
        d.orbit(key, [&](const K &) { all++; });
    }
    block_add(out, cnt);
    block_add(out + 1, all);
}

}  // namespace

// a key as gm_last_error shows it: its ABI words in hex, least significant first
inline std::string key_hex(uint64_t k) {
    char b[32];
    snprintf(b, sizeof b, "0x%llx", (unsigned long long)k);
    return b;
}
inline std::string key_hex(const K128 &k) {
    uint64_t w[3];
    DescOthello8::to_words(k, w);
    char b[96];
    snprintf(b, sizeof b, "0x%llx 0x%llx 0x%llx", (unsigned long long)w[0], (unsigned long long)w[1],
             (unsigned long long)w[2]);
    return b;
}

// the refusal of the key an import kernel noted (index << 3 | reason)
template <class K>
inline int import_refuse(unsigned long long first, const K *keys, const uint16_t *recs) {
    const uint64_t i = first >> 3;
    const std::string k = key_hex(keys[i]);
    switch ((uint32_t)(first & 7)) {
    case IMP_INVALID:
        set_error("gm_import: key %s (index %llu) is not a valid position", k.c_str(), (unsigned long long)i);
        return GM_E_KEY;
    case IMP_TIER:
        set_error("gm_import: key %s (index %llu) lies in a tier above the root's", k.c_str(), (unsigned long long)i);
        return GM_E_KEY;
    case IMP_DEPTH:
        set_error("gm_import: key %s (index %llu) lies %d or more tiers below the root", k.c_str(), (unsigned long long)i,
                  IMPORT_MAX_TIERS);
        return GM_E_CAP;
    case IMP_RECORD:
        set_error("gm_import: key %s (index %llu) has record 0x%04x, not a WIN / LOSS / TIE record", k.c_str(),
                  (unsigned long long)i, recs[i]);
        return GM_E_ARG;
    case IMP_CONFLICT:
        set_error("gm_import: key %s (index %llu) is given twice, or shares a symmetry orbit with another key, with "
                  "different records", k.c_str(), (unsigned long long)i);
        return GM_E_ARG;
    }
    set_error("gm_import: key %s (index %llu) was not found after its insert", k.c_str(), (unsigned long long)i);
    return GM_E_STATE;
}

// GM_TRACE: the phases of an import by events (upload, scan, insert, score, census)
struct ImportClock {
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms[5] = {0, 0, 0, 0, 0};
    bool on = false;
    hipStream_t st = nullptr;
    ImportClock(hipStream_t s, bool enable) : st(s) {
        on = enable && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
    }
    ~ImportClock() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void begin() {
        if (on) (void)hipEventRecord(ev[0], st);
    }
    void end(int phase) {
        if (!on) return;
        float t = 0;
        (void)hipEventRecord(ev[1], st);
        if (hipEventSynchronize(ev[1]) == hipSuccess && hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) ms[phase] += t;
    }
};

// Build `tiers` (empty on entry) from n (key, record) pairs; on GM_OK every tier has its table,
// count, count_all, fcount = count and no interior list.  The caller frees `tiers` on failure.
template <class D>
inline int tiers_import(Ctx *c, const D &d, int64_t t_root, uint32_t loc, const key_t<D> *keys, const uint16_t *recs,
                        uint64_t n, std::vector<SpTierT<key_t<D>>> &tiers) {
    using K = key_t<D>;
    using Front = typename KT<K>::Front;
    using Res = typename KT<K>::Res;
    using Slot = typename KT<K>::Slot;
    constexpr int NT = IMPORT_MAX_TIERS;
    // GM_TEST_IMPORT_CHUNK: tests use a small chunk to drive the re-upload path with a small table
    const char *tc = getenv("GM_TEST_IMPORT_CHUNK");
    const uint64_t limit = tc && atoll(tc) > 0 ? std::min<uint64_t>(atoll(tc), IMPORT_CHUNK) : IMPORT_CHUNK;
    const uint64_t chunk = std::min(n, limit);
    const bool resident = n <= chunk;   // one upload serves every pass
    ImportClock clk(c->stream, trace_on());
    DevBuf<K> dk;
    DevBuf<uint16_t> dr;
    DevBuf<unsigned long long> acc;   // [0] first offender, [1, NT] keys per tier, (NT, 2 NT] fresh inserts per tier
    DevBuf<uint32_t> derr;
    GM_TRY(dk.alloc(chunk));
    GM_TRY(dr.alloc(chunk));
    GM_TRY(acc.alloc(1 + 2 * NT));
    GM_TRY(derr.alloc(1));
    auto upload = [&](uint64_t o, uint64_t m, bool with_recs) -> int {
        clk.begin();
        GM_HIP(hipMemcpyAsync(dk, keys + o, m * sizeof(K), hipMemcpyHostToDevice, c->stream));
        if (with_recs) GM_HIP(hipMemcpyAsync(dr, recs + o, m * 2, hipMemcpyHostToDevice, c->stream));
        clk.end(0);
        return GM_OK;
    };
    std::vector<unsigned long long> h(1 + 2 * NT);

    // ---------------- scan
    GM_HIP(hipMemsetAsync(acc, 0xFF, 8, c->stream));
    GM_HIP(hipMemsetAsync(acc.p + 1, 0, 2 * NT * 8, c->stream));
    for (uint64_t o = 0; o < n; o += chunk) {
        const uint64_t m = std::min(chunk, n - o);
        GM_TRY(upload(o, m, true));
        clk.begin();
        hipLaunchKernelGGL(import_scan_kernel<D>, dim3(grid_counted(m)), dim3(256), 0, c->stream, d, t_root, dk.p, dr.p, m,
                           o, acc.p + 1, acc.p);
        clk.end(1);
    }
    GM_HIP(hipGetLastError());
    GM_HIP(hipMemcpyAsync(h.data(), acc, (1 + NT) * 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    if (h[0] != ~0ull) return import_refuse(h[0], keys, recs);
    size_t ntiers = 0;
    for (size_t t = 0; t < (size_t)NT; t++)
        if (h[1 + t]) ntiers = t + 1;
    tiers.assign(ntiers, SpTierT<K>{});
    std::vector<uint64_t> offered(ntiers);
    for (size_t t = 0; t < ntiers; t++) {
        offered[t] = h[1 + t];
        tiers[t].loc = loc;
        tiers[t].tier = t_root + (int64_t)t;
        if (!offered[t]) continue;
        // GM_TEST_IMPORT_TIGHT: tests start from tables a quarter of the size, which fill up
        // (MAX_PROBE) and drive the re-run below
        tiers[t].cap = getenv("GM_TEST_IMPORT_TIGHT") ? std::max<uint64_t>(64, offered[t] / 4) : table_cap_for(offered[t]);
        GM_TRY(tier_alloc(c, &tiers[t].slots, tiers[t].cap));
    }

    // ---------------- insert (a full table: one re-run into tables of twice the planned size)
    DevBuf<Front> fronts;
    DevBuf<Res> tabs;
    GM_TRY(fronts.alloc(ntiers));
    GM_TRY(tabs.alloc(ntiers));
    for (int attempt = 0;; attempt++) {
        std::vector<Front> hf(ntiers);
        for (size_t t = 0; t < ntiers; t++)
            hf[t] = Front{tiers[t].slots, tiers[t].cap, nullptr, eff_loc(tiers[t].loc, tiers[t].cap)};
        GM_HIP(hipMemcpyAsync(fronts, hf.data(), ntiers * sizeof(Front), hipMemcpyHostToDevice, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));   // hf leaves scope
        GM_HIP(hipMemsetAsync(acc.p + 1 + NT, 0, NT * 8, c->stream));
        GM_HIP(hipMemsetAsync(derr, 0, 4, c->stream));
        for (uint64_t o = 0; o < n; o += chunk) {
            const uint64_t m = std::min(chunk, n - o);
            if (!resident) GM_TRY(upload(o, m, false));
            clk.begin();
            hipLaunchKernelGGL(import_insert_kernel<D>, dim3(grid_for(m)), dim3(256), 0, c->stream, d, t_root, dk.p, m,
                               fronts.p, acc.p + 1 + NT, derr.p);
            clk.end(2);
        }
        GM_HIP(hipGetLastError());
        uint32_t e = 0;
        GM_HIP(hipMemcpyAsync(&e, derr, 4, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipMemcpyAsync(h.data() + 1 + NT, acc.p + 1 + NT, NT * 8, hipMemcpyDeviceToHost, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));
        if (!e) break;
        if (e != DEV_ERR_TABLE_FULL || attempt) return dev_error_to_gm(e);
        for (size_t t = 0; t < ntiers; t++) {
            if (!tiers[t].cap) continue;
            dev_free(c, tiers[t].slots);
            tiers[t].slots = nullptr;
            tiers[t].cap = 2 * table_cap_for(offered[t]);
            GM_TRY(tier_alloc(c, &tiers[t].slots, tiers[t].cap));
        }
    }

    // ---------------- score
    {
        std::vector<Res> hr(ntiers);
        for (size_t t = 0; t < ntiers; t++) hr[t] = res_ref_of(tiers[t]);
        GM_HIP(hipMemcpyAsync(tabs, hr.data(), ntiers * sizeof(Res), hipMemcpyHostToDevice, c->stream));
        GM_HIP(hipStreamSynchronize(c->stream));   // hr leaves scope
    }
    for (uint64_t o = 0; o < n; o += chunk) {
        const uint64_t m = std::min(chunk, n - o);
        if (!resident) GM_TRY(upload(o, m, true));
        clk.begin();
        hipLaunchKernelGGL(import_score_kernel<D>, dim3(grid_for(m)), dim3(256), 0, c->stream, d, t_root, dk.p, dr.p, m, o,
                           tabs.p, acc.p);
        clk.end(3);
    }
    GM_HIP(hipGetLastError());
    GM_HIP(hipMemcpyAsync(h.data(), acc, 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    if (h[0] != ~0ull) return import_refuse(h[0], keys, recs);

    // ---------------- census
    DevBuf<unsigned long long> cen;
    GM_TRY(cen.alloc(2 * ntiers));
    GM_HIP(hipMemsetAsync(cen, 0, 2 * ntiers * 8, c->stream));
    clk.begin();
    for (size_t t = 0; t < ntiers; t++)
        if (tiers[t].cap)
            hipLaunchKernelGGL(import_census_kernel<D>, dim3(grid_counted(tiers[t].cap)), dim3(256), 0, c->stream, d,
                               (const Slot *)tiers[t].slots, tiers[t].cap, cen.p + 2 * t);
    clk.end(4);
    GM_HIP(hipGetLastError());
    std::vector<unsigned long long> hc(2 * ntiers);
    GM_HIP(hipMemcpyAsync(hc.data(), cen, hc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    GM_HIP(hipStreamSynchronize(c->stream));
    uint64_t all = 0;
    for (size_t t = 0; t < ntiers; t++) {
        if (hc[2 * t] != h[1 + NT + t]) {
            set_error("gm_import: tier %zu holds %llu keys after %llu fresh inserts", t, hc[2 * t], h[1 + NT + t]);
            return GM_E_STATE;
        }
        tiers[t].count = tiers[t].fcount = hc[2 * t];
        tiers[t].count_all = hc[2 * t + 1];
        all += hc[2 * t + 1];
    }
    if (clk.on)
        fprintf(stderr, "[gm] import of %llu keys: upload %.3f scan %.3f insert %.3f score %.3f census %.3f ms\n",
                (unsigned long long)n, clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4]);
    if (all != n) {
        // the stored representatives' orbits do not add up to the input: name a key given twice, if any
        std::vector<K> s(keys, keys + n);
        std::sort(s.begin(), s.end(), [](const K &a, const K &b) { return a < b; });
        for (uint64_t i = 1; i < n; i++)
            if (s[i] == s[i - 1]) {
                set_error("gm_import: key %s is given twice", key_hex(s[i]).c_str());
                return GM_E_ARG;
            }
        set_error("gm_import: %llu keys, but the stored representatives' orbits hold %llu positions (first key %s): "
                  "duplicate keys or incomplete orbits; GM_OPT_SYMMETRY 0 imports the keys as given",
                  (unsigned long long)n, (unsigned long long)all, key_hex(keys[0]).c_str());
        return GM_E_ARG;
    }
    return GM_OK;
}

// what gm_import reports of imported tier tables: positions, per-tier counts, table bytes
template <class K>
inline void import_account(Ctx *c, const std::vector<SpTierT<K>> &tiers) {
    uint64_t n = 0, stored = 0, tb = 0;
    c->tier_counts.clear();
    for (auto &T : tiers) {
        stored += T.count;
        n += T.count_all;
        tb += T.cap * sizeof(typename KT<K>::Slot);
        c->tier_counts.push_back(T.count_all);
    }
    c->n_positions = n;
    c->stats.n_positions = n;
    c->stats.n_stored = stored;
    c->stats.n_tiers = (int32_t)tiers.size();
    c->stats.table_bytes = tb;
}

}  // namespace gm
