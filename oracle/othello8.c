/* CPU oracle for Othello on the reference plugin's default 8x8 board (TEST INFRASTRUCTURE ONLY;
 * part of liboracle.so, Python binding oracle/othello8.py).
 *
 * Written from the reference plugin's rules, reference test_games/othello_bit_new.py:36-170,
 * as a walk over squares and directions on a cell array, in the manner of oth_legit /
 * oth_flip_dir of gm_oracle.c -- NOT from the shift-and-mask generator of csrc/games.hpp, so
 * that the two check each other:
 *   gen_moves (:133-170)  squares in the order x = 0..7 outer, y = 0..7 inner; a square is a
 *                         move when it is blank and some direction (dx outer, dy inner) shows
 *                         a run of opponent discs closed by a disc of the mover; no move at
 *                         all gives the single move None;
 *   do_move (:88-130)     None: the pass count + 1 and NOTHING else -- the mover stays (:122-124);
 *                         else the pass count is reset, the disc is placed, every direction's
 *                         closed run is flipped, and the turn changes;
 *   primitive (:58-84)    a full board or a pass count >= 2 ends the game: TIE on equal counts,
 *                         else LOSS when (black > white) xor (turn == 1), else WIN.
 *
 * A position is the plugin's 18-byte string as the three ABI key words of include/gmsolve.h
 * (tests/golden/othello8_words.py): with W / B the white / black planes read big-endian
 * (string bit j = 8y + x is plane bit 63 - j),
 *   I = W << 80 | B << 16 | turn << 8 | pass,   w0 = I mod 2^64, w1 = (I >> 64) mod 2^64, w2 = I >> 128.
 *
 * The solve keeps, per tier (3 * discs + pass count) and per hash bucket, a sorted array of the
 * distinct positions: forward, the children of a tier are thrown into the buckets of their
 * tiers and each bucket is sorted and deduplicated on its own; backward, a child is found by
 * binary search in its bucket.  Buckets are the unit of parallel work, so the result does not
 * depend on the number of threads.  Fold: Appendix A, as gm_oracle.c pref / from_pref. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define WIN 0
#define LOSS 1
#define TIE 2
#define UNDECIDED 4

#define OW 2
#define OB 1

static char o8_err[256];
const char *oracle_othello8_last_error(void) { return o8_err; }

typedef struct { uint64_t w[3]; } o8key;
typedef struct { int cell[64]; int turn, pass; } o8pos;   /* cell[8y + x] */

static int o8_decode(const uint64_t *w, o8pos *s) {
    if (w[2] >> 16) return -1;
    const uint64_t W = (w[1] >> 16) | (w[2] << 48), B = (w[0] >> 16) | (w[1] << 48);
    if (W & B) return -1;
    s->turn = (int)((w[0] >> 8) & 0xFF);
    s->pass = (int)(w[0] & 0xFF);
    if ((s->turn != 1 && s->turn != 2) || s->pass > 2) return -1;
    for (int j = 0; j < 64; j++)
        s->cell[j] = ((W >> (63 - j)) & 1) ? OW : (((B >> (63 - j)) & 1) ? OB : 0);
    return 0;
}
static void o8_encode(const o8pos *s, uint64_t *w) {
    uint64_t W = 0, B = 0;
    for (int j = 0; j < 64; j++) {
        if (s->cell[j] == OW) W |= 1ull << (63 - j);
        if (s->cell[j] == OB) B |= 1ull << (63 - j);
    }
    w[0] = (B << 16) | ((uint64_t)s->turn << 8) | (uint64_t)s->pass;
    w[1] = (B >> 48) | (W << 16);
    w[2] = W >> 48;
}
static int o8_get(const o8pos *s, int x, int y) { return s->cell[8 * y + x]; }
static int o8_mover(const o8pos *s) { return s->turn == 1 ? OB : OW; }
static int o8_discs(const o8pos *s) {
    int n = 0;
    for (int j = 0; j < 64; j++) n += s->cell[j] != 0;
    return n;
}
static int o8_tier(const o8pos *s) { return 3 * o8_discs(s) + s->pass; }

static int o8_prim(const o8pos *s) {
    int black = 0, white = 0;
    for (int j = 0; j < 64; j++) {
        black += s->cell[j] == OB;
        white += s->cell[j] == OW;
    }
    if (black + white != 64 && s->pass < 2) return UNDECIDED;
    if (black == white) return TIE;
    return ((black > white) ^ (s->turn == 1)) ? LOSS : WIN;
}
/* legit_helper (:148-160) from the square next to the candidate: opponent discs, then a mover's */
static int o8_closed_run(const o8pos *s, int x, int y, int dx, int dy) {
    const int me = o8_mover(s), opp = me == OB ? OW : OB;
    int seen = 0;
    for (;; x += dx, y += dy, seen++) {
        if (x < 0 || y < 0 || x >= 8 || y >= 8) return 0;
        const int c = o8_get(s, x, y);
        if (c == opp) continue;
        return c == me && seen > 0;
    }
}
static int o8_legit(const o8pos *s, int x, int y) {
    if (o8_get(s, x, y)) return 0;
    for (int dx = -1; dx <= 1; dx++)
        for (int dy = -1; dy <= 1; dy++)
            if ((dx || dy) && o8_closed_run(s, x + dx, y + dy, dx, dy)) return 1;
    return 0;
}
/* flip_helper / flip_helper2 (:100-118) on the successor: the run is flipped only when closed */
static void o8_flip_dir(o8pos *c, int x, int y, int dx, int dy, int me) {
    const int opp = me == OB ? OW : OB;
    int run[8], n = 0;
    for (;; x += dx, y += dy) {
        if (x < 0 || y < 0 || x >= 8 || y >= 8) return;
        const int v = o8_get(c, x, y);
        if (v == opp) { run[n++] = 8 * y + x; continue; }
        if (v == me)
            for (int i = 0; i < n; i++) c->cell[run[i]] = me;
        return;
    }
}
/* children in gen_moves order; returns their number (>= 1 for a non-primitive position) */
static int o8_kids(const o8pos *s, o8pos *out) {
    int n = 0;
    const int me = o8_mover(s);
    for (int x = 0; x < 8; x++)
        for (int y = 0; y < 8; y++) {
            if (!o8_legit(s, x, y)) continue;
            o8pos c = *s;
            c.pass = 0;
            c.cell[8 * y + x] = me;
            for (int dx = -1; dx <= 1; dx++)
                for (int dy = -1; dy <= 1; dy++)
                    if (dx || dy) o8_flip_dir(&c, x + dx, y + dy, dx, dy, me);
            c.turn = c.turn % 2 + 1;
            out[n++] = c;
        }
    if (n == 0) {
        out[0] = *s;
        out[0].pass += 1;
        n = 1;
    }
    return n;
}

/* primitive value, tier and (for a non-primitive position) the children's words, 3 per child,
 * in gen_moves order; children holds 64 * 3 words.  -1 when the words are no position. */
int oracle_othello8_expand(const uint64_t *words, uint64_t *children, int *n_children, int *primitive,
                           int64_t *tier) {
    o8pos s, kids[64];
    if (o8_decode(words, &s)) { snprintf(o8_err, sizeof o8_err, "words are no 8x8 position"); return -1; }
    *primitive = o8_prim(&s);
    *tier = o8_tier(&s);
    *n_children = 0;
    if (*primitive != UNDECIDED) return 0;
    const int n = o8_kids(&s, kids);
    for (int i = 0; i < n; i++) o8_encode(&kids[i], children + 3 * i);
    *n_children = n;
    return 0;
}

/* ------------------------------------------------------------------ digests */
static uint64_t o8_mix64(uint64_t x) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
static uint64_t o8_term(uint64_t key, uint16_t rec) { return o8_mix64(key * 0x9E3779B97F4A7C15ull + rec); }
/* the layout-independent fold of tests/golden/othello8_words.py */
static uint64_t o8_fold(const uint64_t *w) {
    return o8_mix64(w[0] ^ o8_mix64(w[1] ^ o8_mix64(w[2] ^ 0x6A09E667F3BCC908ull)));
}
/* gm_digest's word for a position: the device's 128-bit key as csrc/games.hpp documents it
 * (lo = white plane; hi = occupied plane with its four centre bits reused: bit 27 white to
 * move, bits 28 / 35 the pass count, bit 36 always set) folded by mix_key (gm_common.hpp) */
static uint64_t o8_device_word(const uint64_t *w) {
    const uint64_t W = (w[1] >> 16) | (w[2] << 48), B = (w[0] >> 16) | (w[1] << 48);
    const int turn = (int)((w[0] >> 8) & 0xFF), pass = (int)(w[0] & 0xFF);
    const uint64_t centre = (1ull << 27) | (1ull << 28) | (1ull << 35) | (1ull << 36);
    const uint64_t hi = ((W | B) & ~centre) | (turn == 2 ? 1ull << 27 : 0) | ((pass & 1) ? 1ull << 28 : 0) |
                        ((pass & 2) ? 1ull << 35 : 0) | (1ull << 36);
    return o8_mix64(W ^ o8_mix64(hi ^ 0x2545F4914F6CDD1Dull));
}

/* ------------------------------------------------------------------ solve */
#define O8_NB 64          /* hash buckets per tier */
#define O8_TIERS 196      /* 3 * 64 + 2 < 196 */
#define O8_SKIP 3         /* a move lands 3 - pass tiers deeper, a pass 1 */

typedef struct { o8key *v; uint64_t n, cap; } o8vec;
typedef struct { o8key *keys; uint16_t *rec; uint64_t n; } o8seg;

static int o8_push(o8vec *a, const o8key *k) {
    if (a->n == a->cap) {
        const uint64_t nc = a->cap ? a->cap * 2 : 256;
        o8key *nv = (o8key *)realloc(a->v, nc * sizeof(o8key));
        if (!nv) return -1;
        a->v = nv;
        a->cap = nc;
    }
    a->v[a->n++] = *k;
    return 0;
}
static int o8_cmp(const void *a, const void *b) {
    const uint64_t *x = ((const o8key *)a)->w, *y = ((const o8key *)b)->w;
    for (int i = 2; i >= 0; i--)
        if (x[i] != y[i]) return x[i] < y[i] ? -1 : 1;
    return 0;
}
static int o8_bucket(const uint64_t *w) { return (int)(o8_fold(w) >> 40) & (O8_NB - 1); }
static int64_t o8_find(const o8seg *s, const o8key *k) {
    uint64_t lo = 0, hi = s->n;
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (o8_cmp(&s->keys[m], k) < 0) lo = m + 1; else hi = m;
    }
    return (lo < s->n && o8_cmp(&s->keys[lo], k) == 0) ? (int64_t)lo : -1;
}
static uint32_t o8_pref(uint16_t rec) {
    const uint32_t v = rec >> 14, r = rec & 0x3FFF;
    if (v == LOSS) return 0x30000u | (0x3FFFu - r);
    if (v == TIE) return 0x20000u | (0x3FFFu - r);
    return 0x10000u | r;
}
static uint16_t o8_from_pref(uint32_t best) {
    const uint32_t cls = best >> 16, low = best & 0xFFFF;
    if (cls == 3) return (uint16_t)((WIN << 14) | (0x3FFFu - low + 1));
    if (cls == 2) return (uint16_t)((TIE << 14) | (0x3FFFu - low + 1));
    return (uint16_t)((LOSS << 14) | (low + 1));
}

typedef struct { o8key k; uint16_t rec; } o8ent;

void oracle_othello8_free(void *p) { free(p); }

/* Strong solve from root_words on `threads` OpenMP threads (<= 0: all).  Outputs the number of
 * positions, the positions per tier (index = tier - the root's tier), the root's record,
 * word_digest and the gm_digest-form digest.  want > 0 also returns table entries in key order
 * (ascending I): all of them when want >= positions, else entries floor(i * positions / want),
 * i < want; *out_words (3 per entry) and *out_recs are freed with oracle_othello8_free.
 * Returns 0, or -1 with oracle_othello8_last_error(). */
int oracle_othello8_solve(const uint64_t *root_words, int threads, uint64_t *n_positions, uint64_t *per_tier,
                          int per_tier_cap, int *n_tiers, uint16_t *root_record, uint64_t *word_digest,
                          uint64_t *gm_digest, uint64_t want, uint64_t **out_words, uint16_t **out_recs,
                          uint64_t *n_out) {
    o8pos rp;
    if (o8_decode(root_words, &rp)) { snprintf(o8_err, sizeof o8_err, "root words are no 8x8 position"); return -1; }
#ifdef _OPENMP
    const int T = threads > 0 ? threads : omp_get_max_threads();
#else
    const int T = 1;
    (void)threads;
#endif
    const int t0 = o8_tier(&rp);
    int err = 0, maxt = t0;
    o8seg *lay = (o8seg *)calloc((size_t)O8_TIERS * O8_NB, sizeof(o8seg));
    o8vec *pend = (o8vec *)calloc((size_t)O8_TIERS * O8_NB, sizeof(o8vec));
    o8vec *loc = (o8vec *)calloc((size_t)T * O8_SKIP * O8_NB, sizeof(o8vec));
    o8ent *all = NULL;
    if (!lay || !pend || !loc) { err = 1; goto done; }
    {
        o8key rk;
        memcpy(rk.w, root_words, sizeof rk.w);
        if (o8_push(&pend[(size_t)t0 * O8_NB + o8_bucket(rk.w)], &rk)) { err = 1; goto done; }
    }
    /* forward: a tier's buckets -> sorted distinct keys -> their children into deeper tiers */
    for (int t = t0; t <= maxt && !err; t++) {
        int bad = 0;
#pragma omp parallel num_threads(T) reduction(| : bad)
        {
#ifdef _OPENMP
            const int th = omp_get_thread_num();
#else
            const int th = 0;
#endif
            o8vec *mine = loc + (size_t)th * O8_SKIP * O8_NB;
#pragma omp for schedule(dynamic, 1)
            for (int b = 0; b < O8_NB; b++) {
                o8vec *pv = &pend[(size_t)t * O8_NB + b];
                o8seg *sg = &lay[(size_t)t * O8_NB + b];
                if (!pv->n) continue;
                qsort(pv->v, pv->n, sizeof(o8key), o8_cmp);
                uint64_t m = 0;
                for (uint64_t i = 0; i < pv->n; i++)
                    if (i == 0 || o8_cmp(&pv->v[i], &pv->v[i - 1])) pv->v[m++] = pv->v[i];
                sg->keys = (o8key *)realloc(pv->v, m * sizeof(o8key));
                if (!sg->keys) sg->keys = pv->v;
                sg->n = m;
                pv->v = NULL;
                pv->n = pv->cap = 0;
                sg->rec = (uint16_t *)malloc(m * sizeof(uint16_t));
                if (!sg->rec) { bad |= 1; continue; }
                for (uint64_t i = 0; i < m; i++) {
                    o8pos s, kids[64];
                    if (o8_decode(sg->keys[i].w, &s)) { bad |= 2; continue; }
                    if (o8_prim(&s) != UNDECIDED) continue;
                    const int nk = o8_kids(&s, kids);
                    for (int c = 0; c < nk; c++) {
                        o8key ck;
                        o8_encode(&kids[c], ck.w);
                        const int d = o8_tier(&kids[c]) - t;
                        if (d < 1 || d > O8_SKIP || t + d >= O8_TIERS) { bad |= 4; continue; }
                        if (o8_push(&mine[(size_t)(d - 1) * O8_NB + o8_bucket(ck.w)], &ck)) bad |= 1;
                    }
                }
            }
        }
        if (bad) {
            snprintf(o8_err, sizeof o8_err, "%s", (bad & 1) ? "out of memory" : (bad & 2) ? "invalid child" :
                     "tier not increasing by 1..3 along a move");
            err = 2;
            break;
        }
        for (int d = 1; d <= O8_SKIP && !err; d++)
            for (int b = 0; b < O8_NB && !err; b++) {
                uint64_t add = 0;
                for (int th = 0; th < T; th++) add += loc[((size_t)th * O8_SKIP + d - 1) * O8_NB + b].n;
                if (!add) continue;
                o8vec *q = &pend[(size_t)(t + d) * O8_NB + b];
                o8key *nv = (o8key *)realloc(q->v, (q->n + add) * sizeof(o8key));
                if (!nv) { err = 1; break; }
                q->v = nv;
                q->cap = q->n + add;
                for (int th = 0; th < T; th++) {
                    o8vec *src = &loc[((size_t)th * O8_SKIP + d - 1) * O8_NB + b];
                    if (src->n) memcpy(q->v + q->n, src->v, src->n * sizeof(o8key));
                    q->n += src->n;
                    src->n = 0;
                }
                if (t + d > maxt) maxt = t + d;
            }
    }
    if (err) goto done;
    /* backward: deepest tier first */
    for (int t = maxt; t >= t0 && !err; t--) {
        int bad = 0;
#pragma omp parallel for num_threads(T) schedule(dynamic, 1) reduction(| : bad)
        for (int b = 0; b < O8_NB; b++) {
            o8seg *sg = &lay[(size_t)t * O8_NB + b];
            for (uint64_t i = 0; i < sg->n; i++) {
                o8pos s, kids[64];
                o8_decode(sg->keys[i].w, &s);
                const int p = o8_prim(&s);
                if (p != UNDECIDED) { sg->rec[i] = (uint16_t)(p << 14); continue; }
                const int nk = o8_kids(&s, kids);
                uint32_t best = 0;
                for (int c = 0; c < nk; c++) {
                    o8key ck;
                    o8_encode(&kids[c], ck.w);
                    const o8seg *cs = &lay[(size_t)o8_tier(&kids[c]) * O8_NB + o8_bucket(ck.w)];
                    const int64_t j = o8_find(cs, &ck);
                    if (j < 0) { bad = 1; continue; }
                    const uint32_t sc = o8_pref(cs->rec[j]);
                    if (sc > best) best = sc;
                }
                sg->rec[i] = o8_from_pref(best);
            }
        }
        if (bad) { snprintf(o8_err, sizeof o8_err, "child missing from its tier"); err = 2; }
    }
    if (err) goto done;
    {
        uint64_t n = 0, wsum = 0, gsum = 0;
        for (int t = t0; t <= maxt; t++) {
            uint64_t nt = 0;
            for (int b = 0; b < O8_NB; b++) {
                const o8seg *sg = &lay[(size_t)t * O8_NB + b];
                uint64_t ws = 0, gs = 0;
#pragma omp parallel for num_threads(T) reduction(+ : ws, gs) schedule(static)
                for (long long i = 0; i < (long long)sg->n; i++) {
                    ws += o8_term(o8_fold(sg->keys[i].w), sg->rec[i]);
                    gs += o8_term(o8_device_word(sg->keys[i].w), sg->rec[i]);
                }
                wsum += ws;
                gsum += gs;
                nt += sg->n;
            }
            if (per_tier && t - t0 < per_tier_cap) per_tier[t - t0] = nt;
            n += nt;
        }
        *n_positions = n;
        *word_digest = wsum;
        *gm_digest = gsum;
        if (n_tiers) *n_tiers = maxt - t0 + 1;
        o8key rk;
        memcpy(rk.w, root_words, sizeof rk.w);
        const o8seg *rs = &lay[(size_t)t0 * O8_NB + o8_bucket(rk.w)];
        *root_record = rs->rec[o8_find(rs, &rk)];
        if (n_out) *n_out = 0;
        if (want && out_words && out_recs && n_out) {
            all = (o8ent *)malloc(n * sizeof(o8ent));
            if (!all) { err = 1; goto done; }
            uint64_t at = 0;
            for (int t = t0; t <= maxt; t++)
                for (int b = 0; b < O8_NB; b++) {
                    const o8seg *sg = &lay[(size_t)t * O8_NB + b];
                    for (uint64_t i = 0; i < sg->n; i++) {
                        all[at].k = sg->keys[i];
                        all[at++].rec = sg->rec[i];
                    }
                }
            qsort(all, n, sizeof(o8ent), o8_cmp);   /* the key is the entry's first member */
            const uint64_t m = want >= n ? n : want;
            *out_words = (uint64_t *)malloc(m * 3 * sizeof(uint64_t));
            *out_recs = (uint16_t *)malloc(m * sizeof(uint16_t));
            if (!*out_words || !*out_recs) {
                free(*out_words);
                free(*out_recs);
                *out_words = NULL;
                *out_recs = NULL;
                err = 1;
                goto done;
            }
            for (uint64_t i = 0; i < m; i++) {
                const uint64_t j = m == n ? i : (uint64_t)(((unsigned __int128)i * n) / m);
                memcpy(*out_words + 3 * i, all[j].k.w, 3 * sizeof(uint64_t));
                (*out_recs)[i] = all[j].rec;
            }
            *n_out = m;
        }
    }
done:
    if (err == 1) snprintf(o8_err, sizeof o8_err, "out of memory");
    free(all);
    if (lay)
        for (size_t i = 0; i < (size_t)O8_TIERS * O8_NB; i++) { free(lay[i].keys); free(lay[i].rec); }
    if (pend)
        for (size_t i = 0; i < (size_t)O8_TIERS * O8_NB; i++) free(pend[i].v);
    if (loc)
        for (size_t i = 0; i < (size_t)T * O8_SKIP * O8_NB; i++) free(loc[i].v);
    free(lay);
    free(pend);
    free(loc);
    return err ? -1 : 0;
}
