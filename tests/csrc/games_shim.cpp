// games_shim.cpp -- array versions of the symmetry hooks and rules of DescOthello and DescToot
// (gamesmanmpi_amd/csrc/games.hpp) for tests/test_symmetry_algebra.py.  Compiled by the test,
// host-only, with ROCm's clang (GM_HD is plain `inline` there; games.hpp needs
// __builtin_bitreverse32) and loaded with ctypes.  Every call takes arrays in and arrays out;
// `sym` is the descriptor's symmetry mask for that call.
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#include "games.hpp"

namespace {

gm::DescOthello oth(int L, uint32_t sym) {
    gm::DescOthello d{};
    if (!gm::DescOthello::make(L, L, &d)) __builtin_trap();
    d.sym = sym;
    return d;
}

gm::DescToot toot(int L, int H, uint32_t sym) {
    gm::DescToot d{};
    if (!gm::DescToot::make(L, H, &d)) __builtin_trap();
    d.sym = sym;
    return d;
}

}  // namespace

extern "C" {

// 1 when make(L, H) accepts the board
int shim_oth_make(int L, int H) {
    gm::DescOthello d{};
    return gm::DescOthello::make(L, H, &d) ? 1 : 0;
}

int shim_toot_make(int L, int H) {
    gm::DescToot d{};
    return gm::DescToot::make(L, H, &d) ? 1 : 0;
}

// ---------------------------------------------------------------- Othello
void shim_oth_xform_plane4(const uint32_t *p, int g, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::DescOthello::xform_plane4(p[i], g);
}

void shim_oth_xform_plane_cells(int L, const uint32_t *p, int g, uint32_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.xform_plane_cells(p[i], g);
}

void shim_oth_xform(int L, const uint64_t *k, int g, uint64_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.xform(k[i], g);
}

void shim_oth_canon(int L, uint32_t sym, const uint64_t *k, uint64_t *out, size_t n) {
    const gm::DescOthello d = oth(L, sym);
    for (size_t i = 0; i < n; i++) out[i] = d.canon(k[i]);
}

void shim_oth_stabilizer(int L, const uint64_t *k, uint32_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.stabilizer(k[i]);
}

// out: 16 slots per key (orbit() promises at most 8; a broken one may not keep that), cnt: how
// many orbit() gave
void shim_oth_orbit(int L, uint32_t sym, const uint64_t *k, uint64_t *out, int32_t *cnt, size_t n) {
    const gm::DescOthello d = oth(L, sym);
    for (size_t i = 0; i < n; i++) {
        int m = 0;
        d.orbit(k[i], [&](uint64_t t) {
            if (m < 16) out[16 * i + m] = t;
            m++;
        });
        cnt[i] = m;
    }
}

// out: MAXC slots per key
void shim_oth_children(int L, uint32_t sym, const uint64_t *k, uint64_t *out, int32_t *cnt, size_t n) {
    const gm::DescOthello d = oth(L, sym);
    for (size_t i = 0; i < n; i++) cnt[i] = d.children(k[i], out + (size_t)gm::DescOthello::MAXC * i);
}

// out: MAXC slots per key, in the order visit_part() gives them; cnt: its return value
void shim_oth_visit_part(int L, uint32_t sym, int part, int nparts, const uint64_t *k, uint64_t *out,
                         int32_t *cnt, size_t n) {
    const gm::DescOthello d = oth(L, sym);
    for (size_t i = 0; i < n; i++) {
        uint64_t *o = out + (size_t)gm::DescOthello::MAXC * i;
        int m = 0;
        const int r = d.visit_part(k[i], part, nparts, [&](uint64_t c) {
            o[m++] = c;
            return true;
        });
        cnt[i] = r == m ? r : -1;
    }
}

void shim_oth_pass_child(int L, uint32_t sym, const uint64_t *k, uint64_t *out, size_t n) {
    const gm::DescOthello d = oth(L, sym);
    for (size_t i = 0; i < n; i++) out[i] = d.pass_child(k[i]);
}

void shim_oth_primitive(int L, const uint64_t *k, int32_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.primitive(k[i]);
}

void shim_oth_tier(int L, const uint64_t *k, int64_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.tier(k[i]);
}

void shim_oth_valid(int L, const uint64_t *k, uint8_t *out, size_t n) {
    const gm::DescOthello d = oth(L, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.valid(k[i]) ? 1 : 0;
}

// ---------------------------------------------------------------- Toot-and-Otto
void shim_toot_mirror_plane(int L, int H, const uint32_t *p, uint32_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.mirror_plane(p[i]);
}

void shim_toot_mirror(int L, int H, const uint64_t *k, uint64_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.mirror(k[i]);
}

void shim_toot_canon(int L, int H, uint32_t sym, const uint64_t *k, uint64_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, sym);
    for (size_t i = 0; i < n; i++) out[i] = d.canon(k[i]);
}

// out: 4 slots per key (orbit() promises at most 2), cnt: how many orbit() gave
void shim_toot_orbit(int L, int H, uint32_t sym, const uint64_t *k, uint64_t *out, int32_t *cnt, size_t n) {
    const gm::DescToot d = toot(L, H, sym);
    for (size_t i = 0; i < n; i++) {
        int m = 0;
        d.orbit(k[i], [&](uint64_t t) {
            if (m < 4) out[4 * i + m] = t;
            m++;
        });
        cnt[i] = m;
    }
}

// out: MAXC slots per key
void shim_toot_children(int L, int H, uint32_t sym, const uint64_t *k, uint64_t *out, int32_t *cnt, size_t n) {
    const gm::DescToot d = toot(L, H, sym);
    for (size_t i = 0; i < n; i++) cnt[i] = d.children(k[i], out + (size_t)gm::DescToot::MAXC * i);
}

void shim_toot_primitive(int L, int H, const uint64_t *k, int32_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.primitive(k[i]);
}

void shim_toot_tier(int L, int H, const uint64_t *k, int64_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.tier(k[i]);
}

void shim_toot_valid(int L, int H, const uint64_t *k, uint8_t *out, size_t n) {
    const gm::DescToot d = toot(L, H, 0);
    for (size_t i = 0; i < n; i++) out[i] = d.valid(k[i]) ? 1 : 0;
}

}  // extern "C"
