// score_shim.cpp -- array versions of the record / preference-score functions of
// gamesmanmpi_amd/csrc/gm_common.hpp for tests/test_score_algebra.py.  Compiled by the test
// with the host C++ compiler (GM_HD is plain `inline` there) and loaded with ctypes.
#include "gm_common.hpp"

#include <stddef.h>

extern "C" {

void shim_score_of_primitive(const int32_t *v, uint16_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::score_of_primitive(v[i]);
}

void shim_parent_score(const uint32_t *b, uint16_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::parent_score(b[i]);
}

void shim_record_of_score(const uint16_t *s, uint16_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::record_of_score(s[i]);
}

void shim_score_of_record(const uint16_t *r, uint16_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::score_of_record(r[i]);
}

void shim_score_overflows(const uint32_t *b, uint8_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::score_overflows(b[i]) ? 1 : 0;
}

void shim_parent_code(const uint32_t *b, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::parent_code(b[i]);
}

void shim_record_of_code(const uint8_t *b, uint16_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) out[i] = gm::record_of_code(b[i]);
}

}  // extern "C"
