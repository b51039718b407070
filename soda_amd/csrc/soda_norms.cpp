// soda_norms.cpp -- the host side of the exact L1 / L2 norms (DESIGN.md 4.10,
// include/soda_hip.h soda_hip_norms_t): fold, value, and the reduction itself
// in plain C++.  No HIP, no allocation, no global state: the file compiles
// with any host compiler on its own (tests/host/norms_main.cpp does).
#include "soda_hip.h"

#include <math.h>
#include <string.h>

namespace {

typedef unsigned __int128 u128;

// W[0, nw) += v[0, nv) << off; false if a bit or a carry leaves the words
bool add_at(uint64_t* W, int nw, const uint64_t* v, int nv, int off) {
  const int w = off / 64, r = off % 64;
  uint64_t carry = 0;
  for (int i = 0; i <= nv || carry; ++i) {
    uint64_t x = 0;
    if (i < nv) x = v[i] << r;
    if (r && i >= 1 && i <= nv) x |= v[i - 1] >> (64 - r);
    if (!x && !carry) continue;
    if (w + i >= nw) return false;
    const uint64_t old = W[w + i];
    const uint64_t sum = old + x;
    const uint64_t out = sum + carry;
    carry = (sum < old) || (out < sum) ? 1 : 0;
    W[w + i] = out;
  }
  return true;
}

// one cell's delta: its class, and for a finite one the integer m and the
// shift s with delta = m x 2^(s + u1) exactly
struct Term {
  int cls;        // 0 finite, 1 NaN, 2 +inf
  uint64_t m;
  int s;
};

Term term(float cur, float prev) {
  const float d = fabsf(cur - prev);
  Term t = {0, 0, 0};
  if (d != d) { t.cls = 1; return t; }
  uint32_t b;
  memcpy(&b, &d, sizeof b);
  const uint32_t e = b >> 23, f = b & 0x7fffffu;
  if (e == 0xff) { t.cls = 2; return t; }
  t.m = e ? (f | 0x800000u) : f;
  t.s = e ? (int)e - 1 : 0;
  return t;
}
Term term(double cur, double prev) {
  const double d = fabs(cur - prev);
  Term t = {0, 0, 0};
  if (d != d) { t.cls = 1; return t; }
  uint64_t b;
  memcpy(&b, &d, sizeof b);
  const uint64_t e = b >> 52, f = b & 0xfffffffffffffull;
  if (e == 0x7ff) { t.cls = 2; return t; }
  t.m = e ? (f | (1ull << 52)) : f;
  t.s = e ? (int)e - 1 : 0;
  return t;
}
template <class T>
Term term(T cur, T prev) {     // integers: the exact unsigned difference
  Term t = {0, 0, 0};
  t.m = cur > prev ? (uint64_t)cur - (uint64_t)prev
                   : (uint64_t)prev - (uint64_t)cur;
  if (sizeof(T) < 8) t.m &= 0xffffffffull;
  return t;
}

template <class T>
int reduce(const T* cur, const T* prev, int dim, const int32_t* extent,
           const int32_t* lo, const int32_t* hi, soda_hip_norms_t* acc) {
  int64_t e[4] = {1, 1, 1, 1}, l[4] = {0, 0, 0, 0}, h[4] = {1, 1, 1, 1};
  for (int d = 0; d < dim; ++d) {
    e[d] = extent[d];
    l[d] = lo[d];
    h[d] = hi[d];
    if (e[d] < 1 || l[d] < 0 || h[d] > e[d]) return SODA_HIP_ERR_INVALID;
  }
  for (int64_t q3 = l[3]; q3 < h[3]; ++q3)
    for (int64_t q2 = l[2]; q2 < h[2]; ++q2)
      for (int64_t q1 = l[1]; q1 < h[1]; ++q1) {
        const int64_t row = ((q3 * e[2] + q2) * e[1] + q1) * e[0];
        for (int64_t x = l[0]; x < h[0]; ++x) {
          const Term t = term(cur[row + x], prev[row + x]);
          if (t.cls == 1) { ++acc->unordered; continue; }
          if (t.cls == 2) { ++acc->infinite; continue; }
          ++acc->count;
          if (!t.m) continue;
          const u128 sq = (u128)t.m * t.m;
          const uint64_t sqw[2] = {(uint64_t)sq, (uint64_t)(sq >> 64)};
          if (!add_at(acc->l1, SODA_HIP_NORMS_L1_WORDS, &t.m, 1, t.s) ||
              !add_at(acc->l2, SODA_HIP_NORMS_L2_WORDS, sqw, 2, 2 * t.s))
            return SODA_HIP_ERR_INVALID;
        }
      }
  return SODA_HIP_OK;
}

bool bit(const uint64_t* W, int i) { return (W[i / 64] >> (i % 64)) & 1u; }

// the correctly rounded double of W[0, nw) x 2^u
double rounded(const uint64_t* W, int nw, int u) {
  int p = -1;                                  // index of the top bit
  for (int i = nw - 1; i >= 0 && p < 0; --i)
    if (W[i]) p = i * 64 + 63 - __builtin_clzll(W[i]);
  if (p < 0) return 0.0;
  if (p + u >= 1024) return INFINITY;
  // mantissa bits a double of this exponent holds: 53, fewer below 2^-1022
  int keep = p + u >= -1022 ? 53 : p + u + 1075;
  if (keep < 0) keep = -1;      // below half the least subnormal either way
  const int q = p + 1 - keep;   // low bits dropped
  uint64_t mant = 0;
  for (int i = p; i >= q && i >= 0; --i) mant = (mant << 1) | (bit(W, i) ? 1u : 0u);
  if (q <= 0) return ldexp((double)mant, u);   // every bit kept: exact
  const bool half = q - 1 <= p && bit(W, q - 1);
  bool sticky = false;
  for (int i = 0; i < q - 1 && !sticky;)       // (bits above p are zero)
    if (i % 64 == 0 && i + 64 <= q - 1) {
      sticky = W[i / 64] != 0;
      i += 64;
    } else {
      sticky = bit(W, i);
      ++i;
    }
  if (half && (sticky || (mant & 1u))) ++mant;
  return ldexp((double)mant, q + u);          // exact; inf above the range
}

void units(uint32_t kind, int* u1, int* u2) {
  *u1 = kind == SODA_HIP_NORMS_F32 ? -149 : kind == SODA_HIP_NORMS_F64 ? -1074 : 0;
  *u2 = 2 * *u1;
}

bool known(uint32_t kind) {
  return kind >= SODA_HIP_NORMS_F32 && kind <= SODA_HIP_NORMS_I64;
}

}  // namespace

extern "C" {

int soda_hip_norms_kind_of(int32_t cell, int32_t* elem) {
  static const int kind[10] = {
      SODA_HIP_NORMS_F32, SODA_HIP_NORMS_F64, SODA_HIP_NORMS_I32,
      SODA_HIP_NORMS_I32, SODA_HIP_NORMS_I32, SODA_HIP_NORMS_I32,
      SODA_HIP_NORMS_I32, SODA_HIP_NORMS_I32, SODA_HIP_NORMS_I64,
      SODA_HIP_NORMS_I64};
  static const int size[10] = {4, 8, 1, 1, 2, 2, 4, 4, 8, 8};
  if (cell < 0 || cell > 9) return 0;
  if (elem) *elem = size[cell];
  return kind[cell];
}

int soda_hip_norms_fold(soda_hip_norms_t* dst, const soda_hip_norms_t* src) {
  if (!dst || !src || dst->kind != src->kind || !known(dst->kind))
    return SODA_HIP_ERR_INVALID;
  dst->count += src->count;
  dst->unordered += src->unordered;
  dst->infinite += src->infinite;
  if (!add_at(dst->l1, SODA_HIP_NORMS_L1_WORDS, src->l1,
              SODA_HIP_NORMS_L1_WORDS, 0) ||
      !add_at(dst->l2, SODA_HIP_NORMS_L2_WORDS, src->l2,
              SODA_HIP_NORMS_L2_WORDS, 0))
    return SODA_HIP_ERR_INVALID;
  return SODA_HIP_OK;
}

int soda_hip_norms_value(const soda_hip_norms_t* acc, int32_t which,
                         double* out) {
  if (!acc || !out || !known(acc->kind) ||
      (which != SODA_HIP_NORMS_WHICH_L1 && which != SODA_HIP_NORMS_WHICH_L2))
    return SODA_HIP_ERR_INVALID;
  int u1, u2;
  units(acc->kind, &u1, &u2);
  if (acc->infinite)
    *out = INFINITY;
  else if (which == SODA_HIP_NORMS_WHICH_L1)
    *out = rounded(acc->l1, SODA_HIP_NORMS_L1_WORDS, u1);
  else
    *out = rounded(acc->l2, SODA_HIP_NORMS_L2_WORDS, u2);
  return SODA_HIP_OK;
}

int soda_hip_norms_host(const void* cur, const void* prev, int32_t cell,
                        int32_t dim, const int32_t* extent, const int32_t* lo,
                        const int32_t* hi, soda_hip_norms_t* acc) {
  if (!cur || !prev || !extent || !lo || !hi || !acc || dim < 1 ||
      dim > SODA_HIP_MAX_DIM)
    return SODA_HIP_ERR_INVALID;
  const int kind = soda_hip_norms_kind_of(cell, nullptr);
  if (!kind || acc->kind != (uint32_t)kind) return SODA_HIP_ERR_INVALID;
#define SODA_NORMS_CASE(C, T)                                              \
  case C:                                                                  \
    return reduce(static_cast<const T*>(cur), static_cast<const T*>(prev), \
                  dim, extent, lo, hi, acc);
  switch (cell) {
    SODA_NORMS_CASE(SODA_HIP_CELL_FLOAT, float)
    SODA_NORMS_CASE(SODA_HIP_CELL_DOUBLE, double)
    SODA_NORMS_CASE(SODA_HIP_CELL_INT8, int8_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_UINT8, uint8_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_INT16, int16_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_UINT16, uint16_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_INT32, int32_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_UINT32, uint32_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_INT64, int64_t)
    SODA_NORMS_CASE(SODA_HIP_CELL_UINT64, uint64_t)
  }
#undef SODA_NORMS_CASE
  return SODA_HIP_ERR_INVALID;
}

}  // extern "C"
