// The host side of the exact norms (soda_hip_norms_fold / _value / _host) in a
// program of its own: closed forms only, no Python, no GPU, no HIP.  Built by
// tests/test_norms.py together with soda_amd/csrc/soda_norms.cpp under
// -fsanitize=address,undefined; every array is a heap block of exactly the
// size the call is told, so a read past a row or a word shows.
#include "soda_hip.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      ++failures;                                                      \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);            \
    }                                                                  \
  } while (0)

static soda_hip_norms_t fresh(int kind) {
  soda_hip_norms_t a;
  std::memset(&a, 0, sizeof a);
  a.kind = (uint32_t)kind;
  return a;
}

template <class T>
static soda_hip_norms_t line(int cell, const std::vector<T>& cur,
                             const std::vector<T>& prev, int lo, int hi,
                             int* status = nullptr) {
  soda_hip_norms_t a = fresh(soda_hip_norms_kind_of(cell, nullptr));
  // exact-size copies: the sanitizer sees any read outside them
  T* c = new T[cur.size()];
  T* p = new T[prev.size()];
  std::memcpy(c, cur.data(), cur.size() * sizeof(T));
  std::memcpy(p, prev.data(), prev.size() * sizeof(T));
  const int32_t ext[1] = {(int32_t)cur.size()}, l[1] = {lo}, h[1] = {hi};
  const int rc = soda_hip_norms_host(c, p, cell, 1, ext, l, h, &a);
  if (status) *status = rc; else EXPECT(rc == SODA_HIP_OK);
  delete[] c;
  delete[] p;
  return a;
}

static double value(const soda_hip_norms_t& a, int which) {
  double v = -1.0;
  EXPECT(soda_hip_norms_value(&a, which, &v) == SODA_HIP_OK);
  return v;
}

static bool rest_zero(const uint64_t* w, int from, int n) {
  for (int i = from; i < n; ++i)
    if (w[i]) return false;
  return true;
}

int main() {
  const int L1 = SODA_HIP_NORMS_WHICH_L1, L2 = SODA_HIP_NORMS_WHICH_L2;
  EXPECT(sizeof(soda_hip_norms_t) == 8 * (4 + 34 + 67));
  int32_t elem = 0;
  EXPECT(soda_hip_norms_kind_of(SODA_HIP_CELL_UINT16, &elem) ==
             SODA_HIP_NORMS_I32 && elem == 2);
  EXPECT(soda_hip_norms_kind_of(10, nullptr) == 0);

  {  // two fp32 deltas of 2^-86: 2^64 units of 2^-149, 2^127 of 2^-298
    const float d = std::ldexp(1.0f, -86);
    soda_hip_norms_t a = line<float>(SODA_HIP_CELL_FLOAT, {d, 0.f, d},
                                     {0.f, 0.f, 0.f}, 0, 3);
    EXPECT(a.count == 3 && a.unordered == 0 && a.infinite == 0);
    EXPECT(a.l1[0] == 0 && a.l1[1] == 1 && rest_zero(a.l1, 2, 34));
    EXPECT(a.l2[0] == 0 && a.l2[1] == 1ull << 63 && rest_zero(a.l2, 2, 67));
    EXPECT(value(a, L1) == std::ldexp(1.0, -85));
    EXPECT(value(a, L2) == std::ldexp(1.0, -171));
  }
  {  // 4096 x 0x1.fffffep-86f: (2^24 - 1) x 2^52 units = 2^76 - 2^52
    std::vector<float> cur(4096, 0x1.fffffep-86f), prev(4096, 0.f);
    soda_hip_norms_t a = line<float>(SODA_HIP_CELL_FLOAT, cur, prev, 0, 4096);
    EXPECT(a.l1[0] == 0ull - (1ull << 52) && a.l1[1] == 4095 &&
           rest_zero(a.l1, 2, 34));
    // squares: (2^24 - 1)^2 x 2^80 x 2^12 = 2^140 - 2^117 + 2^92
    EXPECT(a.l2[0] == 0 && a.l2[1] == (0ull - (1ull << 53)) + (1ull << 28) &&
           a.l2[2] == (1ull << 12) - 1 && rest_zero(a.l2, 3, 67));
  }
  {  // 300 uint64 deltas of 2^64 - 1
    std::vector<uint64_t> cur(300, ~0ull), prev(300, 0ull);
    prev[7] = ~0ull;
    cur[7] = 0ull;                     // either way round
    soda_hip_norms_t a =
        line<uint64_t>(SODA_HIP_CELL_UINT64, cur, prev, 0, 300);
    EXPECT(a.count == 300);
    EXPECT(a.l1[0] == 0ull - 300 && a.l1[1] == 299 && rest_zero(a.l1, 2, 34));
    EXPECT(a.l2[0] == 300 && a.l2[1] == 0ull - 600 && a.l2[2] == 299 &&
           rest_zero(a.l2, 3, 67));
    EXPECT(value(a, L1) == 300.0 * 18446744073709551616.0);
  }
  {  // int8 extremes, int64 extremes, the box cuts
    soda_hip_norms_t a = line<int8_t>(SODA_HIP_CELL_INT8, {-128, 127, 5, 9},
                                      {127, -128, 5, 100}, 0, 3);
    EXPECT(a.count == 3 && a.l1[0] == 510 && a.l2[0] == 2 * 255 * 255);
    soda_hip_norms_t b = line<int64_t>(
        SODA_HIP_CELL_INT64,
        {std::numeric_limits<int64_t>::min(), 3},
        {std::numeric_limits<int64_t>::max(), 3}, 0, 2);
    EXPECT(b.count == 2 && b.l1[0] == ~0ull && b.l1[1] == 0);
    EXPECT(b.l2[0] == 1 && b.l2[1] == ~0ull - 1 && b.l2[2] == 0);
    soda_hip_norms_t c = line<uint16_t>(SODA_HIP_CELL_UINT16, {0, 65535, 1},
                                        {65535, 0, 1}, 1, 2);
    EXPECT(c.count == 1 && c.l1[0] == 65535);
  }
  {  // NaN, both infinities, both zeros, a subnormal
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    soda_hip_norms_t a = line<float>(
        SODA_HIP_CELL_FLOAT, {nan, inf, inf, 0.0f, 1e-45f, -inf, 2.f},
        {1.f, inf, -inf, -0.0f, 0.f, 3.f, 1.f}, 0, 7);
    EXPECT(a.unordered == 2 && a.infinite == 2 && a.count == 3);
    EXPECT(a.l1[0] == 1 && a.l1[2] == 1ull << 21);   // 2^-149 and 1 = 2^149
    EXPECT(value(a, L1) == INFINITY && value(a, L2) == INFINITY);
    a.infinite = 0;
    EXPECT(value(a, L1) == 1.0 && value(a, L2) == 1.0);   // 1 + 2^-149 rounds
  }
  {  // rounding: ties to even, the double range, the subnormal range
    soda_hip_norms_t a = fresh(SODA_HIP_NORMS_I64);
    a.l1[0] = (1ull << 53) + 1;
    EXPECT(value(a, L1) == 9007199254740992.0);          // tie: down to even
    a.l1[0] = (1ull << 53) + 3;
    EXPECT(value(a, L1) == 9007199254740996.0);          // tie: up to even
    a.l1[0] = (1ull << 53) + 1;
    a.l2[0] = 0;
    a.l1[1] = 0;
    a.l2[5] = 1;
    a.l2[0] = 1;                                         // 2^320 + 1: sticky
    EXPECT(value(a, L2) == std::ldexp(1.0, 320));
    a.l2[4] = 1ull << 11;                                // half an ulp + sticky
    EXPECT(value(a, L2) == std::ldexp(1.0, 320) + std::ldexp(1.0, 268));
    a.l2[0] = 0;                                         // exactly half: even
    EXPECT(value(a, L2) == std::ldexp(1.0, 320));
    std::vector<double> big(2, DBL_MAX), zero(2, 0.0);
    soda_hip_norms_t one = line<double>(SODA_HIP_CELL_DOUBLE, big, zero, 0, 1);
    EXPECT(value(one, L1) == DBL_MAX && value(one, L2) == INFINITY);
    soda_hip_norms_t two = line<double>(SODA_HIP_CELL_DOUBLE, big, zero, 0, 2);
    EXPECT(two.infinite == 0 && value(two, L1) == INFINITY);
    // squares of subnormal-range values: below 2^-1074 they round at the
    // least subnormal, not at 53 bits
    std::vector<double> tiny = {std::ldexp(1.0, -537), std::ldexp(1.5, -538),
                                std::ldexp(1.0, -540)};
    std::vector<double> none(3, 0.0);
    soda_hip_norms_t t = line<double>(SODA_HIP_CELL_DOUBLE, tiny, none, 0, 1);
    EXPECT(value(t, L2) == std::ldexp(1.0, -1074));
    t = line<double>(SODA_HIP_CELL_DOUBLE, tiny, none, 1, 2);
    // 2.25 x 2^-1076 = 0.5625 x 2^-1074: above half, up
    EXPECT(value(t, L2) == std::ldexp(1.0, -1074));
    t = line<double>(SODA_HIP_CELL_DOUBLE, tiny, none, 2, 3);
    EXPECT(value(t, L2) == 0.0);                         // 2^-1080: down
    t = fresh(SODA_HIP_NORMS_F64);
    t.l2[16] = 1ull << 49;                               // 2^1073 units: 2^-1075
    EXPECT(value(t, L2) == 0.0);                         // the tie goes to even
    t.l2[0] = 1;
    EXPECT(value(t, L2) == std::ldexp(1.0, -1074));
  }
  {  // fold: bands of a 2-D grid add up to the whole; kinds must match
    const int w = 37, h = 11;
    std::vector<float> cur(w * h), prev(w * h);
    for (int i = 0; i < w * h; ++i) {
      cur[i] = std::ldexp((float)(i % 29 + 1), (i * 7) % 90 - 60);
      prev[i] = (float)(i % 5) * 0.25f;
    }
    const int32_t ext[2] = {w, h};
    soda_hip_norms_t whole = fresh(SODA_HIP_NORMS_F32);
    const int32_t lo[2] = {2, 1}, hi[2] = {w - 3, h - 1};
    EXPECT(soda_hip_norms_host(cur.data(), prev.data(), SODA_HIP_CELL_FLOAT, 2,
                               ext, lo, hi, &whole) == SODA_HIP_OK);
    soda_hip_norms_t sum = fresh(SODA_HIP_NORMS_F32);
    for (int y = 1; y < h - 1; y += 3) {
      soda_hip_norms_t band = fresh(SODA_HIP_NORMS_F32);
      const int32_t blo[2] = {2, y}, bhi[2] = {w - 3, y + 3 < h - 1 ? y + 3 : h - 1};
      EXPECT(soda_hip_norms_host(cur.data(), prev.data(), SODA_HIP_CELL_FLOAT,
                                 2, ext, blo, bhi, &band) == SODA_HIP_OK);
      EXPECT(soda_hip_norms_fold(&sum, &band) == SODA_HIP_OK);
    }
    EXPECT(std::memcmp(&sum, &whole, sizeof sum) == 0);
    EXPECT(whole.count == (uint64_t)(w - 5) * (h - 2));
    soda_hip_norms_t other = fresh(SODA_HIP_NORMS_F64);
    EXPECT(soda_hip_norms_fold(&sum, &other) == SODA_HIP_ERR_INVALID);
    soda_hip_norms_t never = fresh(0);
    EXPECT(soda_hip_norms_fold(&never, &never) == SODA_HIP_ERR_INVALID);
    // a carry out of the last word is refused, not dropped
    soda_hip_norms_t full = fresh(SODA_HIP_NORMS_F64);
    full.l1[33] = ~0ull;
    soda_hip_norms_t bit = fresh(SODA_HIP_NORMS_F64);
    bit.l1[33] = 1;
    EXPECT(soda_hip_norms_fold(&full, &bit) == SODA_HIP_ERR_INVALID);
  }
  {  // refusals of the reduction
    int rc = 0;
    line<float>(SODA_HIP_CELL_FLOAT, {1.f, 2.f}, {0.f, 0.f}, 0, 3, &rc);
    EXPECT(rc == SODA_HIP_ERR_INVALID);
    line<float>(SODA_HIP_CELL_FLOAT, {1.f, 2.f}, {0.f, 0.f}, -1, 2, &rc);
    EXPECT(rc == SODA_HIP_ERR_INVALID);
    soda_hip_norms_t a = fresh(SODA_HIP_NORMS_F64);
    const float c[1] = {1.f};
    const int32_t ext[1] = {1}, lo[1] = {0}, hi[1] = {1};
    EXPECT(soda_hip_norms_host(c, c, SODA_HIP_CELL_FLOAT, 1, ext, lo, hi, &a) ==
           SODA_HIP_ERR_INVALID);                        // kind of another type
    soda_hip_norms_t e = line<float>(SODA_HIP_CELL_FLOAT, {1.f, 2.f},
                                     {0.f, 0.f}, 1, 1);  // empty box
    EXPECT(e.count == 0 && rest_zero(e.l1, 0, 34));
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK norms host\n");
  return 0;
}
