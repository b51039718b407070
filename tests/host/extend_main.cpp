// extend_main.cpp -- soda_hip_extend_host in a program of its own, built by
// tests/test_border.py together with soda_amd/csrc/soda_extend.cpp under
// -fsanitize=address,undefined and run directly: nothing is loaded into
// Python under a sanitizer.
//
// Every case plants cell values that name their own domain coordinates in an
// exactly sized heap array, spoils the ghost frame, refills it, and compares
// every cell with the closed form of its mode per dimension.  The closed forms
// are restated here by stepping: a wrapped index walks back by whole periods,
// a mirrored one bounces off the walls one bounce at a time (loops here, `%`
// in the code under test).
#include "soda_hip.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

int failures = 0;

// the cell of [0, n) index j takes; -1: the constant
int64_t step_map(int64_t j, int64_t n, int mode) {
  switch (mode) {
    case SODA_HIP_BORDER_WRAP:
      while (j < 0) j += n;
      while (j >= n) j -= n;
      return j;
    case SODA_HIP_BORDER_CLAMP:
      return j < 0 ? 0 : j >= n ? n - 1 : j;
    case SODA_HIP_BORDER_MIRROR:       // the wall lies between two cells
      while (j < 0 || j >= n) j = j < 0 ? -1 - j : 2 * n - 1 - j;
      return j;
    case SODA_HIP_BORDER_MIRROR101:    // the wall lies on a cell
      if (n == 1) return 0;
      while (j < 0 || j >= n) j = j < 0 ? -j : 2 * n - 2 - j;
      return j;
    default:
      return j < 0 || j >= n ? -1 : j;
  }
}

template <class T>
T value_of(const int64_t* t, const int32_t* n, int dim) {
  int64_t v = 0;
  for (int d = dim - 1; d >= 0; --d) v = v * n[d] + t[d];
  return (T)(v % 251 + (sizeof(T) > 1 ? v * 256 : 0) + 1);
}

template <class T>
void one(int dim, const int32_t* n, const int32_t* lo, const int32_t* hi,
         const int32_t* mode) {
  // a constant no planted value equals, with all its bytes in use
  const uint64_t bits = 0xF1E2D3C4B5A69788ull;
  const T cst = (T)bits;
  int64_t p[4] = {1, 1, 1, 1}, cells = 1;
  for (int d = 0; d < dim; ++d) {
    p[d] = (int64_t)lo[d] + n[d] + hi[d];
    cells *= p[d];
  }
  T* a = static_cast<T*>(malloc((size_t)cells * sizeof(T)));
  T* want = static_cast<T*>(malloc((size_t)cells * sizeof(T)));
  if (!a || !want) abort();
  for (int64_t i = 0; i < cells; ++i) {
    int64_t c[4], t[4], rest = i;
    bool ghost = false, outside = false;
    for (int d = 0; d < dim; ++d) {
      c[d] = rest % p[d];
      rest /= p[d];
      t[d] = step_map(c[d] - lo[d], n[d], mode[d]);
      if (t[d] < 0) outside = true;
      if (c[d] < lo[d] || c[d] >= lo[d] + n[d]) ghost = true;
    }
    want[i] = outside ? cst : value_of<T>(t, n, dim);
    a[i] = ghost ? (T)~want[i] : want[i];
  }
  const int rc = soda_hip_extend_host(a, (int32_t)sizeof(T), dim, n, lo, hi,
                                      mode, bits);
  if (rc != SODA_HIP_OK || memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: %d-byte cells, %d-D, N0 = %d, ghosts %d / %d, modes %d %d %d "
           "%d (status %d)\n", (int)sizeof(T), dim, n[0], lo[0], hi[0],
           mode[0], mode[1], mode[2], mode[3], rc);
  }
  // a second fill changes nothing
  soda_hip_extend_host(a, (int32_t)sizeof(T), dim, n, lo, hi, mode, bits);
  if (memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: a second fill changed the array\n");
  }
  free(a);
  free(want);
}

void all_sizes(int dim, const int32_t* n, const int32_t* lo,
               const int32_t* hi, const int32_t* mode) {
  one<uint8_t>(dim, n, lo, hi, mode);
  one<uint16_t>(dim, n, lo, hi, mode);
  one<uint32_t>(dim, n, lo, hi, mode);
  one<uint64_t>(dim, n, lo, hi, mode);
}

}  // namespace

int main() {
  int cases = 0;
  const int32_t extents[][4] = {{1, 1, 1, 1}, {2, 1, 2, 1}, {3, 2, 1, 2},
                                {7, 5, 3, 2}};
  const int32_t ghosts[][2][4] = {
      {{0, 0, 0, 0}, {0, 0, 0, 0}},      // no frame at all
      {{2, 1, 1, 1}, {2, 1, 1, 1}},      // symmetric
      {{3, 0, 2, 0}, {0, 2, 0, 1}},      // one-sided, alternating
      {{4, 4, 4, 4}, {4, 4, 4, 4}},      // wider than most of the domains
      {{9, 0, 0, 7}, {0, 11, 5, 0}},     // several bounces, one-sided
  };
  const int W = SODA_HIP_BORDER_WRAP, C = SODA_HIP_BORDER_CLAMP,
            M = SODA_HIP_BORDER_MIRROR, R = SODA_HIP_BORDER_MIRROR101,
            K = SODA_HIP_BORDER_CONSTANT;
  const int32_t modes[][4] = {{W, W, W, W}, {C, C, C, C}, {M, M, M, M},
                              {R, R, R, R}, {K, K, K, K}, {W, C, M, R},
                              {K, M, K, C}, {R, K, W, K}, {M, W, C, K}};
  for (int dim = 1; dim <= 4; ++dim)
    for (const auto& n : extents)
      for (const auto& g : ghosts)
        for (const auto& m : modes) {
          all_sizes(dim, n, g[0], g[1], m);
          cases += 4;
        }
  // refusals: nothing is touched
  uint32_t cell = 7;
  const int32_t one_cell[1] = {1}, none[1] = {0}, neg[1] = {-1}, zero[1] = {0};
  const int32_t wrap[1] = {W}, bad_lo[1] = {-1}, bad_hi[1] = {5};
  if (soda_hip_extend_host(&cell, 3, 1, one_cell, none, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 0, one_cell, none, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 5, one_cell, none, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 1, zero, none, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 1, one_cell, neg, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 1, one_cell, none, none, bad_lo, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 1, one_cell, none, none, bad_hi, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(&cell, 4, 1, one_cell, none, none, nullptr, 0) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_extend_host(nullptr, 4, 1, one_cell, none, none, wrap, 0) !=
          SODA_HIP_ERR_INVALID ||
      cell != 7) {
    ++failures;
    printf("FAIL: a bad argument was not refused\n");
  }
  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("OK %d cases\n", cases);
  return 0;
}
