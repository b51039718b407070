// wrap_main.cpp -- soda_hip_wrap_host in a program of its own, built by
// tests/test_periodic.py together with soda_amd/csrc/soda_wrap.cpp under
// -fsanitize=address,undefined and run directly: nothing is loaded into
// Python under a sanitizer.
//
// Every case plants cell values that name their own torus coordinates in an
// exactly sized heap array, spoils the ghost frame, refills it, and compares
// every cell with the closed form: the cell at padded index i holds the value
// of the torus cell reached by stepping i - ghost_lo back into [0, N) by
// whole periods (loops here, `%` in the code under test).
#include "soda_hip.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

int failures = 0;

int64_t into_torus(int64_t v, int64_t n) {
  while (v < 0) v += n;
  while (v >= n) v -= n;
  return v;
}

// the value of torus cell t: distinct per cell in every byte width for the
// extents below (a 1-byte cell keeps the low byte: still distinct mod 251)
template <class T>
T value_of(const int64_t* t, const int32_t* n, int dim) {
  int64_t v = 0;
  for (int d = dim - 1; d >= 0; --d) v = v * n[d] + t[d];
  return (T)(v % 251 + (sizeof(T) > 1 ? v * 256 : 0) + 1);
}

template <class T>
void one(int dim, const int32_t* n, const int32_t* lo, const int32_t* hi) {
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
    bool ghost = false;
    for (int d = 0; d < dim; ++d) {
      c[d] = rest % p[d];
      rest /= p[d];
      t[d] = into_torus(c[d] - lo[d], n[d]);
      if (c[d] < lo[d] || c[d] >= lo[d] + n[d]) ghost = true;
    }
    want[i] = value_of<T>(t, n, dim);
    a[i] = ghost ? (T)~want[i] : want[i];
  }
  const int rc = soda_hip_wrap_host(a, (int32_t)sizeof(T), dim, n, lo, hi);
  if (rc != SODA_HIP_OK || memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: %d-byte cells, %d-D, N0 = %d, ghosts %d / %d (status %d)\n",
           (int)sizeof(T), dim, n[0], lo[0], hi[0], rc);
  }
  // a second fill changes nothing
  soda_hip_wrap_host(a, (int32_t)sizeof(T), dim, n, lo, hi);
  if (memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: a second fill changed the array\n");
  }
  free(a);
  free(want);
}

void all_sizes(int dim, const int32_t* n, const int32_t* lo,
               const int32_t* hi) {
  one<uint8_t>(dim, n, lo, hi);
  one<uint16_t>(dim, n, lo, hi);
  one<uint32_t>(dim, n, lo, hi);
  one<uint64_t>(dim, n, lo, hi);
}

}  // namespace

int main() {
  int cases = 0;
  const int32_t extents[][4] = {{1, 1, 1, 1}, {3, 2, 1, 2}, {7, 5, 3, 2},
                                {12, 3, 4, 1}};
  const int32_t ghosts[][2][4] = {
      {{0, 0, 0, 0}, {0, 0, 0, 0}},      // no frame at all
      {{2, 1, 1, 1}, {2, 1, 1, 1}},      // symmetric
      {{3, 0, 2, 0}, {0, 2, 0, 1}},      // one-sided, alternating
      {{0, 4, 0, 3}, {5, 0, 1, 0}},
      {{4, 4, 4, 4}, {4, 4, 4, 4}},      // wider than most of the domains
      {{9, 0, 0, 7}, {0, 11, 5, 0}},     // several periods, one-sided
  };
  for (int dim = 1; dim <= 4; ++dim)
    for (const auto& n : extents)
      for (const auto& g : ghosts) {
        all_sizes(dim, n, g[0], g[1]);
        cases += 4;
      }
  // refusals: nothing is touched
  uint32_t cell = 7;
  const int32_t one_cell[1] = {1}, none[1] = {0}, neg[1] = {-1}, zero[1] = {0};
  if (soda_hip_wrap_host(&cell, 3, 1, one_cell, none, none) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_wrap_host(&cell, 4, 0, one_cell, none, none) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_wrap_host(&cell, 4, 5, one_cell, none, none) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_wrap_host(&cell, 4, 1, zero, none, none) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_wrap_host(&cell, 4, 1, one_cell, neg, none) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_wrap_host(nullptr, 4, 1, one_cell, none, none) !=
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
