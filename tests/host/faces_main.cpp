// faces_main.cpp -- soda_hip_extend_faces_host in a program of its own, built
// by tests/test_border_faces.py together with soda_amd/csrc/soda_extend.cpp
// under -fsanitize=address,undefined and run directly: nothing is loaded into
// Python under a sanitizer.
//
// Every case plants cell values that name their own domain coordinates in an
// exactly sized heap array, spoils the ghost frame, refills it, and compares
// every cell with the rule of DESIGN.md 4.16 restated by stepping: below the
// domain the low face's mode, above it the high face's; a wrapped index walks
// back by whole periods, a mirrored one bounces off the walls one bounce at a
// time; a cell outside through constant faces takes the constant of the
// highest such dimension and of that face.
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
  return (T)(v % 241 + (sizeof(T) > 1 ? v * 256 : 0) + 1);
}

template <class T>
void one(int dim, const int32_t* n, const int32_t* lo, const int32_t* hi,
         const int32_t* mlo, const int32_t* mhi) {
  // eight constants no planted value equals (low bytes 0xF2 .. 0xF9, above
  // every value_of), with all their bytes in use
  uint64_t bits[8];
  for (int k = 0; k < 8; ++k)
    bits[k] = 0xF1E2D3C4B5A697F2ull + (uint64_t)k * 0x0101010101010001ull;
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
    int through = -1;                 // 2 * d + side of the highest constant
    for (int d = 0; d < dim; ++d) {
      c[d] = rest % p[d];
      rest /= p[d];
      const int64_t j = c[d] - lo[d];
      t[d] = step_map(j, n[d], j < 0 ? mlo[d] : mhi[d]);
      if (t[d] < 0) through = 2 * d + (j < 0 ? 0 : 1);
      if (j < 0 || j >= n[d]) ghost = true;
    }
    want[i] = through >= 0 ? (T)bits[through] : value_of<T>(t, n, dim);
    a[i] = ghost ? (T)~want[i] : want[i];
  }
  const int rc = soda_hip_extend_faces_host(a, (int32_t)sizeof(T), dim, n, lo,
                                            hi, mlo, mhi, bits);
  if (rc != SODA_HIP_OK || memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: %d-byte cells, %d-D, N0 = %d, ghosts %d / %d, faces %d/%d "
           "%d/%d %d/%d %d/%d (status %d)\n", (int)sizeof(T), dim, n[0], lo[0],
           hi[0], mlo[0], mhi[0], mlo[1], mhi[1], mlo[2], mhi[2], mlo[3],
           mhi[3], rc);
  }
  // a second fill changes nothing
  soda_hip_extend_faces_host(a, (int32_t)sizeof(T), dim, n, lo, hi, mlo, mhi,
                             bits);
  if (memcmp(a, want, (size_t)cells * sizeof(T))) {
    ++failures;
    printf("FAIL: a second fill changed the array\n");
  }
  // equal pairs and one constant: soda_hip_extend_host
  bool alike = true;
  for (int d = 0; d < dim; ++d) alike = alike && mlo[d] == mhi[d];
  if (alike) {
    uint64_t same[8];
    for (int k = 0; k < 8; ++k) same[k] = bits[3];
    memcpy(want, a, (size_t)cells * sizeof(T));
    soda_hip_extend_faces_host(a, (int32_t)sizeof(T), dim, n, lo, hi, mlo, mhi,
                               same);
    soda_hip_extend_host(want, (int32_t)sizeof(T), dim, n, lo, hi, mlo,
                         bits[3]);
    if (memcmp(a, want, (size_t)cells * sizeof(T))) {
      ++failures;
      printf("FAIL: equal pairs differ from soda_hip_extend_host\n");
    }
  }
  free(a);
  free(want);
}

void all_sizes(int dim, const int32_t* n, const int32_t* lo,
               const int32_t* hi, const int32_t* mlo, const int32_t* mhi) {
  one<uint8_t>(dim, n, lo, hi, mlo, mhi);
  one<uint16_t>(dim, n, lo, hi, mlo, mhi);
  one<uint32_t>(dim, n, lo, hi, mlo, mhi);
  one<uint64_t>(dim, n, lo, hi, mlo, mhi);
}

}  // namespace

int main() {
  int cases = 0;
  const int32_t extents[][4] = {{1, 1, 1, 1}, {2, 1, 2, 1}, {3, 5, 1, 2},
                                {7, 5, 3, 2}};
  const int32_t ghosts[][2][4] = {
      {{0, 0, 0, 0}, {0, 0, 0, 0}},      // no frame at all
      {{2, 1, 1, 1}, {2, 1, 1, 1}},      // symmetric
      {{3, 0, 2, 0}, {0, 2, 0, 1}},      // one-sided, alternating
      {{4, 6, 4, 4}, {7, 2, 4, 4}},      // wider than most of the domains
      {{9, 0, 0, 7}, {0, 11, 5, 0}},     // several bounces, one-sided
  };
  const int W = SODA_HIP_BORDER_WRAP, C = SODA_HIP_BORDER_CLAMP,
            M = SODA_HIP_BORDER_MIRROR, R = SODA_HIP_BORDER_MIRROR101,
            K = SODA_HIP_BORDER_CONSTANT;
  const int wall[4] = {C, M, R, K};
  // every pair of wall modes in dimension 0, rotated through the others
  for (int dim = 1; dim <= 4; ++dim)
    for (const auto& n : extents)
      for (const auto& g : ghosts)
        for (int a = 0; a < 4; ++a)
          for (int b = 0; b < 4; ++b) {
            const int32_t mlo[4] = {wall[a], wall[b], W, wall[(a + b) % 4]};
            const int32_t mhi[4] = {wall[b], wall[(a + 1) % 4], W,
                                    wall[(a + 2 * b + 1) % 4]};
            all_sizes(dim, n, g[0], g[1], mlo, mhi);
            cases += 4;
          }
  // equal pairs: soda_hip_extend_host
  const int32_t alike[][4] = {{W, W, W, W}, {K, K, K, K}, {K, M, W, C}};
  for (int dim = 1; dim <= 4; ++dim)
    for (const auto& n : extents)
      for (const auto& m : alike) {
        all_sizes(dim, n, ghosts[3][0], ghosts[3][1], m, m);
        cases += 4;
      }
  // refusals: nothing is touched
  uint32_t cell = 7;
  const uint64_t two[2] = {1, 2};
  const int32_t one_cell[1] = {1}, none[1] = {0}, neg[1] = {-1}, zero[1] = {0};
  const int32_t wrap[1] = {W}, clamp[1] = {C}, bad_lo[1] = {-1},
                bad_hi[1] = {5};
  auto refused = [&](int32_t elem, int32_t dim, const int32_t* n,
                     const int32_t* lo, const int32_t* mlo, const int32_t* mhi,
                     const uint64_t* c) {
    return soda_hip_extend_faces_host(&cell, elem, dim, n, lo, none, mlo, mhi,
                                      c) == SODA_HIP_ERR_INVALID;
  };
  if (!refused(3, 1, one_cell, none, wrap, wrap, two) ||
      !refused(4, 0, one_cell, none, wrap, wrap, two) ||
      !refused(4, 5, one_cell, none, wrap, wrap, two) ||
      !refused(4, 1, zero, none, wrap, wrap, two) ||
      !refused(4, 1, one_cell, neg, wrap, wrap, two) ||
      !refused(4, 1, one_cell, none, bad_lo, clamp, two) ||
      !refused(4, 1, one_cell, none, clamp, bad_hi, two) ||
      !refused(4, 1, one_cell, none, wrap, clamp, two) ||     // one-sided wrap
      !refused(4, 1, one_cell, none, clamp, wrap, two) ||
      !refused(4, 1, one_cell, none, clamp, nullptr, two) ||
      !refused(4, 1, one_cell, none, clamp, clamp, nullptr) ||
      soda_hip_extend_faces_host(nullptr, 4, 1, one_cell, none, none, clamp,
                                 clamp, two) != SODA_HIP_ERR_INVALID ||
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
