// box_main.cpp -- soda_hip_box_host in a program of its own, built by
// tests/test_border_fused.py together with soda_amd/csrc/soda_box.cpp under
// -fsanitize=address,undefined and run directly: nothing is loaded into
// Python under a sanitizer.
//
// Every case plants cell values that name their own coordinates in an exactly
// sized heap source, fills an exactly sized heap destination with a pattern,
// copies a list of boxes and compares every destination cell with what a
// cell-by-cell walk over the boxes says it holds.
#include "soda_hip.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace {

int failures = 0;

struct BoxList {
  int count;
  int32_t to[3][4], from[3][4], size[3][4];
};

template <class T>
T value_of(int64_t cell) {
  return (T)(cell % 251 + (sizeof(T) > 1 ? cell * 256 : 0) + 1);
}

template <class T>
void one(int dim, const int32_t* de, const int32_t* se, const BoxList& b) {
  int64_t dcells = 1, scells = 1;
  for (int d = 0; d < dim; ++d) {
    dcells *= de[d];
    scells *= se[d];
  }
  T* dst = static_cast<T*>(malloc((size_t)dcells * sizeof(T)));
  T* want = static_cast<T*>(malloc((size_t)dcells * sizeof(T)));
  T* src = static_cast<T*>(malloc((size_t)scells * sizeof(T)));
  if (!dst || !want || !src) abort();
  for (int64_t i = 0; i < scells; ++i) src[i] = value_of<T>(i);
  for (int64_t i = 0; i < dcells; ++i) dst[i] = want[i] = (T)0xA5A5A5A5A5A5A5A5ull;
  int32_t to[12], from[12], size[12];
  for (int k = 0; k < b.count; ++k) {
    int64_t cells = 1;
    for (int d = 0; d < dim; ++d) {
      to[k * dim + d] = b.to[k][d];
      from[k * dim + d] = b.from[k][d];
      size[k * dim + d] = b.size[k][d];
      cells *= b.size[k][d];
    }
    for (int64_t i = 0; i < cells; ++i) {
      int64_t rest = i, doff = 0, soff = 0, ds = 1, ss = 1;
      for (int d = 0; d < dim; ++d) {
        const int64_t c = rest % b.size[k][d];
        rest /= b.size[k][d];
        doff += (b.to[k][d] + c) * ds;
        soff += (b.from[k][d] + c) * ss;
        ds *= de[d];
        ss *= se[d];
      }
      want[doff] = src[soff];
    }
  }
  const int rc = soda_hip_box_host(dst, de, src, se, (int32_t)sizeof(T), dim,
                                   b.count, to, from, size);
  if (rc != SODA_HIP_OK || memcmp(dst, want, (size_t)dcells * sizeof(T))) {
    ++failures;
    printf("FAIL: %d-byte cells, %d-D, %d boxes (status %d)\n", (int)sizeof(T),
           dim, b.count, rc);
  }
  free(dst);
  free(want);
  free(src);
}

void all_sizes(int dim, const int32_t* de, const int32_t* se,
               const BoxList& b) {
  one<uint8_t>(dim, de, se, b);
  one<uint16_t>(dim, de, se, b);
  one<uint32_t>(dim, de, se, b);
  one<uint64_t>(dim, de, se, b);
}

}  // namespace

int main() {
  int cases = 0;
  const int32_t dext[][4] = {{9, 7, 5, 3}, {17, 4, 3, 2}, {5, 5, 5, 5}};
  const int32_t sext[][4] = {{11, 6, 4, 4}, {6, 9, 3, 2}, {5, 5, 5, 5}};
  const BoxList lists[] = {
      {0, {}, {}, {}},                                     // no box
      {1, {{0, 0, 0, 0}}, {{0, 0, 0, 0}}, {{5, 4, 3, 2}}},  // at the origins
      {1, {{4, 3, 2, 1}}, {{0, 2, 1, 0}}, {{1, 1, 1, 1}}},  // one cell, last
      {2, {{0, 0, 0, 0}, {3, 1, 1, 1}}, {{1, 1, 0, 0}, {2, 0, 1, 0}},
       {{3, 2, 2, 1}, {2, 3, 2, 1}}},                      // a gather's two
      {3, {{1, 0, 0, 0}, {0, 2, 0, 0}, {2, 0, 1, 1}},
       {{3, 1, 1, 1}, {0, 0, 0, 0}, {1, 1, 0, 0}},
       {{2, 2, 0, 1}, {0, 1, 1, 1}, {3, 2, 2, 1}}},        // two of them empty
  };
  for (int dim = 1; dim <= 4; ++dim)
    for (int e = 0; e < 3; ++e)
      for (const auto& b : lists) {
        all_sizes(dim, dext[e], sext[e], b);
        cases += 4;
      }
  // refusals: nothing is written
  uint32_t cells[4] = {1, 2, 3, 4}, out[4] = {9, 9, 9, 9};
  const int32_t four[1] = {4}, zero[1] = {0}, two[1] = {2}, three[1] = {3};
  const int32_t neg[1] = {-1}, none[1] = {0};
  if (soda_hip_box_host(out, four, cells, four, 3, 1, 1, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 0, 1, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 5, 1, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 1, -1, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 1, 1, three, zero, two) !=
          SODA_HIP_ERR_INVALID ||                       // leaves the destination
      soda_hip_box_host(out, four, cells, four, 4, 1, 1, zero, three, two) !=
          SODA_HIP_ERR_INVALID ||                       // leaves the source
      soda_hip_box_host(out, four, cells, four, 4, 1, 1, neg, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 1, 1, zero, zero, neg) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, none, cells, four, 4, 1, 0, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(out, four, cells, four, 4, 1, 1, nullptr, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      soda_hip_box_host(nullptr, four, cells, four, 4, 1, 1, zero, zero, two) !=
          SODA_HIP_ERR_INVALID ||
      out[0] != 9 || out[1] != 9 || out[2] != 9 || out[3] != 9) {
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
