// soda_wrap.cpp -- the host twin of the wrap kernels (DESIGN.md 4.11,
// include/soda_hip.h soda_hip_wrap_host): the ghost frame of a padded host
// array refilled from its interior, in plain C++.  No HIP, no allocation, no
// global state: the file compiles with any host compiler on its own
// (tests/host/wrap_main.cpp does).
#include "soda_hip.h"

#include <string.h>

namespace {

int64_t wrap(int64_t v, int64_t n) {
  const int64_t m = v % n;
  return m < 0 ? m + n : m;
}

}  // namespace

extern "C" {

int soda_hip_wrap_host(void* array, int32_t elem_bytes, int32_t dim,
                       const int32_t* extent, const int32_t* ghost_lo,
                       const int32_t* ghost_hi) {
  if (!array || !extent || !ghost_lo || !ghost_hi || dim < 1 ||
      dim > SODA_HIP_MAX_DIM ||
      (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 &&
       elem_bytes != 8))
    return SODA_HIP_ERR_INVALID;
  int64_t n[SODA_HIP_MAX_DIM] = {1, 1, 1, 1}, lo[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
  int64_t p[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
  for (int d = 0; d < dim; ++d) {
    if (extent[d] < 1 || ghost_lo[d] < 0 || ghost_hi[d] < 0)
      return SODA_HIP_ERR_INVALID;
    n[d] = extent[d];
    lo[d] = ghost_lo[d];
    p[d] = lo[d] + n[d] + ghost_hi[d];
  }
  char* base = static_cast<char*>(array);
  for (int64_t c3 = 0; c3 < p[3]; ++c3)
    for (int64_t c2 = 0; c2 < p[2]; ++c2)
      for (int64_t c1 = 0; c1 < p[1]; ++c1) {
        const int64_t s3 = lo[3] + wrap(c3 - lo[3], n[3]);
        const int64_t s2 = lo[2] + wrap(c2 - lo[2], n[2]);
        const int64_t s1 = lo[1] + wrap(c1 - lo[1], n[1]);
        const int64_t drow = ((c3 * p[2] + c2) * p[1] + c1) * p[0];
        const int64_t srow = ((s3 * p[2] + s2) * p[1] + s1) * p[0];
        for (int64_t c0 = 0; c0 < p[0]; ++c0) {
          const int64_t s0 = lo[0] + wrap(c0 - lo[0], n[0]);
          if (srow + s0 != drow + c0)     // a ghost cell
            memcpy(base + (drow + c0) * elem_bytes,
                   base + (srow + s0) * elem_bytes, (size_t)elem_bytes);
        }
      }
  return SODA_HIP_OK;
}

}  // extern "C"
