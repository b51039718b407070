// soda_extend.cpp -- the host twin of the extend kernels (DESIGN.md 4.12,
// include/soda_hip.h soda_hip_extend_host): the ghost frame of a padded host
// array refilled from its interior under a border mode per dimension, in plain
// C++.  No HIP, no allocation, no global state: the file compiles with any
// host compiler on its own (tests/host/extend_main.cpp does).
#include "soda_hip.h"

#include <string.h>

namespace {

int64_t mod(int64_t v, int64_t n) {
  const int64_t m = v % n;
  return m < 0 ? m + n : m;
}

// the cell of [0, n) that cell j of the extended line takes; -1: the constant
int64_t map(int64_t j, int64_t n, int32_t mode) {
  switch (mode) {
    case SODA_HIP_BORDER_CLAMP:
      return j < 0 ? 0 : j >= n ? n - 1 : j;
    case SODA_HIP_BORDER_MIRROR: {
      const int64_t t = mod(j, 2 * n);
      return t < n ? t : 2 * n - 1 - t;
    }
    case SODA_HIP_BORDER_MIRROR101: {
      if (n == 1) return 0;
      const int64_t t = mod(j, 2 * n - 2);
      return t < n ? t : 2 * n - 2 - t;
    }
    case SODA_HIP_BORDER_CONSTANT:
      return j < 0 || j >= n ? -1 : j;
    default:
      return mod(j, n);
  }
}

}  // namespace

extern "C" {

int soda_hip_extend_host(void* array, int32_t elem_bytes, int32_t dim,
                         const int32_t* extent, const int32_t* ghost_lo,
                         const int32_t* ghost_hi, const int32_t* modes,
                         uint64_t constant) {
  if (!array || !extent || !ghost_lo || !ghost_hi || !modes || dim < 1 ||
      dim > SODA_HIP_MAX_DIM ||
      (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 &&
       elem_bytes != 8))
    return SODA_HIP_ERR_INVALID;
  int64_t n[SODA_HIP_MAX_DIM] = {1, 1, 1, 1}, lo[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
  int64_t p[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
  int32_t m[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
  for (int d = 0; d < dim; ++d) {
    if (extent[d] < 1 || ghost_lo[d] < 0 || ghost_hi[d] < 0 ||
        modes[d] < SODA_HIP_BORDER_WRAP || modes[d] > SODA_HIP_BORDER_CONSTANT)
      return SODA_HIP_ERR_INVALID;
    n[d] = extent[d];
    lo[d] = ghost_lo[d];
    p[d] = lo[d] + n[d] + ghost_hi[d];
    m[d] = modes[d];
  }
  // the cell's bytes, lowest first, whatever the host's byte order
  unsigned char cst[8];
  for (int b = 0; b < 8; ++b) cst[b] = (unsigned char)(constant >> (8 * b));
  char* base = static_cast<char*>(array);
  for (int64_t c3 = 0; c3 < p[3]; ++c3)
    for (int64_t c2 = 0; c2 < p[2]; ++c2)
      for (int64_t c1 = 0; c1 < p[1]; ++c1) {
        const int64_t s3 = map(c3 - lo[3], n[3], m[3]);
        const int64_t s2 = map(c2 - lo[2], n[2], m[2]);
        const int64_t s1 = map(c1 - lo[1], n[1], m[1]);
        const bool outside = s3 < 0 || s2 < 0 || s1 < 0;
        const int64_t drow = ((c3 * p[2] + c2) * p[1] + c1) * p[0];
        const int64_t srow = outside ? 0 :
            (((lo[3] + s3) * p[2] + lo[2] + s2) * p[1] + lo[1] + s1) * p[0];
        for (int64_t c0 = 0; c0 < p[0]; ++c0) {
          const int64_t s0 = map(c0 - lo[0], n[0], m[0]);
          char* cell = base + (drow + c0) * elem_bytes;
          if (outside || s0 < 0)
            memcpy(cell, cst, (size_t)elem_bytes);
          else if (srow + lo[0] + s0 != drow + c0)     // a ghost cell
            memcpy(cell, base + (srow + lo[0] + s0) * elem_bytes,
                   (size_t)elem_bytes);
        }
      }
  return SODA_HIP_OK;
}

// The same with a mode per FACE and a constant per (dimension, side)
// (DESIGN.md 4.16): below the domain the map of the dimension's low face,
// above it that of its high face; a cell outside through constant faces takes
// the constant of the HIGHEST such dimension, and of that face.
int soda_hip_extend_faces_host(void* array, int32_t elem_bytes, int32_t dim,
                               const int32_t* extent, const int32_t* ghost_lo,
                               const int32_t* ghost_hi,
                               const int32_t* modes_lo,
                               const int32_t* modes_hi,
                               const uint64_t* constants) {
  if (!array || !extent || !ghost_lo || !ghost_hi || !modes_lo || !modes_hi ||
      !constants || dim < 1 || dim > SODA_HIP_MAX_DIM ||
      (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 &&
       elem_bytes != 8))
    return SODA_HIP_ERR_INVALID;
  int64_t n[SODA_HIP_MAX_DIM] = {1, 1, 1, 1}, lo[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
  int64_t p[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
  int32_t ml[SODA_HIP_MAX_DIM] = {0, 0, 0, 0}, mh[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
  // the cells' bytes, lowest first, whatever the host's byte order
  unsigned char cst[SODA_HIP_MAX_DIM][2][8] = {};
  for (int d = 0; d < dim; ++d) {
    if (extent[d] < 1 || ghost_lo[d] < 0 || ghost_hi[d] < 0 ||
        modes_lo[d] < SODA_HIP_BORDER_WRAP ||
        modes_lo[d] > SODA_HIP_BORDER_CONSTANT ||
        modes_hi[d] < SODA_HIP_BORDER_WRAP ||
        modes_hi[d] > SODA_HIP_BORDER_CONSTANT ||
        // a dimension wraps on both faces or on none
        (modes_lo[d] == SODA_HIP_BORDER_WRAP) !=
            (modes_hi[d] == SODA_HIP_BORDER_WRAP))
      return SODA_HIP_ERR_INVALID;
    n[d] = extent[d];
    lo[d] = ghost_lo[d];
    p[d] = lo[d] + n[d] + ghost_hi[d];
    ml[d] = modes_lo[d];
    mh[d] = modes_hi[d];
    for (int side = 0; side < 2; ++side)
      for (int b = 0; b < 8; ++b)
        cst[d][side][b] = (unsigned char)(constants[2 * d + side] >> (8 * b));
  }
  auto face = [&](int d, int64_t c) {
    const int64_t j = c - lo[d];
    return map(j, n[d], j < 0 ? ml[d] : mh[d]);
  };
  char* base = static_cast<char*>(array);
  for (int64_t c3 = 0; c3 < p[3]; ++c3)
    for (int64_t c2 = 0; c2 < p[2]; ++c2)
      for (int64_t c1 = 0; c1 < p[1]; ++c1) {
        const int64_t c[4] = {0, c1, c2, c3};
        int64_t s[4] = {0, 0, 0, 0};
        const unsigned char* rowc = nullptr;     // ascending: the highest stays
        for (int d = 1; d < 4; ++d) {
          s[d] = face(d, c[d]);
          if (s[d] < 0) {
            rowc = cst[d][c[d] < lo[d] ? 0 : 1];
            s[d] = 0;
          }
        }
        const int64_t drow = ((c3 * p[2] + c2) * p[1] + c1) * p[0];
        const int64_t srow =
            (((lo[3] + s[3]) * p[2] + lo[2] + s[2]) * p[1] + lo[1] + s[1]) *
            p[0];
        for (int64_t c0 = 0; c0 < p[0]; ++c0) {
          const int64_t s0 = face(0, c0);
          char* cell = base + (drow + c0) * elem_bytes;
          if (rowc)
            memcpy(cell, rowc, (size_t)elem_bytes);
          else if (s0 < 0)
            memcpy(cell, cst[0][c0 < lo[0] ? 0 : 1], (size_t)elem_bytes);
          else if (srow + lo[0] + s0 != drow + c0)     // a ghost cell
            memcpy(cell, base + (srow + lo[0] + s0) * elem_bytes,
                   (size_t)elem_bytes);
        }
      }
  return SODA_HIP_OK;
}

}  // extern "C"
