// soda_box.cpp -- the host twin of the box kernels (DESIGN.md 4.13,
// include/soda_hip.h soda_hip_box_host): boxes copied between two dense host
// arrays of different extents, in plain C++.  No HIP, no allocation, no global
// state: the file compiles with any host compiler on its own
// (tests/host/box_main.cpp does).
#include "soda_hip.h"

#include <string.h>

extern "C" {

int soda_hip_box_host(void* dst, const int32_t* dst_extent, const void* src,
                      const int32_t* src_extent, int32_t elem_bytes,
                      int32_t dim, int32_t num_boxes,
                      const int32_t* dst_origin, const int32_t* src_origin,
                      const int32_t* size) {
  if (!dst || !src || !dst_extent || !src_extent || dim < 1 ||
      dim > SODA_HIP_MAX_DIM || num_boxes < 0 ||
      (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 &&
       elem_bytes != 8))
    return SODA_HIP_ERR_INVALID;
  if (num_boxes && (!dst_origin || !src_origin || !size))
    return SODA_HIP_ERR_INVALID;
  for (int d = 0; d < dim; ++d)
    if (dst_extent[d] < 1 || src_extent[d] < 1) return SODA_HIP_ERR_INVALID;
  // every box lies inside both arrays, or nothing is written
  for (int b = 0; b < num_boxes; ++b)
    for (int d = 0; d < dim; ++d) {
      const int64_t n = size[b * dim + d];
      const int64_t to = dst_origin[b * dim + d], from = src_origin[b * dim + d];
      if (n < 0 || to < 0 || from < 0 || to + n > dst_extent[d] ||
          from + n > src_extent[d])
        return SODA_HIP_ERR_INVALID;
    }
  char* out = static_cast<char*>(dst);
  const char* in = static_cast<const char*>(src);
  for (int b = 0; b < num_boxes; ++b) {
    int64_t n[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
    int64_t to[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
    int64_t from[SODA_HIP_MAX_DIM] = {0, 0, 0, 0};
    int64_t de[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
    int64_t se[SODA_HIP_MAX_DIM] = {1, 1, 1, 1};
    bool empty = false;
    for (int d = 0; d < dim; ++d) {
      n[d] = size[b * dim + d];
      to[d] = dst_origin[b * dim + d];
      from[d] = src_origin[b * dim + d];
      de[d] = dst_extent[d];
      se[d] = src_extent[d];
      if (n[d] == 0) empty = true;
    }
    if (empty) continue;
    for (int64_t c3 = 0; c3 < n[3]; ++c3)
      for (int64_t c2 = 0; c2 < n[2]; ++c2)
        for (int64_t c1 = 0; c1 < n[1]; ++c1) {
          const int64_t drow =
              (((to[3] + c3) * de[2] + to[2] + c2) * de[1] + to[1] + c1) *
                  de[0] + to[0];
          const int64_t srow =
              (((from[3] + c3) * se[2] + from[2] + c2) * se[1] + from[1] + c1) *
                  se[0] + from[0];
          memcpy(out + drow * elem_bytes, in + srow * elem_bytes,
                 (size_t)(n[0] * elem_bytes));
        }
  }
  return SODA_HIP_OK;
}

}  // extern "C"
