// soda_rt_wrap.h -- periodic domains: the ghost frame of a padded array
// (DESIGN.md 4.11).
//
// Pasted behind soda_rt.h into the wrap modules (codegen/hip/wrap.py), and
// only those.  One kernel per cell size and dimension count does three jobs,
// told apart by its argument set alone:
//
//   fill  in place on a padded array: every ghost cell takes the interior
//         cell it mirrors.  Reads interior cells only, writes ghost cells
//         only: corners, edges and faces need no order among them.
//   pad   dense domain array -> padded array, every cell of it.
//   crop  interior of a padded array -> dense domain array.
//
// All three are "destination cell c takes source cell add + ((c - sub) mod n)"
// per dimension, the modulo the mathematical one.  The work is a list of
// regions of destination rows (a row: the cells along dimension 0); a region
// gives every row the same number of items, one lane takes one item:
//
//   whole rows  (pad, crop; fill: the rows with an outer coordinate in the
//               ghost frame) -- an item is a fragment of 16 bytes, laid so
//               that the DESTINATION is aligned; where its cells are
//               consecutive in the source and the source is aligned too it
//               moves as one load and one store, else cell by cell;
//   row ends    (fill: the rows inside the torus) -- an item is one ghost cell
//               of dimension 0.
//
// Cells are moved, never computed with: the kernels are built per cell size on
// unsigned integers.  Offsets are 64-bit element counts.  Nothing here indexes
// the argument block with a run-time value (that would copy it to scratch).

#define SODA_WRAP_BLOCK 256
#define SODA_WRAP_MAX_REGIONS 5

// must match WrapArgs in soda_periodic.cpp
struct soda_hip_wrap_args_t {
  void* dst[16];          // blockIdx.y picks the tensor
  const void* src[16];
  int32_t dext[4];        // extent of the destination arrays
  int32_t sext[4];        // ... of the source arrays
  int32_t n[4];           // the torus
  int32_t sub[4];
  int32_t add[4];
  int32_t glo[4];         // ghost cells below the torus (fill)
  int32_t nreg;
  // a region's rows: dimension d (1 <= d < DIM) runs over the whole
  // destination extent where d < level, over the ghost cells where d == level,
  // over the torus where d > level.  level = DIM: every row; level = 0: the
  // rows inside the torus
  int32_t level[SODA_WRAP_MAX_REGIONS];
  uint32_t per_row[SODA_WRAP_MAX_REGIONS];   // items of a row
  uint32_t ends[SODA_WRAP_MAX_REGIONS];      // != 0: row ends, cell by cell
  uint32_t reserved;
  uint64_t start[SODA_WRAP_MAX_REGIONS];     // first item of the region
  uint64_t total;                            // items of all regions
};

SODA_DEV int soda_wrap_mod(int v, int n) {
  const int m = v % n;
  return m < 0 ? m + n : m;
}

template <class U, int DIM>
SODA_DEV void soda_wrap_run(const soda_hip_wrap_args_t& a) {
  constexpr int V = 16 / (int)sizeof(U);
  U* dst = nullptr;
  const U* src = nullptr;
  _Pragma("unroll") for (int t = 0; t < 16; ++t)
    if (blockIdx.y == (unsigned)t) {
      dst = static_cast<U*>(a.dst[t]);
      src = static_cast<const U*>(a.src[t]);
    }
  const int D0 = a.dext[0], N0 = a.n[0], sub0 = a.sub[0], add0 = a.add[0];
  const uint64_t step = (uint64_t)gridDim.x * SODA_WRAP_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * SODA_WRAP_BLOCK + threadIdx.x;
       i < a.total; i += step) {
    int level = 0;
    uint32_t per_row = 1u, ends = 0u;
    uint64_t first = 0ull;
    _Pragma("unroll") for (int k = 0; k < SODA_WRAP_MAX_REGIONS; ++k)
      if (k < a.nreg && i >= a.start[k]) {
        level = a.level[k];
        per_row = a.per_row[k];
        ends = a.ends[k];
        first = a.start[k];
      }
    const uint64_t j = i - first;
    uint32_t row = (uint32_t)(j / per_row);
    const int item = (int)(j - (uint64_t)row * per_row);
    // the row's coordinates in the destination, the source row it mirrors
    int64_t doff = 0, soff = 0, dstride = a.dext[0], sstride = a.sext[0];
    _Pragma("unroll") for (int d = 1; d < DIM; ++d) {
      const uint32_t radix = d < level    ? (uint32_t)a.dext[d]
                             : d == level ? (uint32_t)(a.dext[d] - a.n[d])
                                          : (uint32_t)a.n[d];
      int t;
      if (d < DIM - 1) {
        t = (int)(row % radix);
        row /= radix;
      } else {
        t = (int)row;
      }
      const int c = d < level    ? t
                    : d == level ? (t < a.glo[d] ? t : t + a.n[d])
                                 : a.glo[d] + t;
      const int s = a.add[d] + soda_wrap_mod(c - a.sub[d], a.n[d]);
      doff += c * dstride;
      soff += s * sstride;
      dstride *= a.dext[d];
      sstride *= a.sext[d];
    }
    U* drow = dst + doff;
    const U* srow = src + soff;
    if (ends) {
      const int x = item < a.glo[0] ? item : item + N0;
      drow[x] = srow[add0 + soda_wrap_mod(x - sub0, N0)];
      continue;
    }
    // fragment `item` of the row, counted from the 16-byte boundary at or
    // below the row's first cell
    const int off = (int)((reinterpret_cast<uint64_t>(drow) / sizeof(U)) % V);
    const int x0 = item * V - off;
    const bool whole = x0 >= 0 && x0 + V <= D0 && x0 >= sub0 &&
                       x0 - sub0 + V <= N0;
    const U* sp = srow + (add0 + x0 - sub0);
    if (whole && reinterpret_cast<uint64_t>(sp) % 16 == 0) {
      U frag[V];
      soda_load_frag<U, V, false>(frag, sp);
      soda_store_frag<U, V, false>(drow + x0, frag);
    } else {
      _Pragma("unroll") for (int e = 0; e < V; ++e) {
        const int x = x0 + e;
        if (x >= 0 && x < D0)
          drow[x] = srow[add0 + soda_wrap_mod(x - sub0, N0)];
      }
    }
  }
}

#define SODA_WRAP_KERNEL(NAME, U, DIM)                                   \
  extern "C" __global__ void __launch_bounds__(SODA_WRAP_BLOCK)          \
  NAME(soda_hip_wrap_args_t a) { soda_wrap_run<U, DIM>(a); }
