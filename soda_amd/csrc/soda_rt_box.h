// soda_rt_box.h -- the box mover: a short list of boxes copied between dense
// arrays of different extents.
//
// Pasted behind soda_rt.h into the box modules (codegen/hip/box.py), and only
// those.  A fused bordered run gathers the rims of the padded state into narrow
// strips and scatters the strips' rims back with it; it depends on no stencil
// and on no border mode.  One kernel per cell size and dimension count; one
// launch moves every box of its list for every tensor (blockIdx.y).
//
// A box is a destination origin, a source origin and a size, all in cells.  Its
// rows move as soda_rt_extend.h's do: as 16-byte fragments aligned on the
// DESTINATION, a fragment as one load and one store where it lies whole inside
// the row and its source is aligned too, cell by cell elsewhere -- at the two
// ends of a row, and everywhere in a box whose source and destination differ
// in their alignment.
//
// Cells are moved, never computed with (unsigned integers per cell size).
// Offsets are 64-bit element counts.  Which box an item belongs to is
// wave-uniform or nearly so and is read with compile-time indices only:
// nothing here indexes the argument block with a run-time value.

#define SODA_BOX_BLOCK 256
#define SODA_BOX_MAX 4

// must match BoxArgs in soda_periodic.cpp
struct soda_hip_box_args_t {
  void* dst[16];          // blockIdx.y picks the tensor
  const void* src[16];
  int32_t dext[4];        // extent of the destination arrays
  int32_t sext[4];        // ... of the source arrays
  int32_t nbox;
  uint32_t reserved;
  int32_t dorg[SODA_BOX_MAX][4];   // first cell of the box in the destination
  int32_t sorg[SODA_BOX_MAX][4];   // ... in the source
  int32_t size[SODA_BOX_MAX][4];   // cells per dimension, all >= 1
  uint32_t per_row[SODA_BOX_MAX];  // fragments a row of the box may need
  uint64_t start[SODA_BOX_MAX];    // first item of the box
  uint64_t total;                  // items of all boxes
};

template <class U, int DIM>
SODA_DEV void soda_box_run(const soda_hip_box_args_t& a) {
  constexpr int V = 16 / (int)sizeof(U);
  U* dst = nullptr;
  const U* src = nullptr;
  _Pragma("unroll") for (int t = 0; t < 16; ++t)
    if (blockIdx.y == (unsigned)t) {
      dst = static_cast<U*>(a.dst[t]);
      src = static_cast<const U*>(a.src[t]);
    }
  const uint64_t step = (uint64_t)gridDim.x * SODA_BOX_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * SODA_BOX_BLOCK + threadIdx.x;
       i < a.total; i += step) {
    int dorg[DIM], sorg[DIM], size[DIM];
    _Pragma("unroll") for (int d = 0; d < DIM; ++d) {
      dorg[d] = 0;
      sorg[d] = 0;
      size[d] = 1;
    }
    uint32_t per_row = 1u;
    uint64_t first = 0ull;
    _Pragma("unroll") for (int k = 0; k < SODA_BOX_MAX; ++k)
      if (k < a.nbox && i >= a.start[k]) {
        _Pragma("unroll") for (int d = 0; d < DIM; ++d) {
          dorg[d] = a.dorg[k][d];
          sorg[d] = a.sorg[k][d];
          size[d] = a.size[k][d];
        }
        per_row = a.per_row[k];
        first = a.start[k];
      }
    const uint64_t j = i - first;
    uint32_t row = (uint32_t)(j / per_row);
    const int item = (int)(j - (uint64_t)row * per_row);
    // the row's first cell in either array
    int64_t doff = dorg[0], soff = sorg[0];
    int64_t dstride = a.dext[0], sstride = a.sext[0];
    _Pragma("unroll") for (int d = 1; d < DIM; ++d) {
      int t;
      if (d < DIM - 1) {
        t = (int)(row % (uint32_t)size[d]);
        row /= (uint32_t)size[d];
      } else {
        t = (int)row;
      }
      doff += (int64_t)(dorg[d] + t) * dstride;
      soff += (int64_t)(sorg[d] + t) * sstride;
      dstride *= a.dext[d];
      sstride *= a.sext[d];
    }
    U* drow = dst + doff;
    const U* srow = src + soff;
    // fragment `item` of the row, counted from the 16-byte boundary at or
    // below the row's first cell
    const int off = (int)((reinterpret_cast<uint64_t>(drow) / sizeof(U)) % V);
    const int x0 = item * V - off;
    const bool whole = x0 >= 0 && x0 + V <= size[0];
    if (whole && reinterpret_cast<uint64_t>(srow + x0) % 16 == 0) {
      U frag[V];
      soda_load_frag<U, V, false>(frag, srow + x0);
      soda_store_frag<U, V, false>(drow + x0, frag);
    } else {
      _Pragma("unroll") for (int e = 0; e < V; ++e) {
        const int x = x0 + e;
        if (x >= 0 && x < size[0]) drow[x] = srow[x];
      }
    }
  }
}

#define SODA_BOX_KERNEL(NAME, U, DIM)                                 \
  extern "C" __global__ void __launch_bounds__(SODA_BOX_BLOCK)        \
  NAME(soda_hip_box_args_t a) { soda_box_run<U, DIM>(a); }
