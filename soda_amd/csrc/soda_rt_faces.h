// soda_rt_faces.h -- bordered domains whose two faces differ: the ghost frame
// of a padded array under a border mode per FACE (the low and the high wall of
// every dimension) and, per tensor, a constant per face.
//
// Pasted behind soda_rt.h into the faces modules (codegen/hip/faces.py), and
// only those.  The kernel is soda_rt_extend.h's with another rule per cell:
// one kernel per cell size and dimension count does the same three jobs by its
// argument set (fill in place, pad dense -> padded, crop padded -> dense) over
// the same list of regions -- whole rows as 16-byte fragments aligned on the
// destination, row ends one ghost cell per lane -- restated here so that the
// wrap and the extend modules' text stays what it is.
//
// Where the extend kernel says "destination cell c takes source cell
// add + m(c - sub)", m the map of the dimension's mode, this one takes the map
// of the dimension's LOW face where c - sub < 0 and of its HIGH face elsewhere
// (inside [0, n) every map is the identity, so either serves there).  A cell
// outside through a `constant` face takes a constant; where it is outside
// through such faces in several dimensions, that of the HIGHEST dimension, and
// of that face.  So a row that is outside through a constant face of an outer
// dimension is still one splat, its x-corners included, and every other ghost
// row still maps to ONE source row.
//
// Cells are moved, never computed with (unsigned integers per cell size; a
// constant is the cell's bit pattern).  Offsets are 64-bit element counts.
// Modes and constants are wave-uniform, read with compile-time indices only:
// nothing here indexes the argument block with a run-time value, and the side
// is chosen by compare and select.

#define SODA_FACES_BLOCK 256
#define SODA_FACES_MAX_REGIONS 5

// include/soda_hip.h SODA_HIP_BORDER_*
#define SODA_FACES_WRAP 0
#define SODA_FACES_CLAMP 1
#define SODA_FACES_MIRROR 2
#define SODA_FACES_MIRROR101 3
#define SODA_FACES_CONSTANT 4

// must match FacesArgs in soda_periodic.cpp: the wrap kernel's block, then
// the modes of the low and of the high faces and the constants
struct soda_hip_faces_args_t {
  void* dst[16];          // blockIdx.y picks the tensor
  const void* src[16];
  int32_t dext[4];        // extent of the destination arrays
  int32_t sext[4];        // ... of the source arrays
  int32_t n[4];           // the domain
  int32_t sub[4];
  int32_t add[4];
  int32_t glo[4];         // ghost cells below the domain (fill)
  int32_t nreg;
  // a region's rows, as in soda_rt_wrap.h
  int32_t level[SODA_FACES_MAX_REGIONS];
  uint32_t per_row[SODA_FACES_MAX_REGIONS];   // items of a row
  uint32_t ends[SODA_FACES_MAX_REGIONS];      // != 0: row ends, cell by cell
  uint32_t reserved;
  uint64_t start[SODA_FACES_MAX_REGIONS];     // first item of the region
  uint64_t total;                             // items of all regions
  int32_t mode_lo[4];     // SODA_FACES_* of the low face per dimension
  int32_t mode_hi[4];     // ... of the high face
  // per tensor, dimension and side (0 low, 1 high): the cell's bits in the
  // low bytes
  uint64_t constant[16][4][2];
};

// v mod m (the mathematical one) for m up to 2^32 - 1
SODA_DEV uint32_t soda_faces_mod(int v, uint32_t m) {
  return v >= 0 ? (uint32_t)v % m : m - 1u - (uint32_t)(-(v + 1)) % m;
}

// The cell of [0, n) that cell j of the extended line takes under the modes of
// the two faces; -1: none (outside through a constant face).
SODA_DEV int soda_faces_map(int j, int n, int mode_lo, int mode_hi) {
  const int mode = j < 0 ? mode_lo : mode_hi;
  const uint32_t un = (uint32_t)n;
  if (mode == SODA_FACES_CLAMP) return j < 0 ? 0 : j >= n ? n - 1 : j;
  if (mode == SODA_FACES_MIRROR) {
    const uint32_t t = soda_faces_mod(j, 2u * un);
    return (int)(t < un ? t : 2u * un - 1u - t);
  }
  if (mode == SODA_FACES_MIRROR101) {
    if (n == 1) return 0;
    const uint32_t t = soda_faces_mod(j, 2u * un - 2u);
    return (int)(t < un ? t : 2u * un - 2u - t);
  }
  if (mode == SODA_FACES_CONSTANT) return j < 0 || j >= n ? -1 : j;
  return (int)soda_faces_mod(j, un);
}

template <class U, int DIM>
SODA_DEV void soda_faces_run(const soda_hip_faces_args_t& a) {
  constexpr int V = 16 / (int)sizeof(U);
  U* dst = nullptr;
  const U* src = nullptr;
  U cst[DIM][2];          // the tensor's constants: registers, never indexed
                          // with a run-time value
  _Pragma("unroll") for (int d = 0; d < DIM; ++d) cst[d][0] = cst[d][1] = (U)0;
  _Pragma("unroll") for (int t = 0; t < 16; ++t)
    if (blockIdx.y == (unsigned)t) {
      dst = static_cast<U*>(a.dst[t]);
      src = static_cast<const U*>(a.src[t]);
      _Pragma("unroll") for (int d = 0; d < DIM; ++d) {
        cst[d][0] = (U)a.constant[t][d][0];
        cst[d][1] = (U)a.constant[t][d][1];
      }
    }
  const int D0 = a.dext[0], N0 = a.n[0], sub0 = a.sub[0], add0 = a.add[0];
  const int lo0 = a.mode_lo[0], hi0 = a.mode_hi[0];
  const uint64_t step = (uint64_t)gridDim.x * SODA_FACES_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * SODA_FACES_BLOCK + threadIdx.x;
       i < a.total; i += step) {
    int level = 0;
    uint32_t per_row = 1u, ends = 0u;
    uint64_t first = 0ull;
    _Pragma("unroll") for (int k = 0; k < SODA_FACES_MAX_REGIONS; ++k)
      if (k < a.nreg && i >= a.start[k]) {
        level = a.level[k];
        per_row = a.per_row[k];
        ends = a.ends[k];
        first = a.start[k];
      }
    const uint64_t j = i - first;
    uint32_t row = (uint32_t)(j / per_row);
    const int item = (int)(j - (uint64_t)row * per_row);
    // the row's coordinates in the destination; the ONE source row it takes,
    // or none: outside through a constant face, and then `rowc`, the constant
    // of the highest such dimension (the loop ascends: the last one stays)
    int64_t doff = 0, soff = 0, dstride = a.dext[0], sstride = a.sext[0];
    bool outside = false;
    U rowc = (U)0;
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
      const int jd = c - a.sub[d];
      const int s = soda_faces_map(jd, a.n[d], a.mode_lo[d], a.mode_hi[d]);
      if (s < 0) {
        outside = true;
        rowc = jd < 0 ? cst[d][0] : cst[d][1];
      }
      doff += c * dstride;
      soff += (a.add[d] + (s < 0 ? 0 : s)) * sstride;
      dstride *= a.dext[d];
      sstride *= a.sext[d];
    }
    U* drow = dst + doff;
    const U* srow = src + soff;
    if (ends) {
      const int x = item < a.glo[0] ? item : item + N0;
      const int s = soda_faces_map(x - sub0, N0, lo0, hi0);
      const U c0 = x - sub0 < 0 ? cst[0][0] : cst[0][1];
      drow[x] = outside ? rowc : s < 0 ? c0 : srow[add0 + s];
      continue;
    }
    // fragment `item` of the row, counted from the 16-byte boundary at or
    // below the row's first cell
    const int off = (int)((reinterpret_cast<uint64_t>(drow) / sizeof(U)) % V);
    const int x0 = item * V - off;
    const bool in_row = x0 >= 0 && x0 + V <= D0;
    if (outside) {
      if (in_row) {
        U frag[V];
        _Pragma("unroll") for (int e = 0; e < V; ++e) frag[e] = rowc;
        soda_store_frag<U, V, false>(drow + x0, frag);
      } else {
        _Pragma("unroll") for (int e = 0; e < V; ++e) {
          const int x = x0 + e;
          if (x >= 0 && x < D0) drow[x] = rowc;
        }
      }
      continue;
    }
    // inside the domain along x every map is the identity
    const bool whole = in_row && x0 >= sub0 && x0 - sub0 + V <= N0;
    const U* sp = srow + (add0 + x0 - sub0);
    if (whole && reinterpret_cast<uint64_t>(sp) % 16 == 0) {
      U frag[V];
      soda_load_frag<U, V, false>(frag, sp);
      soda_store_frag<U, V, false>(drow + x0, frag);
    } else {
      _Pragma("unroll") for (int e = 0; e < V; ++e) {
        const int x = x0 + e;
        if (x >= 0 && x < D0) {
          const int s = soda_faces_map(x - sub0, N0, lo0, hi0);
          const U c0 = x - sub0 < 0 ? cst[0][0] : cst[0][1];
          drow[x] = s < 0 ? c0 : srow[add0 + s];
        }
      }
    }
  }
}

#define SODA_FACES_KERNEL(NAME, U, DIM)                                  \
  extern "C" __global__ void __launch_bounds__(SODA_FACES_BLOCK)         \
  NAME(soda_hip_faces_args_t a) { soda_faces_run<U, DIM>(a); }
