// soda_rt_norms.h -- exact L1 / L2 norms of a residual.
//
// Pasted behind soda_rt.h into the norms modules (codegen/hip/norms.py), and
// only those.  Per cell the delta of `cur` against `prev` is the one
// soda_rt_residual.h takes; a finite delta is an integer m times 2^(s + u), so
// the sums of |d| and d^2 are kept as wide integers: per lane in registers
// (units of a lane-local 2^b), per block in LDS, per run in the caller's
// struct.  Every step is an addition modulo 2^(64 W) with every carry
// delivered, so the words are the true sums in any order; the lane's window
// decides only how often it has to go to LDS.

// must match soda_hip_norms_t in include/soda_hip.h, taken as 64-bit words:
// 0 kind | reserved, 1 count, 2 unordered, 3 infinite, l1[34], l2[67]
#define SODA_NORMS_L1_WORDS 34
#define SODA_NORMS_L2_WORDS 67
#define SODA_NORMS_L1_AT 4
#define SODA_NORMS_L2_AT (SODA_NORMS_L1_AT + SODA_NORMS_L1_WORDS)
#define SODA_NORMS_WORDS (SODA_NORMS_L2_AT + SODA_NORMS_L2_WORDS)
#define SODA_NORMS_BLOCK 256

typedef unsigned long long soda_u64;
typedef unsigned __int128 soda_u128;

// the kernels' one argument: dense `cur` and `prev` of `extent`, the cells
// [lo, hi) counted, the struct they are added to
struct soda_hip_norms_args_t {
  const void* cur;
  const void* prev;
  soda_u64* acc;
  int32_t extent[4];
  int32_t lo[4];
  int32_t hi[4];
};

// ---- a cell's delta: class (0 finite, 1 NaN, 2 +inf), m, s ------------------
template <class T>
struct soda_norms_cell {   // integers: the exact unsigned difference, s = 0
  static constexpr int kWin = 0;
  static constexpr int kMant = sizeof(T) < 8 ? 32 : 64;
  SODA_DEV int decode(T cur, T prev, soda_u64& m, int& s) {
    m = cur > prev ? (soda_u64)cur - (soda_u64)prev
                   : (soda_u64)prev - (soda_u64)cur;
    if (sizeof(T) < 8) m &= 0xffffffffull;
    s = 0;
    return 0;
  }
};
// float / double: one IEEE fabs(cur - prev) in the cell's precision, taken
// apart: m the mantissa with its hidden bit (without, for a subnormal), s the
// biased exponent less one (0 for a subnormal): d = m x 2^(s - 149 | 1074).
// kWin: how far above the lane's base b a shift may lie.  A square is below
// 2^(106 + 2 kWin) and the lane's 192 bits must take 2^16 of them.  kMant:
// the bits of m (integers: of the delta); narrow ones get 64-bit arithmetic
// (soda_norms_add).
template <>
struct soda_norms_cell<float> {
  static constexpr int kWin = 35;
  static constexpr int kMant = 24;
  SODA_DEV int decode(float cur, float prev, soda_u64& m, int& s) {
    const float d = __builtin_fabsf(cur - prev);
    const unsigned b = __builtin_bit_cast(unsigned, d);
    const unsigned e = b >> 23, f = b & 0x7fffffu;
    m = e ? (f | 0x800000u) : f;
    s = e ? (int)e - 1 : 0;
    return d != d ? 1 : e == 0xffu ? 2 : 0;
  }
};
template <>
struct soda_norms_cell<double> {
  static constexpr int kWin = 35;
  static constexpr int kMant = 53;
  SODA_DEV int decode(double cur, double prev, soda_u64& m, int& s) {
    const double d = __builtin_fabs(cur - prev);
    const soda_u64 b = __builtin_bit_cast(soda_u64, d);
    const unsigned e = (unsigned)(b >> 52);
    const soda_u64 f = b & 0xfffffffffffffull;
    m = e ? (f | (1ull << 52)) : f;
    s = e ? (int)e - 1 : 0;
    return d != d ? 1 : e == 0x7ffu ? 2 : 0;
  }
};

// ---- long accumulators in memory --------------------------------------------
// W[idx] += v, the carry forwarded word by word: the old value an atomic
// returns shows whether this very addition wrapped.  `idx < nw` holds by the
// sizing of the struct (64 bits of headroom); it is tested all the same, so
// that no input can send a store out of the words.
SODA_DEV void soda_norms_add_word(soda_u64* W, int nw, int idx, soda_u64 v) {
  while (v != 0ull && idx < nw) {
    const soda_u64 old = atomicAdd(&W[idx], v);
    v = (old + v < old) ? 1ull : 0ull;
    ++idx;
  }
}
// W += (x2 : x1 : x0) << off
SODA_DEV void soda_norms_add_at(soda_u64* W, int nw, int off, soda_u64 x0,
                                soda_u64 x1, soda_u64 x2) {
  const int w = off >> 6, r = off & 63;
  const soda_u64 y0 = x0 << r;
  const soda_u64 y1 = r ? (x1 << r) | (x0 >> (64 - r)) : x1;
  const soda_u64 y2 = r ? (x2 << r) | (x1 >> (64 - r)) : x2;
  const soda_u64 y3 = r ? x2 >> (64 - r) : 0ull;
  soda_norms_add_word(W, nw, w, y0);
  soda_norms_add_word(W, nw, w + 1, y1);
  soda_norms_add_word(W, nw, w + 2, y2);
  soda_norms_add_word(W, nw, w + 3, y3);
}

// ---- what one lane holds ------------------------------------------------------
// sum of |d| in units of 2^(b + u1) (128 bits), of d^2 in units of
// 2^(2 b + u2) (192 bits), `n` values since the last flush.  b < 0: empty.
struct soda_norms_lane_t {
  soda_u128 l1;
  soda_u128 l2_lo;
  soda_u64 l2_hi;
  int b;
  unsigned n;
  unsigned count, unordered, infinite;
};
#define SODA_NORMS_LANE_MAX 65535u   // values a lane adds between two flushes

SODA_DEV void soda_norms_init(soda_norms_lane_t& s) {
  s.l1 = 0;
  s.l2_lo = 0;
  s.l2_hi = 0ull;
  s.b = -1;
  s.n = 0u;
  s.count = s.unordered = s.infinite = 0u;
}

// the lane's sums into the block's words (LDS), the lane empty again
SODA_DEV void soda_norms_flush(soda_norms_lane_t& s, soda_u64* sh) {
  if (s.n != 0u) {
    soda_norms_add_at(sh + SODA_NORMS_L1_AT, SODA_NORMS_L1_WORDS, s.b,
                      (soda_u64)s.l1, (soda_u64)(s.l1 >> 64), 0ull);
    soda_norms_add_at(sh + SODA_NORMS_L2_AT, SODA_NORMS_L2_WORDS, 2 * s.b,
                      (soda_u64)s.l2_lo, (soda_u64)(s.l2_lo >> 64), s.l2_hi);
  }
  s.l1 = 0;
  s.l2_lo = 0;
  s.l2_hi = 0ull;
  s.n = 0u;
}

template <class T>
SODA_DEV void soda_norms_add(soda_norms_lane_t& s, T cur, T prev,
                             soda_u64* sh) {
  typedef soda_norms_cell<T> cell_t;
  soda_u64 m;
  int e;
  const int cls = cell_t::decode(cur, prev, m, e);
  if (cls == 1) { ++s.unordered; return; }
  if (cls == 2) { ++s.infinite; return; }
  ++s.count;
  if (m == 0ull) return;
  // fast path: the shift lies in the window above the base and room is left;
  // else the lane hands its sums to the block and takes a new base, half a
  // window below this value
  if (s.b < 0 || e < s.b || e - s.b > cell_t::kWin ||
      s.n >= SODA_NORMS_LANE_MAX) {
    soda_norms_flush(s, sh);
    s.b = e > cell_t::kWin / 2 ? e - cell_t::kWin / 2 : 0;
  }
  const int t = cell_t::kWin ? e - s.b : 0;
  if constexpr (2 * cell_t::kMant <= 64 && cell_t::kMant + cell_t::kWin <= 64) {
    // m x 2^t and m^2 fit 64 bits, m^2 x 2^(2 t) 128 (fp32: below 2^59, 2^48
    // and 2^118): 64-bit shift and product, nothing beyond the low 128 bits
    // but the carry
    s.l1 += (soda_u128)(m << t);
    const soda_u128 lo = (soda_u128)(m * m) << (2 * t);
    s.l2_lo += lo;
    s.l2_hi += s.l2_lo < lo ? 1ull : 0ull;
  } else {
    const soda_u128 sq = (soda_u128)m * m;        // exact: up to 128 bits
    s.l1 += (soda_u128)m << t;
    const soda_u128 lo = sq << (2 * t);
    const soda_u64 hi = t ? (soda_u64)(sq >> (128 - 2 * t)) : 0ull;
    s.l2_lo += lo;
    s.l2_hi += hi + (s.l2_lo < lo ? 1ull : 0ull);
  }
  ++s.n;
}

// ---- the kernel ----------------------------------------------------------------
// A block owns one segment of 256 fragments of V cells of a row -- or, of
// shorter rows, as many whole rows as its 256 lanes hold -- and strides over
// the rows of an array of DIM dimensions (the library launches a whole number
// of rows' worth of blocks, and a V that divides the row length).
template <class T, int V, int DIM>
SODA_DEV void soda_norms_run(const soda_hip_norms_args_t& a, soda_u64* sh) {
  for (unsigned i = threadIdx.x; i < SODA_NORMS_WORDS; i += SODA_NORMS_BLOCK)
    sh[i] = 0ull;
  __syncthreads();
  soda_norms_lane_t acc;
  soda_norms_init(acc);
  // a row of fewer fragments than the block has lanes: the block takes `rpb`
  // rows at a time, lane l fragment l % frags of the (l / frags)-th of them
  // (one division per lane, outside the loop)
  const unsigned frags = (unsigned)a.extent[0] / V;
  const unsigned rpb = frags < SODA_NORMS_BLOCK ? SODA_NORMS_BLOCK / frags : 1u;
  const unsigned nx =
      rpb > 1u ? 1u : (frags + SODA_NORMS_BLOCK - 1u) / SODA_NORMS_BLOCK;
  const unsigned xc = blockIdx.x % nx, r0 = blockIdx.x / nx,
                 rstep = gridDim.x / nx;
  const unsigned sub = rpb > 1u ? threadIdx.x / frags : 0u;
  const unsigned fx = rpb > 1u ? threadIdx.x - sub * frags
                               : xc * SODA_NORMS_BLOCK + threadIdx.x;
  const int x = (int)(fx * V);
  // (a row is a whole number of fragments: in or out as a whole)
  const bool x_in =
      sub < rpb && fx < frags && x + V > a.lo[0] && x < a.hi[0];
  unsigned rows = 1u;
  for (int d = 1; d < DIM; ++d) rows *= (unsigned)a.extent[d];
  const T* __restrict__ cur_p = (const T*)a.cur;
  const T* __restrict__ prev_p = (const T*)a.prev;
  for (unsigned row = r0 * rpb + sub; row < rows; row += rstep * rpb) {
    bool rows_ok = true;
    unsigned rest = row;
    _Pragma("unroll") for (int d = 1; d < DIM; ++d) {
      int q;
      if (d < DIM - 1) {
        q = (int)(rest % (unsigned)a.extent[d]);
        rest /= (unsigned)a.extent[d];
      } else {
        q = (int)rest;
      }
      rows_ok = rows_ok && q >= a.lo[d] && q < a.hi[d];
    }
    if (x_in && rows_ok) {
      const int64_t c = (int64_t)row * a.extent[0] + x;
      T cur[V], prev[V];
      soda_load_frag<T, V, false>(cur, cur_p + c);
      soda_load_frag<T, V, false>(prev, prev_p + c);
      _Pragma("unroll") for (int e = 0; e < V; ++e)
        if (x + e >= a.lo[0] && x + e < a.hi[0])
          soda_norms_add(acc, cur[e], prev[e], sh);
    }
  }
  soda_norms_flush(acc, sh);
  if (acc.count) atomicAdd(&sh[1], (soda_u64)acc.count);
  if (acc.unordered) atomicAdd(&sh[2], (soda_u64)acc.unordered);
  if (acc.infinite) atomicAdd(&sh[3], (soda_u64)acc.infinite);
  __syncthreads();
  // the block's words that are not zero into the caller's struct
  for (unsigned i = 1u + threadIdx.x; i < SODA_NORMS_WORDS;
       i += SODA_NORMS_BLOCK) {
    const soda_u64 v = sh[i];
    if (v == 0ull) continue;
    if (i < SODA_NORMS_L1_AT)
      atomicAdd(&a.acc[i], v);
    else if (i < SODA_NORMS_L2_AT)
      soda_norms_add_word(a.acc + SODA_NORMS_L1_AT, SODA_NORMS_L1_WORDS,
                          (int)i - SODA_NORMS_L1_AT, v);
    else
      soda_norms_add_word(a.acc + SODA_NORMS_L2_AT, SODA_NORMS_L2_WORDS,
                          (int)i - SODA_NORMS_L2_AT, v);
  }
}

#define SODA_NORMS_KERNEL(NAME, T, V, DIM)                                  \
  extern "C" __global__ void __launch_bounds__(SODA_NORMS_BLOCK)            \
  NAME(soda_hip_norms_args_t a) {                                           \
    __shared__ soda_u64 soda_sh[SODA_NORMS_WORDS];                          \
    soda_norms_run<T, V, DIM>(a, soda_sh);                                  \
  }

// one block: the struct zeroed, its kind set
extern "C" __global__ void __launch_bounds__(SODA_NORMS_BLOCK)
soda_norms_zero(soda_u64* acc, soda_u64 kind) {
  if (threadIdx.x < SODA_NORMS_WORDS)
    acc[threadIdx.x] = threadIdx.x == 0u ? kind : 0ull;
}
