// soda_rt_residual.h -- residual of a run's last iteration.
//
// Pasted behind soda_rt.h into modules lowered with LowerOptions.residual, and
// only those.  Per cell the delta of `cur` (the output after N iterations)
// against `prev` (the input the last iteration saw) is taken in the cell
// type's own arithmetic; four order-independent quantities are kept -- two
// counts, two maxima -- so the result is the same bits however lanes, waves
// and blocks reduce.

// must match soda_hip_residual_t in include/soda_hip.h
struct soda_hip_residual_t {
  unsigned long long changed;         // cells whose delta is non-zero or NaN
  unsigned long long unordered;       // cells whose delta is NaN
  unsigned long long max_float_bits;  // largest float delta, bits of a double
  unsigned long long max_int;         // largest integer delta
};

// must match soda_hip_resbox_t in include/soda_hip.h: the cells counted of
// every pair, [lo, hi) per dimension of the arrays a launch addresses
#define SODA_RES_MAX_PAIRS 8
struct soda_hip_resbox_t {
  int32_t lo[SODA_RES_MAX_PAIRS][4];
  int32_t hi[SODA_RES_MAX_PAIRS][4];
};

// What one lane has seen so far.  One field per kind of cell; a kernel's
// pairs touch the ones of their types and the compiler drops the rest.  A
// lane counts in 32 bits (a chunk, or a grid-stride share of an array, is far
// below 2^32 cells); the counts widen before they leave the lane.
struct soda_res_lane_t {
  unsigned changed;
  unsigned unordered;
  float max_f32;
  double max_f64;
  unsigned max_i32;
  unsigned long long max_i64;
};

SODA_DEV void soda_res_init(soda_res_lane_t& s) {
  s.changed = 0u;
  s.unordered = 0u;
  s.max_f32 = 0.0f;
  s.max_f64 = 0.0;
  s.max_i32 = 0u;
  s.max_i64 = 0ull;
}

// float / double: fabs(cur - prev), one IEEE subtraction in the cell's
// precision.  NaN counts as changed and unordered and stays out of the
// maximum (`d > max` is false for it); +0 against -0 gives +0: unchanged.
SODA_DEV void soda_res_add(soda_res_lane_t& s, float cur, float prev, bool ok) {
  const float d = __builtin_fabsf(cur - prev);
  s.changed += (ok && !(d == 0.0f)) ? 1u : 0u;
  s.unordered += (ok && d != d) ? 1u : 0u;
  s.max_f32 = (ok && d > s.max_f32) ? d : s.max_f32;
}
SODA_DEV void soda_res_add(soda_res_lane_t& s, double cur, double prev, bool ok) {
  const double d = __builtin_fabs(cur - prev);
  s.changed += (ok && !(d == 0.0)) ? 1u : 0u;
  s.unordered += (ok && d != d) ? 1u : 0u;
  s.max_f64 = (ok && d > s.max_f64) ? d : s.max_f64;
}
// integers up to 32 bits: |cur - prev| is below 2^32, so the wrapping
// unsigned difference of the larger and the smaller is exact
#define SODA_RES_INT32(T)                                                    \
  SODA_DEV void soda_res_add(soda_res_lane_t& s, T cur, T prev, bool ok) {   \
    const unsigned d = cur > prev ? (unsigned)cur - (unsigned)prev           \
                                  : (unsigned)prev - (unsigned)cur;          \
    s.changed += (ok && d != 0u) ? 1u : 0u;                                  \
    s.max_i32 = (ok && d > s.max_i32) ? d : s.max_i32;                       \
  }
SODA_RES_INT32(int8_t)
SODA_RES_INT32(uint8_t)
SODA_RES_INT32(int16_t)
SODA_RES_INT32(uint16_t)
SODA_RES_INT32(int32_t)
SODA_RES_INT32(uint32_t)
#undef SODA_RES_INT32
// int64 / uint64: the unsigned 64-bit absolute difference
#define SODA_RES_INT64(T)                                                    \
  SODA_DEV void soda_res_add(soda_res_lane_t& s, T cur, T prev, bool ok) {   \
    const unsigned long long d =                                             \
        cur > prev ? (unsigned long long)cur - (unsigned long long)prev      \
                   : (unsigned long long)prev - (unsigned long long)cur;     \
    s.changed += (ok && d != 0ull) ? 1u : 0u;                                \
    s.max_i64 = (ok && d > s.max_i64) ? d : s.max_i64;                       \
  }
SODA_RES_INT64(int64_t)
SODA_RES_INT64(uint64_t)
#undef SODA_RES_INT64

// ---- the tail: one wave reduction, then lane 0's atomics --------------------
// A 64-bit value moved within its row of 16 lanes by DPP row_shr:n, lanes
// without a source read 0 -- the identity of both the sum and the unsigned
// maximum.
template <int kCtrl>
SODA_DEV unsigned long long soda_res_dpp(unsigned long long v) {
  // (through soda_opaque: the shifted halves stay instructions of their own,
  // see soda_rt.h on folding integer DPP operands)
  const int lo = soda_opaque(__builtin_amdgcn_update_dpp(
      0, (int)(unsigned)v, kCtrl, 0xf, 0xf, true));
  const int hi = soda_opaque(__builtin_amdgcn_update_dpp(
      0, (int)(unsigned)(v >> 32), kCtrl, 0xf, 0xf, true));
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
SODA_DEV unsigned long long soda_res_lane(unsigned long long v, int lane) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
  const unsigned hi =
      (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}
// sum / maximum over the wave, the same value in every lane.  All 64 lanes
// must be active (the kernels call it outside any divergent branch).
SODA_DEV unsigned long long soda_res_wave_sum(unsigned long long v) {
  v += soda_res_dpp<0x111>(v);   // row_shr:1
  v += soda_res_dpp<0x112>(v);   // row_shr:2
  v += soda_res_dpp<0x114>(v);   // row_shr:4
  v += soda_res_dpp<0x118>(v);   // row_shr:8: lane 15 of a row holds its sum
  return soda_res_lane(v, 15) + soda_res_lane(v, 31) + soda_res_lane(v, 47) +
         soda_res_lane(v, 63);
}
SODA_DEV unsigned long long soda_res_max2(unsigned long long a,
                                          unsigned long long b) {
  return a > b ? a : b;
}
SODA_DEV unsigned long long soda_res_wave_max(unsigned long long v) {
  v = soda_res_max2(v, soda_res_dpp<0x111>(v));
  v = soda_res_max2(v, soda_res_dpp<0x112>(v));
  v = soda_res_max2(v, soda_res_dpp<0x114>(v));
  v = soda_res_max2(v, soda_res_dpp<0x118>(v));
  return soda_res_max2(
      soda_res_max2(soda_res_lane(v, 15), soda_res_lane(v, 31)),
      soda_res_max2(soda_res_lane(v, 47), soda_res_lane(v, 63)));
}

// End of a kernel: the wave's four values, then one atomic each from lane 0,
// skipped where the operand is zero.  The bit pattern of a non-negative,
// non-NaN double orders like its value, +inf included, and an fp32 delta
// widens exactly: one unsigned 64-bit maximum serves both precisions.
SODA_DEV void soda_res_flush(const soda_res_lane_t& s, soda_hip_residual_t* r) {
  const double f32 = (double)s.max_f32;
  const double mf = f32 > s.max_f64 ? f32 : s.max_f64;
  const unsigned long long mi =
      soda_res_max2((unsigned long long)s.max_i32, s.max_i64);
  const unsigned long long changed =
      soda_res_wave_sum((unsigned long long)s.changed);
  const unsigned long long unordered =
      soda_res_wave_sum((unsigned long long)s.unordered);
  const unsigned long long max_f = soda_res_wave_max(
      (unsigned long long)__builtin_bit_cast(long long, mf));
  const unsigned long long max_i = soda_res_wave_max(mi);
  if ((threadIdx.x & 63u) == 0u) {
    if (changed) atomicAdd(&r->changed, changed);
    if (unordered) atomicAdd(&r->unordered, unordered);
    if (max_f) atomicMax(&r->max_float_bits, max_f);
    if (max_i) atomicMax(&r->max_int, max_i);
  }
}
