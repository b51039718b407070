// soda_rt_banked.h -- row fragments of a tensor dealt over NB DRAM banks.
//
// Pasted behind soda_rt.h into the modules of the BANKED form of a wire
// stream's dense program only (MarchConfig.banks); every other module's text
// is what it was.  The twins of soda_buf_load_frag / soda_buf_store_frag:
//
// Stream element k of a tensor on NB banks lives in bank k % NB at index
// k / NB (reference docs/data-layout.md "Multi-Bank").  A lane's fragment is V
// consecutive cells from element e on; with NB | V and NB | e it is V / NB
// consecutive elements of EVERY bank from index e / NB on, and cell j of the
// fragment is element j / NB of bank j % NB.  So a fragment is NB accesses of
// 1 / NB of its bytes, each coalesced across the lanes like the dense one, and
// the (de)interleave happens in registers.
//
// Offsets.  The kernels keep computing the DENSE byte offset `off` of a
// fragment -- in range, or carrying SODA_OOB_X / SODA_OOB_ROW (soda_rt.h) --
// and every bank is addressed at off / NB through a resource of
// dense_records / NB bytes (soda_make_rsrc_bank).  That keeps the out-of-range
// discipline:
//   * in range:  off + bytes <= dense_records, NB | off (the generator admits
//     the form only where fragments start on bank-group boundaries), so
//     off / NB + bytes / NB <= dense_records / NB: the same cells, no other.
//   * with a sentinel:  off >= 2^30 >= dense_records (windows are at most
//     SODA_BUF_WINDOW_MAX = 2^30 bytes), and NB | dense_records (NB divides
//     the row pitch), so floor(off / NB) >= dense_records / NB = the bank's
//     num_records: dropped.  A division cannot wrap, and `off` itself did not
//     (soda_rt.h: sums of parts stay below 2^32).
// Single cells (edge-lane halo loads) sit at bank byte offset
// floor(cell / NB) * sizeof(T) = (off / NB) rounded DOWN to a cell; 2^30 / NB
// is a multiple of every cell size, so the rounding keeps a sentinel-carrying
// offset at or above the bank's num_records as well.

template <int NB>
SODA_DEV soda_rsrc_t soda_make_rsrc_bank(const void* bank_base,
                                         int64_t dense_bytes) {
  static_assert(NB == 2 || NB == 4, "banks per tensor");
  const int64_t b = dense_bytes < 0 ? 0
                    : dense_bytes > SODA_BUF_WINDOW_MAX ? SODA_BUF_WINDOW_MAX
                                                        : dense_bytes;
  return soda_make_rsrc(bank_base, b / NB);
}

template <class T, int V, int NB, bool kNonTemporal = false, class... R>
SODA_DEV void soda_buf_load_frag_banked(T (&dst)[V], unsigned off, R... banks) {
  static_assert(sizeof...(R) == NB && V % NB == 0, "NB resources, NB | V");
  int b = 0;
  auto one = [&](soda_rsrc_t r) {
    T part[V / NB];
    soda_buf_load_frag<T, V / NB, kNonTemporal>(part, r, off / NB);
#pragma unroll
    for (int j = 0; j < V / NB; ++j) dst[j * NB + b] = part[j];
    ++b;
  };
  (one(banks), ...);
}

template <class T, int V, int NB, bool kNonTemporal = false, class... R>
SODA_DEV void soda_buf_store_frag_banked(unsigned off, const T (&src)[V],
                                         R... banks) {
  static_assert(sizeof...(R) == NB && V % NB == 0, "NB resources, NB | V");
  int b = 0;
  auto one = [&](soda_rsrc_t r) {
    T part[V / NB];
#pragma unroll
    for (int j = 0; j < V / NB; ++j) part[j] = src[j * NB + b];
    soda_buf_store_frag<T, V / NB, kNonTemporal>(r, off / NB, part);
    ++b;
  };
  (one(banks), ...);
}

// one cell at dense byte offset `off`, from the bank the generator worked out
// for it (the cell's position relative to the strip decides, a constant)
template <class T, int NB>
SODA_DEV void soda_buf_load_cell_banked(T (&dst)[1], soda_rsrc_t bank,
                                        unsigned off) {
  soda_buf_load_frag<T, 1, false>(dst, bank,
                                  (off / NB) & ~(unsigned)(sizeof(T) - 1));
}
