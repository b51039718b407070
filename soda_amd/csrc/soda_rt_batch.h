// soda_rt_batch.h -- one launch over a batch of independent grids.
//
// Pasted behind soda_rt.h into the modules lowered with LowerOptions.batch
// only (their kernels' names end in `_bt`); every other module's text is what
// it was.
//
// A batched kernel is launched on a grid of (blocks, batch, 1): blockIdx.y is
// the ITEM, and everything a block derives from blockIdx.x / gridDim.x -- the
// XCD reorder, its strip and chunk, skip_from / skip_count -- is what it is in
// the unbatched kernel.  The items of a tensor lie one behind the other like a
// contiguous [N, ...] array, so item i of every input, output and
// library-owned local starts
//     i * extent[0] * ... * extent[dim - 1]   cells
// behind the pointer in its a.buf[] slot.  `param` arrays are not moved (every
// item reads the same ones), nor is the debug slot; origin / gextent hold for
// every item alike.
//
// The generator copies the argument block at the top of a batched kernel and
// moves the slots of the copy.  All of it is wave-uniform arithmetic on kernel
// arguments: it lands in the scalar base address of the buffer resources
// (soda_make_rsrc) resp. in the scalar pointers the `direct` and `ldswin`
// kernels index from, costs no vector register and no instruction in a row
// loop.  A buffer window stays relative to the ITEM's base: the 1 GiB limit
// (SODA_BUF_WINDOW_MAX) is per item, the batch as a whole may be any size.

// cells between the same cell of two neighbouring items
template <int kDim>
SODA_DEV int64_t soda_batch_cells(const soda_hip_kargs_t& a) {
  int64_t cells = 1;
#pragma unroll
  for (int d = 0; d < kDim; ++d) cells *= (int64_t)a.extent[d];
  return cells;
}

// slot `base` of the argument block, `cells` cells of kElem bytes further on
template <int kElem>
SODA_DEV void* soda_batch_base(void* base, int64_t cells) {
  return static_cast<char*>(base) + cells * kElem;
}
