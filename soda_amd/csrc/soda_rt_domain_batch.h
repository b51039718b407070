// soda_rt_domain_batch.h -- the wrap and extend kernels over a batch of
// independent domains.
//
// Pasted behind soda_rt_wrap.h resp. soda_rt_extend.h into the BATCHED wrap
// and extend modules only (codegen/hip/wrap.py, extend.py with batch=True;
// their kernels' names end in `_bt`); every other module's text is what it
// was.
//
// A batched helper kernel is launched on a grid of (blocks, tensors, batch):
// blockIdx.y stays the tensor, blockIdx.z is the ITEM, and everything a lane
// derives from blockIdx.x / gridDim.x is what it is in the unbatched kernel.
// The items of an array lie one behind the other like a contiguous [N, ...]
// array.  The argument is the unbatched kernel's block followed by two cell
// counts, the distance between the same cell of two neighbouring items in
// the destination and in the source arrays (fill: prod(P), prod(P); pad:
// prod(P), prod(N); crop: prod(N), prod(P)).
//
// The kernel copies the block, moves the 16 dst and 16 src slots of the copy
// by blockIdx.z items -- compile-time slot indices, wave-uniform arithmetic on
// kernel arguments, as in soda_rt_batch.h: no vector register, no scratch --
// and runs the unbatched body on the copy.  An item's base need not be
// 16-byte aligned: the body lays its fragments by the row's address.

// must match the steps soda_periodic.cpp puts behind WrapArgs / ExtendArgs
template <class Args>
struct soda_hip_domain_bt_args_t {
  Args a;
  uint64_t dstep;         // cells from an item to the next, destination
  uint64_t sstep;         // ... source
};

// the dst / src slots of `a` moved by blockIdx.z items of cells of type U
template <class U, class Args>
SODA_DEV void soda_domain_bt_move(Args& a, uint64_t dstep, uint64_t sstep) {
  const uint64_t item = (uint64_t)blockIdx.z;
  _Pragma("unroll") for (int t = 0; t < 16; ++t) {
    a.dst[t] = static_cast<U*>(a.dst[t]) + item * dstep;
    a.src[t] = static_cast<const U*>(a.src[t]) + item * sstep;
  }
}

// ARGS / RUN: soda_hip_wrap_args_t / soda_wrap_run, or the extend pair
#define SODA_DOMAIN_BT_KERNEL(NAME, ARGS, RUN, U, DIM)                   \
  extern "C" __global__ void __launch_bounds__(256)                      \
  NAME(soda_hip_domain_bt_args_t<ARGS> b) {                              \
    ARGS a = b.a;                                                        \
    soda_domain_bt_move<U>(a, b.dstep, b.sstep);                         \
    RUN<U, DIM>(a);                                                      \
  }
