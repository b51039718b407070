/* soda_hip.h -- C ABI of the MI355X stencil execution backend (libsoda_hip.so).
 *
 * This is the drop-in boundary for the hot path "execute the stencil a .soda
 * file describes".  In the reference that path is GENERATED code reached
 * through two interfaces, both replaced here:
 *
 *   (1) the kernel C ABI the generated host calls,
 *         extern "C" void <app>_kernel(ap_uint<BW>* bank_i_<out>...,
 *                                      ap_uint<BW>* bank_i_<in>...,
 *                                      uint64_t coalesced_data_num);
 *       reference src/soda/codegen/frt/host.py:44-59 (declaration),
 *       :282-289 (call), src/soda/codegen/xilinx/hls_kernel.py:62-66
 *       (definition).  Argument order there is OUTPUTS FIRST, THEN INPUTS;
 *       soda_hip_run_device() keeps that order.  The reference kernel
 *       returns void and has no error channel; every function here returns
 *       a status instead (0 = success, cf. `return 0;` frt/host.py:429).
 *
 *   (2) the operator-level host entry,
 *         int soda::app::<app>(const T* var_<in>_ptr, const int32_t extent[],
 *                              const int32_t stride[], const int32_t min[],
 *                              ... same four per output ..., const char*
 *                              bitstream, int burst_width, int tile_size_d...,
 *                              int unroll_factor);
 *       reference src/soda/codegen/frt/host.py:62-88 (signature), :181-249
 *       (tile + scatter), :282-322 (launch), :340-427 (gather of the valid
 *       box).  soda_hip_run_host() takes the same (ptr, extent, stride, min)
 *       quadruple per tensor; `min` is accepted and ignored exactly as the
 *       reference body ignores it; strides are honoured on the caller's
 *       arrays only (frt/host.py:236-246,395-424).
 *
 * The FPGA bitstream argument is replaced by a program handle made from HIP
 * source text (what `sodac --hip-kernel` prints) JIT-compiled for gfx950 plus
 * a launch plan.  Plain C types only; no C++ or torch types cross this ABI.
 * The library is synchronous per call unless a stream is given; it is not
 * re-entrant per program handle (the reference promises none either: single
 * host thread, frt/host.py:319-322) -- on the GPU too: one handle is one queue
 * of work, see "Streams, scratch, graphs" at soda_hip_run_device.
 *
 * Result contract (reference docs/data-layout.md:12-25, frt/host.py:357-375):
 * only cells inside the valid box of each output are defined; everything else
 * in an output array is unspecified.
 */
#ifndef SODA_HIP_H_
#define SODA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped when a struct that crosses the boundary changes layout (7: the plan
 * carries the program's per-iteration reach; 8: the plan says whether its
 * kernels are batched, with soda_hip_run_device_batch,
 * soda_hip_plan_geometry_batch / _schedule_batch and the _batch forms of
 * calibrate / pass_times / schedule).  Entry points added under 7 (no struct
 * changed): soda_hip_host_register / _unregister,
 * soda_hip_host_weave_banks, soda_hip_stream_set_device_dense_min_tile,
 * soda_hip_stream_set_banked / _set_banked_pair (kargs.reserved[0] carries
 * the stream length to their programs); and
 * soda_hip_stream_create accepts wire[o] == NULL for an output on one bank
 * that the program stores at its wire position itself.  Added under 8:
 * soda_hip_program_scratch.  9: the residual of a run's last iteration -- the
 * kernel descriptor names its twin, the plan carries `residual`, with
 * soda_hip_run_device_residual / _until, soda_hip_plan_residual_box and
 * soda_hip_last_residual.  Added under 9 (no struct changed): the residual
 * on slabs and groups -- soda_hip_plan_residual_slab_box,
 * soda_hip_run_device_slab_residual, soda_hip_plan_launches_residual,
 * soda_hip_group_run_residual, soda_hip_group_residual,
 * soda_hip_group_last_residual, soda_hip_group_run_until; and the exact L1 /
 * L2 norms of the residual -- soda_hip_norms_t with soda_hip_norms_fold /
 * _value / _host / _create / _destroy / _zero / _accumulate,
 * soda_hip_run_device_norms and soda_hip_run_device_until_norm; and periodic
 * domains -- soda_hip_wrap_host, soda_hip_periodic_plan / _create / _destroy /
 * _info / _fill / _run_padded / _run_device; and bordered domains --
 * soda_hip_extend_host, soda_hip_border_plan / _create / _destroy / _info /
 * _fill / _run_padded / _run_device with soda_hip_border_desc_t; and their
 * fused form -- soda_hip_box_host, soda_hip_border_fused_plan / _create /
 * _destroy / _info / _move / _run_padded / _run_device with
 * soda_hip_border_fused_desc_t; and a border mode and a constant per face --
 * soda_hip_border_faces_t with soda_hip_extend_faces_host and the `_faces`
 * twin of every entry that takes a bordered or a fused bordered request. */
#define SODA_HIP_ABI_VERSION 9
#define SODA_HIP_MAX_DIM 4
#define SODA_HIP_MAX_TENSORS 16
#define SODA_HIP_MAX_KERNELS 32
#define SODA_HIP_MAX_PASSES 8
#define SODA_HIP_MAX_PASS_KERNELS 16
#define SODA_HIP_MAX_PARAMS 8
#define SODA_HIP_NAME_LEN 96
#define SODA_HIP_MAX_RES_PAIRS 8       /* input / output pairs of a residual */
#define SODA_HIP_RES_NONE (-(1 << 30)) /* residual plan: no dependence */

enum soda_hip_status {
  SODA_HIP_OK = 0,
  SODA_HIP_ERR_INVALID = 1,     /* bad argument / plan / extent */
  SODA_HIP_ERR_COMPILE = 2,     /* hiprtc rejected the source; see last_error */
  SODA_HIP_ERR_RUNTIME = 3,     /* a HIP call failed; see last_error */
  SODA_HIP_ERR_NOMEM = 4,       /* host or device allocation failed */
  SODA_HIP_ERR_NODEVICE = 5,    /* no usable GPU */
  SODA_HIP_ERR_UNSUPPORTED = 6  /* valid request this build cannot serve */
};

/* Argument block every generated kernel receives by value
 * (`extern "C" __global__ void k(soda_hip_kargs_t a)`).  Tensor slots are
 * program-wide: inputs first, then outputs, then locals. */
typedef struct soda_hip_kargs {
  void* buf[SODA_HIP_MAX_TENSORS];     /* device pointers by slot */
  int64_t stride[SODA_HIP_MAX_DIM];    /* in elements; dimension 0 fastest */
  int32_t extent[SODA_HIP_MAX_DIM];    /* cells per dimension */
  int32_t ntile[SODA_HIP_MAX_DIM];     /* blocks per dimension; grid.x = product */
  int32_t tile[SODA_HIP_MAX_DIM];      /* cells one block owns (the kernel
                                          descriptor's tile: chunk lengths are
                                          run-time values, tuned per GPU/extent
                                          without recompiling) */
  int32_t origin[SODA_HIP_MAX_DIM];    /* position of the arrays' cell 0 in ... */
  int32_t gextent[SODA_HIP_MAX_DIM];   /* ... the global grid (a slab of a
                                          multi-GPU run; = 0 / extent else):
                                          `border: preserve` is about the
                                          GLOBAL border */
  int32_t skip_from;                   /* a launch may cover a marching kernel's
                                          chunks with a run of them left out:
                                          block tile t along the streamed
                                          dimension stands for tile
                                          t + (t >= skip_from ? skip_count : 0)
                                          (ntile there = tiles launched).  The
                                          chunks next to a slab's ghost rows
                                          and the rest then run as two
                                          launches, around a halo exchange
                                          (soda_hip_run_device_slab); 0, 0
                                          everywhere else */
  int32_t skip_count;
  int32_t reserved[2];
} soda_hip_kargs_t;

typedef struct soda_hip_kernel_desc {
  char name[SODA_HIP_NAME_LEN];        /* extern "C" symbol in the code object */
  int32_t block[3];                    /* threads per block */
  int32_t tile[SODA_HIP_MAX_DIM];      /* output cells one block owns, per dim */
  int32_t lds_bytes;                   /* dynamic LDS */
  /* What the library needs to check a launch and to shape it for the extent
   * it is given at RUN time (the reference bakes tile sizes into its kernel
   * at compile time, hls_kernel.py:30-202; here only the code is fixed, the
   * launch geometry is not).  All zero: a kernel with a fixed tile and no
   * constraint. */
  int32_t vec;                         /* cells per lane: extent[0] must be a
                                          multiple (0 / 1: any) */
  int32_t march_dim;                   /* 1 + the dimension a marching kernel
                                          streams along (its tile there is the
                                          chunk, a run-time value); 0: none */
  int32_t waves_along;                 /* waves of a block along that dimension */
  int32_t warm;                        /* row steps of pipeline warm-up a chunk
                                          pays on top of its own rows */
  int32_t window_extra;                /* buffer addressing: planes beyond the
                                          chunk one wave's window spans; the
                                          window must stay <= 1 GiB.  -1: plain
                                          pointers, no limit */
  int32_t max_elem;                    /* bytes of the widest element so addressed */
  int32_t vgprs;                       /* registers per lane of the compiled
                                          kernel (occupancy); 0: unknown, the
                                          tile is used as given */
  int32_t pipe;                        /* waves sharing the fused iterations */
  int32_t chunk_fixed;                 /* 1: never re-size the chunk */
  /* time model of one launch, used to pick the chunk and, per pass, the
   * multiset of passes that advances `iterate` iterations fastest on THIS
   * extent:  max(k * (chunk + warm - warm_saved) * step_ns, bytes / HBM rate)
   * with k = waves per SIMD the grid needs */
  float step_ns;                       /* one row step of one wave, ns of SIMD
                                          issue time; 0: memory time only */
  float warm_saved;                    /* row steps' worth of work the peeled
                                          warm-up skips */
  float bytes_per_cell;                /* HBM bytes per cell per launch (inputs
                                          + outputs), before halo re-reads */
  float lane_redundancy;               /* lanes of a strip / lanes that store */
  int32_t max_extent0;                 /* > 0: the kernel's block covers the
                                          whole row (its waves hand x-halos
                                          over through LDS): extent[0] must not
                                          exceed this, else ERR_INVALID */
  int32_t twin;                        /* ABI 9, plans with a residual only:
                                          index of this kernel's twin -- the
                                          same kernel, same stores, which also
                                          takes the residual of its last fused
                                          iteration: `k(soda_hip_kargs_t a,
                                          soda_hip_residual_t* r,
                                          soda_hip_resbox_t box)` -- or -1 */
} soda_hip_kernel_desc_t;

/* The residual of the last iteration of a run of N iterations: how much that
 * iteration changed the grid.  32 device bytes.
 *   pairs   every output o pairs with the input i it replaces, by position
 *           (under `border: preserve`: the input it keeps its border from).
 *           `cur` is o after N iterations; `prev` is that input as the last
 *           iteration saw it: o after N - 1 iterations, or the caller's input
 *           when N = 1.
 *   cells   o's valid box after N iterations (the whole array under `border:
 *           preserve`).
 *   delta   per cell, in the cell type's own arithmetic.  float and double:
 *           fabs(cur - prev), one IEEE operation in the cell's precision.
 *           Integers up to 32 bits: |cur - prev| exactly, in 64 bits.  int64
 *           and uint64: the unsigned 64-bit absolute difference.
 * All four fields are sums or maxima of exact per-cell values, taken over all
 * pairs: no reduction order can change them. */
typedef struct soda_hip_residual {
  uint64_t changed;          /* cells whose delta is non-zero or NaN; +0
                                against -0 is unchanged */
  uint64_t unordered;        /* cells whose delta is NaN (a NaN cell, or
                                inf - inf): counted in `changed`, left out of
                                the maxima */
  uint64_t max_float_bits;   /* bit pattern of the largest float delta as a
                                double (an fp32 delta widens exactly; for
                                non-negative non-NaN values the pattern orders
                                like the value; +inf is an ordinary value) */
  uint64_t max_int;          /* largest integer delta */
} soda_hip_residual_t;

/* Third argument of a residual kernel: the cells counted, [lo, hi) per pair
 * and dimension of the arrays the launch addresses. */
typedef struct soda_hip_resbox {
  int32_t lo[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
  int32_t hi[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
} soda_hip_resbox_t;

/* What a plan says about residuals (plan.residual.present != 0: the program
 * was built with LowerOptions.residual / sodac --hip-residual).  `kernel` is
 * `<app>_residual(kargs, r, box)`: dense cur (output slots) against dense prev
 * (input slots), launched on a whole number of rows' worth of blocks.  The rest lets the library
 * find every output's valid box after N iterations without the program text:
 * one iteration maps the bounds of its inputs' windows to its outputs',
 *   lo(o) = min(base_lo[o], min over i of dep_lo[o][i] + min(lo(i), 0))
 * per dimension, `hi` alike with max (SODA_HIP_RES_NONE: o does not read i);
 * N rounds from zero windows give the window of N iterations, the box is the
 * array less that window.  whole != 0 (`border: preserve`): the whole array. */
typedef struct soda_hip_residual_plan {
  int32_t present;
  int32_t kernel;
  int32_t zero_kernel;   /* `<app>_residual_zero(soda_hip_residual_t* r)`: one
                            block of 64 threads zeroes the struct */
  int32_t whole;
  int32_t base_lo[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
  int32_t base_hi[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
  int32_t dep_lo[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
  int32_t dep_hi[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
} soda_hip_residual_plan_t;

/* One way of advancing the program by `fused_iters` iterations: the listed
 * kernels launched in order (one fused kernel, or one kernel per stage). */
typedef struct soda_hip_pass_desc {
  int32_t fused_iters;
  int32_t num_kernels;
  int32_t kernel[SODA_HIP_MAX_PASS_KERNELS];
  float cost;                          /* relative time of one such pass (any
                                          unit) where the kernels carry no time
                                          model (step_ns and bytes_per_cell all
                                          zero); <= 0 in every pass: schedule
                                          greedily, deepest first */
} soda_hip_pass_desc_t;

typedef struct soda_hip_plan {
  int32_t abi_version;                 /* SODA_HIP_ABI_VERSION */
  int32_t dim;
  int32_t num_inputs;
  int32_t num_outputs;
  int32_t num_locals;                  /* scratch tensors the library owns */
  int32_t num_params;                  /* `param` arrays (ref grammar.py:41-45,
                                          frt/host.py:72-78): small read-only
                                          arrays, C order, the same for every
                                          iteration */
  int32_t param_elems[SODA_HIP_MAX_PARAMS];  /* elements per param array */
  /* slots: inputs, outputs, locals, params -- bytes per element of each */
  int32_t elem_size[SODA_HIP_MAX_TENSORS];
  int32_t num_kernels;
  soda_hip_kernel_desc_t kernels[SODA_HIP_MAX_KERNELS];
  int32_t num_passes;                  /* sorted by fused_iters, largest first;
                                          the last one must have fused_iters 1
                                          when the program iterates.  A run of
                                          N iterations uses the multiset of
                                          passes of least total cost that adds
                                          up to N, deepest first */
  soda_hip_pass_desc_t passes[SODA_HIP_MAX_PASSES];
  /* ABI 7: cells ONE iteration of the program reads below / above a cell
   * along the last dimension (the per-iteration growth of the outputs'
   * windows, reference core.py:858-919), valid if has_reach != 0.  Lets the
   * host-array entries cut a run into bands along that dimension -- each band
   * a window run with iterate x reach ghost rows -- so that the copy-in of
   * band i + 1 and the copy-out of band i - 1 run beside the kernels of band
   * i; without it they copy in, run, copy out. */
  int32_t has_reach;
  int32_t reach_lo, reach_hi;
  /* ABI 8: != 0 -- every kernel of the plan is a batched one: it takes
   * blockIdx.y as the item of a batch of grids that lie one behind the other
   * in every input, output and local (not in the param arrays) and is
   * launched on (blocks, batch, 1).  Only such a plan runs through
   * soda_hip_run_device_batch; every other entry runs it as a batch of 1. */
  int32_t batched;
  /* ABI 9: the residual kernels of the plan.  Kernels named here or as a
   * `twin` belong to no pass. */
  soda_hip_residual_plan_t residual;
} soda_hip_plan_t;

typedef struct soda_hip_program soda_hip_program_t;   /* opaque */
typedef struct soda_hip_event soda_hip_event_t;       /* opaque */

/* -- library ------------------------------------------------------------ */
int soda_hip_abi_version(void);
const char* soda_hip_status_string(int status);
/* Copies the calling thread's last error text (NUL-terminated) into buf;
 * returns the full length. */
size_t soda_hip_last_error(char* buf, size_t cap);
int soda_hip_device_count(int* count);
/* sizeof() of the ABI structs as this library was compiled, for bindings to
 * check their mirrors: 0 kargs, 1 kernel_desc, 2 pass_desc, 3 plan,
 * 4 host_tensor, 5 stream_desc, 6 slab_run, 7 group_desc, 8 slab_info,
 * 9 group_stats, 10 launch_info, 11 residual, 12 resbox, 14 norms,
 * 15 periodic_desc, 16 periodic_info, 17 border_desc, 18 border_fused_desc,
 * 19 border_strip, 20 border_fused_info, 21 border_fused_boxes,
 * 22 border_faces; 0 for anything else (13 among them). */
size_t soda_hip_sizeof(int which);

/* -- JIT: HIP source text -> gfx950 code object (hiprtc; needs no GPU) ---- */
int soda_hip_compile(const char* source, const char* name,
                     const char* const* options, int32_t num_options,
                     void** code, size_t* code_size);
void soda_hip_free_code(void* code);
/* Version of the hiprtc that compiles (kernels built by another version may
 * differ in registers and code size, which the launch geometry and the
 * choice of peeled warm-up depend on: caches are keyed by it). */
int soda_hip_compiler_version(int32_t* major, int32_t* minor);

/* -- launch geometry (pure functions of the plan: no GPU, no program) ------- */
/* What a run on `extent` would use: the tile of every kernel (num_kernels x
 * SODA_HIP_MAX_DIM values; chunk lengths sized so the grid fills the 1024
 * SIMDs of an MI355X in whole rounds of equally loaded waves) and the modelled
 * time of every pass in nanoseconds (num_passes values; 0 where the kernels
 * carry no model).  Fails with SODA_HIP_ERR_INVALID -- text in last_error --
 * if a kernel cannot run this extent: rows that are not a multiple of its
 * vector width, a plane too large for its 1 GiB buffer window.  Either output
 * may be NULL. */
int soda_hip_plan_geometry(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t* tiles, float* pass_ns);
/* How many times each pass runs to advance `iterate` iterations on `extent`
 * (num_passes values): the multiset of least total modelled time. */
int soda_hip_plan_schedule(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, int32_t* count);
/* The same two for ONE launch over `batch` grids of `extent`
 * (soda_hip_run_device_batch): the batch multiplies the independent tiles the
 * chunk lengths are sized for and the cells and waves of the time model; the
 * 1 GiB buffer-window check is per item.  batch = 1 is what the two functions
 * above return; batch outside 1..SODA_HIP_MAX_BATCH: SODA_HIP_ERR_INVALID. */
#define SODA_HIP_MAX_BATCH 65535       /* gridDim.y */
int soda_hip_plan_geometry_batch(const soda_hip_plan_t* plan,
                                 const int32_t* extent, int32_t batch,
                                 int32_t* tiles, float* pass_ns);
int soda_hip_plan_schedule_batch(const soda_hip_plan_t* plan,
                                 const int32_t* extent, int32_t batch,
                                 int32_t iterate, int32_t* count);

/* -- program = code object + plan, bound to one device -------------------- */
int soda_hip_program_create(const void* code, size_t code_size,
                            const soda_hip_plan_t* plan, int32_t device,
                            soda_hip_program_t** program);
int soda_hip_program_destroy(soda_hip_program_t* program);

/* Replaces <app>_kernel(): runs `iterate` iterations on device-resident,
 * dense (dim-0-fastest) arrays of `extent`.  outputs first, then inputs, as in
 * the reference ABI.  Inputs are never written.  Asynchronous on `stream`
 * (a hipStream_t, or NULL for the default stream); scratch buffers are owned
 * by the program and reused across calls.  `inputs` holds the num_inputs
 * tensors followed by the num_params param arrays (device pointers to
 * param_elems[k] elements each), the order of the reference's operator
 * signature (frt/host.py:72-78: inputs, outputs, then params).
 *
 * The device entry contract -- two preconditions on the caller's addresses,
 * checked by every run entry below before anything is launched
 * (SODA_HIP_ERR_INVALID, last_error ends in "nothing was launched"):
 *   overlap    no output shares a byte with an input, a param array or
 *              another output, each tensor taken as the dense array of
 *              `extent` (of `batch` such arrays).  Inputs may share.
 *   alignment  every input and output starts on a multiple of
 *              min(16, vec x its cell size) bytes, `vec` being the largest
 *              kernel_desc.vec of the plan (cells per lane; 0 counts as 1); a
 *              param array on a multiple of its cell size.  Kernels move a
 *              tensor in fragments of `vec` cells, one instruction of up to
 *              16 bytes each; extent[0] is a multiple of `vec`
 *              (soda_hip_plan_geometry refuses any other), so every row,
 *              plane, kept row range and slab window starts on a fragment
 *              boundary iff the array does.  A program built for a row length
 *              that is not a multiple of 16 bytes has a smaller `vec` and
 *              asks for less: 4 bytes for an odd number of float cells.
 * What the hardware would make of a misaligned fragment is not measured
 * anywhere; the library never launches on one.  Inside these rules a run
 * writes no byte outside its output arrays and reads none outside its inputs
 * and param arrays (tests/test_device_entry.py runs every kernel family
 * between guard bands).
 *
 * Streams, scratch, graphs -- what "asynchronous on `stream`" means for every
 * soda_hip_run_device* entry and for soda_hip_stream_run_device
 * (tests/test_async.py runs them on a live stream, ahead of their inputs):
 *   ordering   every kernel, fill and copy pass of a call is enqueued on
 *              `stream`, in order; nothing goes to the default stream.  The
 *              one exception, the side stream of a split pass
 *              (SODA_HIP_SPLIT=side), forks from `stream` and joins it again
 *              by events inside the call: whatever follows the call on
 *              `stream` sees all of its results.
 *   blocking   two kinds of call wait for the GPU and are NOT asynchronous:
 *              the first run of more than one iteration on an extent of a
 *              program that calibrates by itself (below), and a call that
 *              grows the program's scratch -- the ping-pong temporaries, the
 *              locals, a stream object's staging arrays: a larger extent, a
 *              larger batch, the first trimmed run of three passes or more.
 *              Growing allocates, and where it replaces a buffer it first
 *              waits for the whole device: earlier calls may still use it.
 *              Scratch never shrinks (soda_hip_program_scratch tells).
 *   one queue  a handle is one queue of work: its scratch is shared by all of
 *              its calls.  Calls on ONE stream need nothing; a call on another
 *              stream must be ordered behind the handle's earlier calls by
 *              the caller (an event), and two streams may not run one handle
 *              at the same time.  Handles are independent of each other.
 *   graphs     a call on a stream that is being captured never calibrates and
 *              never allocates: if its scratch would have to grow it returns
 *              SODA_HIP_ERR_INVALID before anything is launched or allocated,
 *              and the capture stays valid.  The recipe: run the call once
 *              eagerly with the same extent, iterate, batch and keep range
 *              (soda_hip_program_calibrate first, if the clock is to pick the
 *              schedule), then capture.  The graph holds the addresses of
 *              the program's scratch: it may be replayed until a later call
 *              on the handle grows that scratch, or the handle is destroyed
 *              -- replaying it after that uses freed memory.  Eager calls
 *              that fit the scratch may run between replays, ordered against
 *              them like any two calls.  Runs that are handed events
 *              (soda_hip_run_device_slab) and group runs are not meant for
 *              capture. */
/* Same, for arrays that are a window of a larger grid (one GPU's slab):
 * `origin` = global position of cell 0 of the arrays, `global_extent` = size
 * of the whole grid (NULL, NULL = the arrays are the grid).  Only programs
 * with `border: preserve` look at them. */
int soda_hip_run_device_window(soda_hip_program_t* program,
                               void* const* outputs,
                               const void* const* inputs,
                               const int32_t* extent, const int32_t* origin,
                               const int32_t* global_extent, int32_t iterate,
                               void* stream);

/* Same, when the caller needs only part of the result: the cells [keep_lo,
 * keep_hi) along the LAST dimension (a slab's own rows -- its ghost rows are
 * refreshed by the next halo exchange anyway).  One iteration reads `reach_lo`
 * cells below and `reach_hi` above a cell along that dimension.  Every pass is
 * then launched only on the rows the iterations still to come can carry into
 * the kept range (a cone that narrows pass by pass); outside it the outputs
 * are unspecified -- NOT "unchanged": the last pass still stores up to
 * fused_iters x reach rows on either side of [keep_lo, keep_hi), computed with
 * zeros where the launch ended, and leaves the rows beyond those as they
 * were (no pass before the last one writes the outputs of such a run: they
 * alternate between temporaries of the program), so a caller that reuses the
 * output arrays sees a mix of stale and wrong rows there.  A side with keep_lo = 0 (keep_hi = extent) is never
 * trimmed.  The reference has no counterpart: its host tiles with a
 * replicated halo and recomputes all of it (frt/host.py:124-128). */
int soda_hip_run_device_cone(soda_hip_program_t* program,
                             void* const* outputs, const void* const* inputs,
                             const int32_t* extent, const int32_t* origin,
                             const int32_t* global_extent, int32_t iterate,
                             int32_t keep_lo, int32_t keep_hi,
                             int32_t reach_lo, int32_t reach_hi, void* stream);
/* Same, for a slab whose ghost rows are refreshed by a halo exchange the
 * caller runs on another stream -- RCCL send/recv, peer copies; the library
 * only sees the two events -- so that the exchange hides under the compute:
 *   ghost_lo / ghost_hi  rows [0, ghost_lo) and [extent - ghost_hi, extent) of
 *                        the INPUT arrays are being written by an exchange
 *                        that is complete when `ghosts_ready` (a hipEvent_t)
 *                        fires.  The chunks of the first pass whose inputs
 *                        stay clear of these rows are launched at once, the
 *                        others behind the event.  NULL: the ghosts are fresh;
 *   send_lo / send_hi    rows [keep_lo, keep_lo + send_lo) and [keep_hi -
 *                        send_hi, keep_hi) of the RESULT are what the
 *                        neighbours fetch next.  The chunks of the last pass
 *                        that deliver them, AND every chunk that writes a row
 *                        outside [keep_lo, keep_hi) -- the result's ghost
 *                        rows, which the next exchange overwrites -- whether
 *                        or not that side sends anything (a one-sided reach
 *                        has ghosts above and sends below), go first;
 *                        `sendable` (a hipEvent_t, recorded exactly once per
 *                        call; NULL: none) fires behind them; the rest of
 *                        the pass follows and writes kept rows only -- the
 *                        next exchange may start while it computes.
 * A split pass is two launches on `stream`, the part that does not depend on
 * the exchange first (environment SODA_HIP_SPLIT=side: the boundary chunks on
 * a stream the program owns, ordered against `stream` by events, so the parts
 * share the GPU -- measured slower).  Passes that are not one
 * marching kernel along the last dimension run whole: wait, compute, signal.
 * What the library cannot see is who still READS the arrays a call writes: a
 * neighbour that fetches rows of this slab's state on ITS stream must have
 * finished before a later call overwrites that state.  With a two-sided reach
 * the event chain implies it (its fetch -> its next pass -> its `sendable` ->
 * my next exchange -> my `ghosts_ready`); with a one-sided reach -- a slab
 * that sends to a neighbour it never receives from -- the caller has to order
 * `stream` behind that neighbour's fetch itself (soda_group.cpp does; a
 * transport that batches a rank's sends with its receives, like
 * dist.StreamOverlap, is covered by `ghosts_ready`).
 * The reference has no counterpart (one
 * device, frt/host.py:319-322); SURVEY.md 8(e): "compute boundary planes
 * first, send, compute interior". */
typedef struct soda_hip_slab_run {
  int32_t keep_lo, keep_hi;            /* as in soda_hip_run_device_cone */
  int32_t reach_lo, reach_hi;
  int32_t ghost_lo, ghost_hi;
  int32_t send_lo, send_hi;
  void* ghosts_ready;
  void* sendable;
} soda_hip_slab_run_t;
int soda_hip_run_device_slab(soda_hip_program_t* program, void* const* outputs,
                             const void* const* inputs, const int32_t* extent,
                             const int32_t* origin,
                             const int32_t* global_extent, int32_t iterate,
                             const soda_hip_slab_run_t* run, void* stream);
/* The launches a soda_hip_run_device_slab call on `extent` would issue, in
 * order, by the plan's time model (no GPU, no program; `run` may be NULL, its
 * two events only count as "given" or not): which rows of the last dimension
 * every pass covers and how a pass next to the exchange is cut -- block tiles
 * of `chunk` rows, `chunks` of them, the boundary [0, bnd_lo) U [bnd_hi,
 * chunks) on the side stream, the interior beside it.  At most `capacity`
 * entries are written; *count is the number of launches. */
typedef struct soda_hip_launch_info {
  int32_t fused_iters;
  int32_t lo, hi;
  int32_t wait, record, split;
  int32_t chunk, chunks, bnd_lo, bnd_hi;
} soda_hip_launch_info_t;
int soda_hip_plan_launches(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, const soda_hip_slab_run_t* run,
                           int32_t capacity, soda_hip_launch_info_t* launches,
                           int32_t* count);
/* Cells along the last dimension the passes of the last run covered, summed
 * over the passes (a run that trims reports fewer than passes x extent). */
int soda_hip_last_rows(soda_hip_program_t* program, int64_t* rows);
int soda_hip_run_device(soda_hip_program_t* program, void* const* outputs,
                        const void* const* inputs, const int32_t* extent,
                        int32_t iterate, void* stream);
/* soda_hip_run_device on `batch` independent grids of `extent` in ONE launch
 * per kernel: every input and output pointer addresses `batch` dense items,
 * one behind the other like a contiguous [batch, ...] array; the param arrays
 * are shared by all items.  Per item the semantics (and the bits) are those of
 * soda_hip_run_device; asynchronous on `stream`.  The program's scratch -- the
 * ping-pong temporaries, the locals of passes made of several kernels -- is
 * sized for the batch and grows when a later call brings a larger one; chunk
 * lengths, the schedule and its calibration are chosen for the whole launch
 * and remembered per (extent, batch).  No tensor of the call may overlap
 * another, each taken as `batch` items long.  SODA_HIP_ERR_INVALID, text in
 * last_error: batch outside 1..SODA_HIP_MAX_BATCH, or a program whose plan is
 * not batched (LowerOptions.batch / sodac --hip-batch) -- the entry never
 * falls back to a loop of launches.  batch = 1 is legal. */
int soda_hip_run_device_batch(soda_hip_program_t* program,
                              void* const* outputs, const void* const* inputs,
                              const int32_t* extent, int32_t batch,
                              int32_t iterate, void* stream);

/* soda_hip_run_device that also tells how much the LAST of the `iterate`
 * iterations changed the grid: the soda_hip_residual_t defined above is left
 * in the caller's 32 device bytes `residual_dev` (8-byte aligned, no byte
 * shared with an output).  Same contract checks, same guard behaviour, inputs
 * are never written.  Asynchronous on `stream` under "Streams, scratch,
 * graphs": the struct is zeroed by a small kernel of the program enqueued on
 * `stream` inside the call, nothing waits on the host, and the call can be captured once an eager
 * call has sized the scratch -- every replay zeroes and refills the struct.
 * The passes are the multiset soda_hip_run_device would launch; only their
 * order may differ: a scheduled pass whose kernel has a twin goes last and is
 * launched as its twin (the deepest such pass).  If no scheduled pass has
 * one -- `direct`, `ldswin`, `tile3d` passes, a marching depth whose twin did
 * not fit -- or SODA_HIP_RESIDUAL_GENERIC=1 is set (A/B runs), the run ends in
 * the one-iteration pass, taken out of a deeper pass's count if the schedule
 * had none (iterate - 1 iterations are scheduled, one is added), followed by
 * `<app>_residual` over the outputs and that pass's inputs.
 * SODA_HIP_ERR_UNSUPPORTED, nothing launched: a program built without
 * `residual`.  Slabs are served by soda_hip_run_device_slab_residual, groups
 * by soda_hip_group_run_residual; batches are not served. */
int soda_hip_run_device_residual(soda_hip_program_t* program,
                                 void* const* outputs,
                                 const void* const* inputs,
                                 const int32_t* extent, int32_t iterate,
                                 void* residual_dev, void* stream);
/* Iterates until converged.  SYNCHRONOUS: advances `check_every` iterations at
 * a time through the entry above (the last chunk may be shorter), after each
 * chunk fetches the 32 bytes and waits for them, and stops when
 *   unordered == 0 && max_float <= tol && max_int <= int_tol
 * or when `max_iterate` iterations are done.  SODA_HIP_OK either way;
 * *iterations_done and *result_host (either may be NULL) tell which.  The
 * struct is that of the last iteration done, its cells the valid box after
 * ALL iterations done so far.  Chunks ping-pong between the caller's outputs
 * and scratch of the program (soda_hip_program_scratch counts it); the
 * caller's inputs are read by the first chunk only and never written; the
 * final iterate ends up in `outputs`, by one device copy per output if it
 * landed in scratch. */
int soda_hip_run_device_until(soda_hip_program_t* program,
                              void* const* outputs, const void* const* inputs,
                              const int32_t* extent, int32_t max_iterate,
                              int32_t check_every, double tol,
                              uint64_t int_tol,
                              soda_hip_residual_t* result_host,
                              int32_t* iterations_done, void* stream);
/* The cells a residual over `iterate` iterations on `extent` counts: [lo, hi)
 * per output and dimension (num_outputs x dim values each), clipped to the
 * array.  Pure function of the plan (no GPU). */
int soda_hip_plan_residual_box(const soda_hip_plan_t* plan,
                               const int32_t* extent, int32_t iterate,
                               int32_t* lo, int32_t* hi);
/* How the last soda_hip_run_device_residual / _slab_residual call of the
 * program took its residual: 0 not at all, 1 in the twin of its last pass, 2
 * by `<app>_residual`; *fused_iters (may be NULL): the fusion depth of that
 * last pass. */
int soda_hip_last_residual(soda_hip_program_t* program, int32_t* mode,
                           int32_t* fused_iters);

/* The cells ONE SLAB of a larger grid counts: [lo, hi) per output and
 * dimension, in the coordinates of the slab's arrays (cell 0 of which sits at
 * `origin` of the grid of `global_extent`).  That is the box
 * soda_hip_plan_residual_box gives for `global_extent` and `iterate`, cut to
 * the rows [keep_lo, keep_hi) of the slab's last dimension -- the rows the slab
 * keeps; its ghost rows are some other slab's to count -- moved by `origin`
 * and clipped to `extent`.  Slabs whose kept rows partition the global rows
 * partition the global box: every cell counts once.  Under `border: preserve`
 * the global box is the whole grid, a slab counts its kept rows.  A slab whose
 * kept rows miss the global box gets lo == hi and counts nothing.  Pure
 * function of the plan (no GPU). */
int soda_hip_plan_residual_slab_box(const soda_hip_plan_t* plan,
                                    const int32_t* global_extent,
                                    const int32_t* origin,
                                    const int32_t* extent, int32_t keep_lo,
                                    int32_t keep_hi, int32_t iterate,
                                    int32_t* lo, int32_t* hi);
/* soda_hip_run_device_slab that also leaves, in the 32 device bytes
 * `residual_dev`, the slab's share of the residual of the last of `iterate`
 * iterations: the cells of soda_hip_plan_residual_slab_box taken at
 * `box_iterate`, the number of iterations the STATE has seen since its inputs
 * were the caller's -- in a run of several exchange intervals more than this
 * call's `iterate`; box_iterate < iterate: SODA_HIP_ERR_INVALID.  The shares
 * of all slabs combine exactly: counts add, maxima take the larger.
 * The pass that takes the residual goes last, as in
 * soda_hip_run_device_residual, and the rows every earlier pass covers are
 * the cone of the order really launched (soda_hip_plan_launches_residual
 * shows them).  A last pass that is split around the exchange runs its twin
 * twice on one struct and one box -- first the boundary chunks, `sendable`
 * recorded exactly once behind them, then the interior -- so when `sendable`
 * fires the send rows are complete but THE RESIDUAL IS NOT: it is complete
 * when the interior has finished, i.e. for whatever follows the call on
 * `stream`.  Where `<app>_residual` takes it, that kernel runs behind both
 * parts.  The ghost rows of the result, which the last pass writes too, lie
 * outside the box.  The struct is zeroed by `<app>_residual_zero` on `stream`
 * inside the call.  "Streams, scratch, graphs" applies as to
 * soda_hip_run_device_slab: with events not meant for capture. */
int soda_hip_run_device_slab_residual(
    soda_hip_program_t* program, void* const* outputs,
    const void* const* inputs, const int32_t* extent, const int32_t* origin,
    const int32_t* global_extent, int32_t iterate, int32_t box_iterate,
    const soda_hip_slab_run_t* run, void* residual_dev, void* stream);
/* soda_hip_plan_launches for a run that takes a residual (by the model; no
 * GPU): the last entry is the pass that takes it, *mode how -- 1: launched as
 * its twin (both parts, if split), 2: followed by `<app>_residual`.
 * SODA_HIP_ERR_UNSUPPORTED: a plan without residual. */
int soda_hip_plan_launches_residual(const soda_hip_plan_t* plan,
                                    const int32_t* extent, int32_t iterate,
                                    const soda_hip_slab_run_t* run,
                                    int32_t capacity,
                                    soda_hip_launch_info_t* launches,
                                    int32_t* count, int32_t* mode);

/* -- exact L1 and L2 norms of the residual ---------------- */
/* The sums of |d| and of d^2 over the deltas d that soda_hip_residual_t takes
 * its maxima of -- same pairs, same cells, same per-cell delta -- accumulated
 * as wide integers (a long accumulator): every finite delta is an integer
 * times 2^u, so is its square, and integer addition has no order.  The words
 * equal the CPU's, bit for bit, however lanes, waves, blocks and slabs add.
 *   kind       SODA_HIP_NORMS_*: which units apply (0: a struct never zeroed)
 *   count      cells whose delta is finite (zero included): those summed
 *   unordered  cells whose delta is NaN, left out of both sums
 *   infinite   cells whose delta is +inf, left out of both sums
 *   l1, l2     little-endian multiword unsigned integers: the sum of |d| in
 *              units of 2^u1, the sum of d^2 in units of 2^u2:
 *                F32  u1 = -149,  u2 = -298     I32 (cells up to 32 bits)  0, 0
 *                F64  u1 = -1074, u2 = -2148    I64                        0, 0
 *              Sized for F64 and 2^64 cells: the largest double is below
 *              2^1024, so a sum is below 2^(1024 + 1074 + 64) = 2^2162 (34
 *              words), of squares below 2^(2048 + 2148 + 64) = 2^4260 (67).
 * The square is exact: an fp32 mantissa squared has 48 bits, an fp64 one 106
 * (the two 53-bit integers multiplied as integers), a 64-bit integer delta
 * 128.  One struct size serves every kind; 840 bytes, 8-byte aligned. */
#define SODA_HIP_NORMS_L1_WORDS 34
#define SODA_HIP_NORMS_L2_WORDS 67
enum soda_hip_norms_kind {
  SODA_HIP_NORMS_F32 = 1,
  SODA_HIP_NORMS_F64 = 2,
  SODA_HIP_NORMS_I32 = 3,   /* integer cells of 8, 16 or 32 bits */
  SODA_HIP_NORMS_I64 = 4
};
/* The ten cell types a norms handle is made for; the kind follows. */
enum soda_hip_cell {
  SODA_HIP_CELL_FLOAT = 0, SODA_HIP_CELL_DOUBLE = 1,
  SODA_HIP_CELL_INT8 = 2, SODA_HIP_CELL_UINT8 = 3,
  SODA_HIP_CELL_INT16 = 4, SODA_HIP_CELL_UINT16 = 5,
  SODA_HIP_CELL_INT32 = 6, SODA_HIP_CELL_UINT32 = 7,
  SODA_HIP_CELL_INT64 = 8, SODA_HIP_CELL_UINT64 = 9
};
typedef struct soda_hip_norms {
  uint32_t kind;
  uint32_t reserved;
  uint64_t count;
  uint64_t unordered;
  uint64_t infinite;
  uint64_t l1[SODA_HIP_NORMS_L1_WORDS];
  uint64_t l2[SODA_HIP_NORMS_L2_WORDS];
} soda_hip_norms_t;
#define SODA_HIP_NORMS_WHICH_L1 1
#define SODA_HIP_NORMS_WHICH_L2 2

/* Pure host functions: no GPU, no allocation, no error text (the status says
 * it all), safe from any thread. */
/* SODA_HIP_NORMS_* of a SODA_HIP_CELL_*, bytes per cell in *elem (may be
 * NULL); 0 for anything else. */
int soda_hip_norms_kind_of(int32_t cell, int32_t* elem);
/* dst += src: counts and sums add.  Kinds must match (SODA_HIP_ERR_INVALID);
 * a sum that leaves its words -- more than 2^64 cells -- is
 * SODA_HIP_ERR_INVALID too, dst then unspecified. */
int soda_hip_norms_fold(soda_hip_norms_t* dst, const soda_hip_norms_t* src);
/* The correctly rounded (to nearest, ties to even) double of the sum of |d|
 * (which = SODA_HIP_NORMS_WHICH_L1) or of d^2 (_L2); +inf above the double
 * range, and +inf when infinite != 0.  `unordered` does not enter: the caller
 * looks at it. */
int soda_hip_norms_value(const soda_hip_norms_t* acc, int32_t which,
                         double* out);
/* The same reduction in plain C++: the cells [lo, hi) (dim values each) of two
 * dense dim-0-fastest host arrays of `extent`, ADDED to *acc, whose kind must
 * be the cell type's (SODA_HIP_ERR_INVALID otherwise; a zeroed struct of that
 * kind to start from: memset and set `kind`). */
int soda_hip_norms_host(const void* cur, const void* prev, int32_t cell,
                        int32_t dim, const int32_t* extent, const int32_t* lo,
                        const int32_t* hi, soda_hip_norms_t* acc);

/* The kernels (soda_amd/codegen/hip/norms.py: a module of its own per cell
 * type and dimension count, independent of any stencil) loaded on `device`.
 * Allocates nothing after create. */
typedef struct soda_hip_norms_handle soda_hip_norms_handle_t;   /* opaque */
int soda_hip_norms_create(const void* code, size_t code_size, int32_t cell,
                          int32_t dim, int32_t device,
                          soda_hip_norms_handle_t** handle);
int soda_hip_norms_destroy(soda_hip_norms_handle_t* handle);
/* Zeroes the 840 device bytes `acc_dev` (8-byte aligned) and sets their kind:
 * a one-block kernel on `stream`, a kernel node like every other under
 * capture. */
int soda_hip_norms_zero(soda_hip_norms_handle_t* handle, void* acc_dev,
                        void* stream);
/* Adds the cells [lo, hi) of the dense device arrays `cur` against `prev`
 * (both of `extent`, aligned to the cell size) to *acc_dev.  Asynchronous on
 * `stream` under "Streams, scratch, graphs"; never allocates, never waits:
 * capturable as it stands.  Does not zero: several pairs, bands or boxes may
 * add into one struct.  An empty box launches nothing. */
int soda_hip_norms_accumulate(soda_hip_norms_handle_t* handle, const void* cur,
                              const void* prev, const int32_t* extent,
                              const int32_t* lo, const int32_t* hi,
                              void* acc_dev, void* stream);
/* soda_hip_run_device_residual by its generic path, with the norms in place of
 * `<app>_residual`: iterate - 1 iterations are scheduled, the run ends in the
 * one-iteration pass, then *acc_dev is zeroed and every pair's outputs are
 * accumulated against that pass's inputs over the box of
 * soda_hip_plan_residual_box after `iterate` iterations.  Same refusals, same
 * contract checks, inputs never written; asynchronous and capturable like
 * that entry.  SODA_HIP_ERR_UNSUPPORTED, nothing launched: a program built
 * without `residual`; pairs whose cell sizes give another kind or size than
 * the handle's (a program of mixed cell types).  SODA_HIP_ERR_INVALID: a
 * handle of another dimension count or device, a struct that overlaps an
 * output. */
int soda_hip_run_device_norms(soda_hip_program_t* program,
                              soda_hip_norms_handle_t* norms,
                              void* const* outputs, const void* const* inputs,
                              const int32_t* extent, int32_t iterate,
                              void* acc_dev, void* stream);
/* soda_hip_run_device_until with the stop rule
 *   unordered == 0 && infinite == 0 && norm <= tol
 * norm = value(l1) for which = SODA_HIP_NORMS_WHICH_L1, sqrt(value(l2)) for
 * _L2.  SYNCHRONOUS; fetches the struct after each chunk; *result_host is the
 * struct of the last chunk. */
int soda_hip_run_device_until_norm(soda_hip_program_t* program,
                                   soda_hip_norms_handle_t* norms,
                                   void* const* outputs,
                                   const void* const* inputs,
                                   const int32_t* extent, int32_t max_iterate,
                                   int32_t check_every, int32_t which,
                                   double tol, soda_hip_norms_t* result_host,
                                   int32_t* iterations_done, void* stream);

/* -- periodic domains: a program on a torus ---------------- */
/* Every run entry above computes on an open box.  Here the domain of extent N
 * is a torus: cell N is cell 0, in every dimension.  The state lives in PADDED
 * arrays of extent P[d] = ghost_lo[d] + N[d] + ghost_hi[d], dense and
 * dim-0-fastest; the interior [ghost_lo, ghost_lo + N) is the torus, and a
 * ghost cell at padded index i mirrors the interior cell
 *   ghost_lo + ((i - ghost_lo) mod N)        (the mathematical modulo)
 * in every dimension at once -- a domain narrower than its ghost frame wraps
 * more than once.  An array whose ghost cells all hold that is WRAPPED.
 * A frame as wide as k iterations reach carries k iterations of the program's
 * ordinary kernels on the padded extent: SODA programs are translation
 * invariant, so a ghost cell evolves into what the wrap of the evolved
 * interior gives, for as long as its window stays inside the array.  The run
 * entries advance k iterations through the ordinary run path on P, refill
 * the frame with one small kernel (codegen/hip/wrap.py, a module of its own
 * per cell size and dimension count), and go on.  The result does not depend
 * on k, bit for bit.
 * Residuals, norms and runs until converged: the block "residual, norms and
 * run_until on a domain" below.
 * Batches of tori: the block "batched domains" below.
 * Not served on a torus: slabs, groups, ranks, the wire format,
 * `border: preserve` (a torus has no border). */
typedef struct soda_hip_periodic_desc {
  int32_t extent[SODA_HIP_MAX_DIM];    /* N, the torus */
  int32_t refill_every;                /* k: iterations between two refills;
                                          0: the largest fused_iters of the
                                          plan's passes, so that a chunk is one
                                          launch at the deepest depth */
  int32_t ghost_lo[SODA_HIP_MAX_DIM];  /* cells k iterations reach below ... */
  int32_t ghost_hi[SODA_HIP_MAX_DIM];  /* ... and above a cell, at least: the
                                          most over all outputs of the window
                                          of k iterations (the caller's to
                                          compute: Stencil.window_bounds(k)).
                                          The library rounds ghost_hi[0] up
                                          until P[0] is a multiple of the
                                          plan's widest `vec` */
  int32_t preserve;                    /* != 0: the program was written with
                                          `border: preserve`, which the plan
                                          does not say: refused */
  int32_t not_iterable;                /* != 0: the outputs are not of the
                                          inputs' types (the plan holds cell
                                          sizes only): iterate > 1 is refused
                                          as on a plan with other numbers of
                                          inputs and outputs */
} soda_hip_periodic_desc_t;
typedef struct soda_hip_periodic_info {
  int32_t refill_every;                /* k as resolved */
  int32_t ghost_lo[SODA_HIP_MAX_DIM];
  int32_t ghost_hi[SODA_HIP_MAX_DIM];  /* [0] as rounded */
  int32_t padded[SODA_HIP_MAX_DIM];    /* P */
  int32_t reserved;
  int64_t scratch_bytes;               /* device bytes a handle holds: one
                                          padded array per input, two per
                                          output (one if the program cannot
                                          iterate) */
} soda_hip_periodic_info_t;
/* The fill on a host array, in plain C++ (no GPU, no allocation): every ghost
 * cell of the padded, dense, dim-0-fastest `array` of `elem_bytes`-byte cells
 * (1, 2, 4 or 8) takes its interior cell.  `extent` is N. */
int soda_hip_wrap_host(void* array, int32_t elem_bytes, int32_t dim,
                       const int32_t* extent, const int32_t* ghost_lo,
                       const int32_t* ghost_hi);
/* What a handle over `plan` and `desc` would use, and how `iterate`
 * iterations are cut: *info (ghosts, P, k; scratch_bytes), and the iterations
 * of every chunk -- k each, the last may be shorter -- in chunks[0, *count)
 * (at most `capacity` written; `chunks` may be NULL, iterate 0: no chunks).
 * Pure function (no GPU, no program).  Refuses what
 * soda_hip_periodic_create and the run entries refuse:
 *   SODA_HIP_ERR_UNSUPPORTED  desc->preserve or a plan whose residual says
 *                             `whole`; a batched plan;
 *   SODA_HIP_ERR_INVALID      extent < 1, negative ghosts or k; with
 *                             plan->has_reach, ghosts along the last
 *                             dimension below k x reach; iterate > 1 on a
 *                             plan with other numbers or cell sizes of
 *                             inputs and outputs, or desc->not_iterable;
 *                             P the kernels cannot run: P[0] beyond a
 *                             max_extent0, a plane above the 1 GiB window
 *                             (soda_hip_plan_geometry on P). */
int soda_hip_periodic_plan(const soda_hip_plan_t* plan,
                           const soda_hip_periodic_desc_t* desc,
                           int32_t iterate, soda_hip_periodic_info_t* info,
                           int32_t capacity, int32_t* chunks, int32_t* count);
/* A handle over `program` for ONE torus.  wrap_code[i] / wrap_code_size[i]:
 * the code object of the wrap module of 1 << i byte cells and the program's
 * dimension count, i = 0..3; needed for every cell size among the program's
 * inputs and outputs, NULL elsewhere.  All scratch of the handle is allocated
 * here.  A refusal (soda_hip_periodic_plan's, or a program on wire-format
 * banks: SODA_HIP_ERR_UNSUPPORTED) launches nothing and allocates nothing.
 * The handle must be destroyed before its program. */
typedef struct soda_hip_periodic soda_hip_periodic_t;   /* opaque */
int soda_hip_periodic_create(soda_hip_program_t* program,
                             const soda_hip_periodic_desc_t* desc,
                             const void* const* wrap_code,
                             const size_t* wrap_code_size,
                             soda_hip_periodic_t** handle);
int soda_hip_periodic_destroy(soda_hip_periodic_t* handle);
int soda_hip_periodic_info(soda_hip_periodic_t* handle,
                           soda_hip_periodic_info_t* info);
/* The primitive: refills the ghost frame of `count` caller-owned padded device
 * arrays in place, array i with the cells of the program's output i (count <=
 * num_outputs), each aligned to its cell size.  One launch per cell size
 * among them -- one in all for a program of one cell type.  Reads interior
 * cells only, writes ghost cells only.  Asynchronous on `stream`, never
 * allocates, capturable as it stands. */
int soda_hip_periodic_fill(soda_hip_periodic_t* handle, void* const* arrays,
                           int32_t count, void* stream);
/* `iterate` iterations on PADDED device arrays; the state stays padded and
 * device-resident across calls.  `inputs` (the num_inputs tensors, then the
 * param arrays, which pass through unchanged) arrive WRAPPED, `outputs` leave
 * wrapped, the inputs are never written.  Chunks of k iterations (the last
 * may be shorter) go through soda_hip_run_device on P, a fill behind each;
 * they ping-pong between `outputs` and one scratch set of the handle so that
 * the last chunk lands in `outputs`.  The device entry contract holds on the
 * padded arrays.  Under "Streams, scratch, graphs": asynchronous on `stream`,
 * never allocates in the handle; the PROGRAM's own scratch is sized for P by
 * the first call like any soda_hip_run_device on P (and that call calibrates,
 * where the program does), after which the call can be captured.  One queue:
 * the handle shares its program's.  SODA_HIP_ERR_INVALID, nothing launched:
 * iterate < 1, iterate > 1 on a program that cannot iterate. */
int soda_hip_periodic_run_padded(soda_hip_periodic_t* handle,
                                 void* const* outputs,
                                 const void* const* inputs, int32_t iterate,
                                 void* stream);
/* The same on DENSE domain arrays of N: the inputs are padded into scratch
 * (every cell, ghosts included), the loop above runs on scratch, the interior
 * is cropped into `outputs`.  The device entry contract of soda_hip_run_device
 * holds on the dense arrays -- overlap, alignment, inputs never written, no
 * byte outside the outputs -- and so does "Streams, scratch, graphs" as for
 * the entry above.  Every cell of every output is defined. */
int soda_hip_periodic_run_device(soda_hip_periodic_t* handle,
                                 void* const* outputs,
                                 const void* const* inputs, int32_t iterate,
                                 void* stream);

/* -- bordered domains: a border mode per dimension --------- */
/* The padded arrays, handle and entries of the block above with another rule
 * for the ghost frame.  Each dimension d has a mode; with g = ghost_lo[d] and
 * j = i - g, padded index i takes interior index g + m(j) along d:
 *   WRAP       j mod N                                   (numpy `wrap`)
 *   CLAMP      min(max(j, 0), N - 1)                     (`edge`)
 *   MIRROR     t = j mod 2N;  t < N ? t : 2N - 1 - t     (`symmetric`)
 *   MIRROR101  N == 1: 0; else t = j mod (2N - 2);
 *              t < N ? t : 2N - 2 - t                    (`reflect`)
 *   CONSTANT   none: a cell with j outside [0, N) takes the tensor's constant
 * (`mod` the mathematical modulo; a frame wider than the domain bounces more
 * than once).  The map is separable: a cell outside in ANY constant dimension
 * takes the constant, every other cell the interior cell given by the maps of
 * all dimensions at once.  An array whose ghost cells all hold that is
 * EXTENDED.  A run of `iterate` iterations lets every iteration see its inputs
 * extended over the window of ONE iteration: only a wrapped ghost evolves into
 * the wrap of the evolved interior, so with any other mode in any dimension
 * the frame is refilled after every iteration (refill_every resolves to 1).
 * With every dimension WRAP the request is the torus above, at its own
 * refill_every, bit for bit.
 * Residuals, norms and runs until converged: the block "residual, norms and
 * run_until on a domain" below.
 * Batches of bordered domains: the block "batched domains" below.
 * Not served on a bordered domain: slabs, groups, ranks, the wire format,
 * `border: preserve`. */
#define SODA_HIP_BORDER_WRAP 0
#define SODA_HIP_BORDER_CLAMP 1
#define SODA_HIP_BORDER_MIRROR 2
#define SODA_HIP_BORDER_MIRROR101 3
#define SODA_HIP_BORDER_CONSTANT 4
typedef struct soda_hip_border_desc {
  soda_hip_periodic_desc_t domain;     /* extent, refill_every (0 or 1 unless
                                          every mode is WRAP), the ghosts of
                                          refill_every iterations, preserve,
                                          not_iterable: as above */
  int32_t mode[SODA_HIP_MAX_DIM];      /* SODA_HIP_BORDER_* per dimension */
  int32_t reserved;
  uint64_t constant[SODA_HIP_MAX_TENSORS];  /* per INPUT tensor: the cell's bit
                                          pattern in the low bytes.  Output o's
                                          ghost takes the constant of input o,
                                          the input it replaces when the
                                          program iterates.  Bits are moved,
                                          never computed with */
} soda_hip_border_desc_t;
/* The fill on a host array, in plain C++ (no GPU, no allocation):
 * soda_hip_wrap_host with a mode per dimension and one constant. */
int soda_hip_extend_host(void* array, int32_t elem_bytes, int32_t dim,
                         const int32_t* extent, const int32_t* ghost_lo,
                         const int32_t* ghost_hi, const int32_t* modes,
                         uint64_t constant);
/* soda_hip_periodic_plan for a bordered domain.  Pure function.  With every
 * mode WRAP it IS soda_hip_periodic_plan on desc->domain.  Otherwise
 * refill_every resolves to 1, every chunk is 1 iteration, and on top of that
 * function's refusals:
 *   SODA_HIP_ERR_INVALID      a mode that is none of SODA_HIP_BORDER_*;
 *                             refill_every > 1 with a mode other than WRAP. */
int soda_hip_border_plan(const soda_hip_plan_t* plan,
                         const soda_hip_border_desc_t* desc, int32_t iterate,
                         soda_hip_periodic_info_t* info, int32_t capacity,
                         int32_t* chunks, int32_t* count);
/* A handle over `program` for ONE bordered domain.  code[i] / code_size[i]:
 * the code object of the EXTEND module (codegen/hip/extend.py) of 1 << i byte
 * cells and the program's dimension count, i = 0..3; needed for every cell
 * size among the program's inputs and outputs, NULL elsewhere.  All scratch of
 * the handle is allocated here.  A refusal (soda_hip_border_plan's, or a
 * program on wire-format banks: SODA_HIP_ERR_UNSUPPORTED) launches nothing
 * and allocates nothing.  The handle must be destroyed before its program. */
typedef struct soda_hip_periodic soda_hip_border_t;  /* opaque: the handle of
                                          the block above, which keeps its
                                          modes */
int soda_hip_border_create(soda_hip_program_t* program,
                           const soda_hip_border_desc_t* desc,
                           const void* const* code, const size_t* code_size,
                           soda_hip_border_t** handle);
int soda_hip_border_destroy(soda_hip_border_t* handle);
int soda_hip_border_info(soda_hip_border_t* handle,
                         soda_hip_periodic_info_t* info);
/* The primitive: refills the ghost frame of `count` caller-owned padded device
 * arrays in place, array i with the cells and the constant of the program's
 * output i (count <= num_outputs), each aligned to its cell size.  One launch
 * per cell size among them -- one in all for a program of one cell type.
 * Reads interior cells only, writes ghost cells only.  Asynchronous on
 * `stream`, never allocates, capturable as it stands. */
int soda_hip_border_fill(soda_hip_border_t* handle, void* const* arrays,
                         int32_t count, void* stream);
/* `iterate` iterations on PADDED device arrays; the state stays padded and
 * device-resident across calls.  `inputs` (the num_inputs tensors, then the
 * param arrays, which pass through unchanged) arrive EXTENDED, `outputs` leave
 * extended, the inputs are never written.  Chunks of k iterations (the last
 * may be shorter) go through soda_hip_run_device on P, a fill behind each;
 * they ping-pong between `outputs` and one scratch set of the handle so that
 * the last chunk lands in `outputs`.  The device entry contract holds on the
 * padded arrays.  Under "Streams, scratch, graphs": asynchronous on `stream`,
 * never allocates in the handle; the PROGRAM's own scratch is sized for P by
 * the first call like any soda_hip_run_device on P (and that call calibrates,
 * where the program does), after which the call can be captured.  One queue:
 * the handle shares its program's.  SODA_HIP_ERR_INVALID, nothing launched:
 * iterate < 1, iterate > 1 on a program that cannot iterate. */
int soda_hip_border_run_padded(soda_hip_border_t* handle, void* const* outputs,
                               const void* const* inputs, int32_t iterate,
                               void* stream);
/* The same on DENSE domain arrays of N: the inputs are padded into scratch
 * (every cell, ghosts included), the loop above runs on scratch, the interior
 * is cropped into `outputs`.  The device entry contract of soda_hip_run_device
 * holds on the dense arrays -- overlap, alignment, inputs never written, no
 * byte outside the outputs -- and so does "Streams, scratch, graphs" as for
 * the entry above.  Every cell of every output is defined. */
int soda_hip_border_run_device(soda_hip_border_t* handle, void* const* outputs,
                               const void* const* inputs, int32_t iterate,
                               void* stream);

/* -- batched domains: many tori or bordered grids at once -- */
/* The two blocks above over `batch` independent domains of ONE extent, for a
 * program whose plan is batched (LowerOptions.batch): every array -- the
 * caller's dense or padded ones, the handle's scratch -- is `batch` items one
 * behind the other like a contiguous [batch, ...] array, every item is wrapped
 * or extended on its own, and each chunk, fill, pad and crop is ONE launch per
 * kernel for all items (the helper kernels' `_bt` forms take the item from
 * blockIdx.z; the program's kernels run as in soda_hip_run_device_batch).
 * Per item the semantics and the bits are those of an unbatched handle on
 * that item alone.  Param arrays are shared by all items.
 *
 * The plan entries: pure functions.  P, the ghosts, k and the chunks are what
 * soda_hip_periodic_plan / soda_hip_border_plan give for the same plan built
 * without `batch`; scratch_bytes is that figure times `batch`; the geometry is
 * checked by soda_hip_plan_geometry_batch on P.  They refuse what those
 * entries refuse, but for a batched plan, and with SODA_HIP_ERR_INVALID:
 * `batch` outside 1..SODA_HIP_MAX_BATCH, a plan that is not batched (the
 * entries never fall back to a loop of launches). */
int soda_hip_periodic_plan_batch(const soda_hip_plan_t* plan,
                                 const soda_hip_periodic_desc_t* desc,
                                 int32_t batch, int32_t iterate,
                                 soda_hip_periodic_info_t* info,
                                 int32_t capacity, int32_t* chunks,
                                 int32_t* count);
int soda_hip_border_plan_batch(const soda_hip_plan_t* plan,
                               const soda_hip_border_desc_t* desc,
                               int32_t batch, int32_t iterate,
                               soda_hip_periodic_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count);
/* A handle of the types above, fixed to one (extent, batch).  code[i]: the
 * code object of the BATCHED wrap resp. extend module (codegen/hip/wrap.py,
 * extend.py with batch=True) of 1 << i byte cells.  All scratch -- [batch,
 * P...] per array -- is allocated here; a refusal (the plan entries') launches
 * and allocates nothing.
 * soda_hip_<kind>_info, _fill, _run_padded, _run_device and _destroy serve
 * such a handle under their contracts as written, each array taken as `batch`
 * items long: the device entry contract on the whole arrays, asynchronous,
 * never allocating in the handle, capturable after the first eager call (which
 * sizes the program's scratch and calibrates for (P, batch)).
 * SODA_HIP_ERR_UNSUPPORTED on such a handle, nothing launched:
 * _run_padded_residual, _run_padded_norms, _run_until, _run_until_norm (the
 * residual of a batch is not served).  soda_hip_border_fused_* has no batched
 * form and keeps refusing a batched plan. */
int soda_hip_periodic_create_batch(soda_hip_program_t* program,
                                   const soda_hip_periodic_desc_t* desc,
                                   int32_t batch,
                                   const void* const* wrap_code,
                                   const size_t* wrap_code_size,
                                   soda_hip_periodic_t** handle);
int soda_hip_border_create_batch(soda_hip_program_t* program,
                                 const soda_hip_border_desc_t* desc,
                                 int32_t batch, const void* const* code,
                                 const size_t* code_size,
                                 soda_hip_border_t** handle);

/* -- bordered domains, fused away from the walls ----------- */
/* The block above advances one iteration per launch.  Here a chunk of n <= T
 * iterations (T: the depth) takes an extended state S to the extended S':
 *   interior  n iterations of the ordinary kernels on P, fused as deep as the
 *             plan allows.  With a frame of ONE iteration's reach in a wall
 *             dimension every domain cell at least (n - 1) x reach_lo from a
 *             low wall and (n - 1) x reach_hi from a high wall comes out right;
 *             a WRAP dimension, whose frame carries T iterations, is right
 *             over its whole width.
 *   strips    per wall dimension d whose reach is not zero ONE strip: a
 *             bordered domain of the block above, with the request's modes and
 *             constants, of extent N with N[d] replaced by L + H -- the
 *             domain's cells [0, L) and [N[d] - H, N[d]) side by side,
 *             L = H = T x (reach_lo[d] + reach_hi[d]).  It is gathered from S,
 *             advanced n iterations one at a time, and its cells
 *             [0, take_lo) and [L + H - take_hi, L + H) along d,
 *             take = (T - 1) x reach, are scattered into the interior's
 *             result; they are clear of the false neighbours in the strip's
 *             middle for every n <= T.
 *   fill      one ordinary fill of the frame of P.
 * All on the one stream, in that order.  Every cell is computed by the same
 * expression from the same values as in the block above: the result equals
 * soda_hip_border_run_* bit for bit, whatever the depth.
 * The depth resolves to 1 -- and the handle is the block above's -- when it is
 * given as 1, when the program cannot iterate, or when some wall dimension
 * has N[d] < L + H.  With every mode WRAP the handle is the torus at
 * refill_every = depth. */
typedef struct soda_hip_border_fused_desc {
  soda_hip_border_desc_t border;       /* as above; domain.refill_every 0 or 1
                                          (the depth takes its place);
                                          ghost_lo / ghost_hi: at least reach in
                                          a wall dimension, depth x reach in a
                                          WRAP dimension */
  int32_t depth;                       /* T; 0: the largest fused_iters of the
                                          plan's passes */
  int32_t reach_lo[SODA_HIP_MAX_DIM];  /* cells ONE iteration reaches below ... */
  int32_t reach_hi[SODA_HIP_MAX_DIM];  /* ... and above a cell, the most over
                                          all outputs (the caller's to compute:
                                          Stencil.window_bounds(1)); with
                                          plan->has_reach, along the last
                                          dimension at least the plan's reach */
  int32_t reserved;
} soda_hip_border_fused_desc_t;
typedef struct soda_hip_border_strip {
  int32_t dim;                         /* the wall dimension d */
  int32_t lo, hi;                      /* L, H */
  int32_t take_lo, take_hi;            /* cells along d the scatter takes at
                                          the low / the high wall */
  int32_t reserved;
  int32_t extent[SODA_HIP_MAX_DIM];    /* N with N[d] = L + H */
  soda_hip_periodic_info_t info;       /* the strip's own handle: ghosts (the
                                          request's; [0] as rounded for this
                                          extent), padded extent, scratch */
} soda_hip_border_strip_t;
typedef struct soda_hip_border_fused_info {
  soda_hip_periodic_info_t main;       /* the handle on N; refill_every: 1, or
                                          the depth on a torus */
  int32_t depth;                       /* T as resolved */
  int32_t num_strips;                  /* 0 at depth 1 and on a torus */
  soda_hip_border_strip_t strip[SODA_HIP_MAX_DIM];  /* by rising dimension */
  int64_t scratch_bytes;               /* main and strips together */
} soda_hip_border_fused_info_t;
/* The box mover on host arrays, in plain C++ (no GPU, no allocation): box b
 * copies size[b * dim + d] cells per dimension from `src` (dense,
 * dim-0-fastest, of src_extent) at src_origin[b * dim + d] to `dst` (of
 * dst_extent) at dst_origin[b * dim + d].  A box with a size of 0 is empty.
 * The arrays must not overlap.  SODA_HIP_ERR_INVALID, nothing written: a cell
 * size other than 1, 2, 4 or 8 bytes, dim outside 1..4, a negative size or
 * origin, a box that leaves either array. */
int soda_hip_box_host(void* dst, const int32_t* dst_extent, const void* src,
                      const int32_t* src_extent, int32_t elem_bytes,
                      int32_t dim, int32_t num_boxes,
                      const int32_t* dst_origin, const int32_t* src_origin,
                      const int32_t* size);
/* soda_hip_border_plan for the fused form: *info, and the iterations of every
 * chunk -- the depth each, the last may be shorter -- in chunks[0, *count).
 * Pure function.  Refuses what soda_hip_border_plan refuses, on N and on every
 * strip's extent, and:
 *   SODA_HIP_ERR_INVALID      depth < 0; a negative reach; with
 *                             plan->has_reach, a reach along the last
 *                             dimension below the plan's; a frame narrower than
 *                             reach in a wall dimension or than depth x reach
 *                             in a WRAP dimension. */
int soda_hip_border_fused_plan(const soda_hip_plan_t* plan,
                               const soda_hip_border_fused_desc_t* desc,
                               int32_t iterate,
                               soda_hip_border_fused_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count);
/* A handle over `program` for ONE bordered domain, fused.  code / code_size:
 * the EXTEND modules as for soda_hip_border_create; box_code / box_code_size:
 * the BOX modules (codegen/hip/box.py) likewise, needed where the plan has
 * strips.  All scratch is allocated here, the strips' included.  A refusal
 * launches nothing and allocates nothing.  The handle must be destroyed before
 * its program. */
typedef struct soda_hip_border_fused soda_hip_border_fused_t;   /* opaque */
int soda_hip_border_fused_create(soda_hip_program_t* program,
                                 const soda_hip_border_fused_desc_t* desc,
                                 const void* const* code,
                                 const size_t* code_size,
                                 const void* const* box_code,
                                 const size_t* box_code_size,
                                 soda_hip_border_fused_t** handle);
int soda_hip_border_fused_destroy(soda_hip_border_fused_t* handle);
int soda_hip_border_fused_info(soda_hip_border_fused_t* handle,
                               soda_hip_border_fused_info_t* info);
/* The primitive: the two boxes of strip `strip` (0 .. num_strips - 1) between
 * `count` caller-owned padded device arrays on either side, pair i with the
 * cells of the program's output i (count <= num_outputs), each aligned to its
 * cell size: main_arrays of P, strip_arrays of the strip's padded extent.
 * gather != 0: the domain's cells [0, L) and [N[d] - H, N[d]) along the
 * strip's dimension, over the whole domain elsewhere, from main_arrays into
 * the strip's domain; gather == 0, the scatter: the strip's cells
 * [0, take_lo) and [L + H - take_hi, L + H) into the domain's two rims in
 * main_arrays.  Frames are neither read nor written.  One launch per cell
 * size among the arrays.  Asynchronous on `stream`, never allocates,
 * capturable as it stands. */
int soda_hip_border_fused_move(soda_hip_border_fused_t* handle, int32_t strip,
                               int32_t gather, void* const* main_arrays,
                               void* const* strip_arrays, int32_t count,
                               void* stream);
/* soda_hip_border_run_padded / _run_device in chunks of the depth, under the
 * same contracts: asynchronous on `stream`, the inputs never written, the
 * device entry contract on the caller's arrays, param arrays passed through,
 * never allocating in the handle.  The PROGRAM's scratch is sized by the first
 * call for P and for every strip's extent (and that call calibrates, where the
 * program does), after which the call can be captured.  One queue, no side
 * streams. */
int soda_hip_border_fused_run_padded(soda_hip_border_fused_t* handle,
                                     void* const* outputs,
                                     const void* const* inputs,
                                     int32_t iterate, void* stream);
int soda_hip_border_fused_run_device(soda_hip_border_fused_t* handle,
                                     void* const* outputs,
                                     const void* const* inputs,
                                     int32_t iterate, void* stream);

/* -- residual, norms and run_until on a domain ------------- */
/* The residual of soda_hip_run_device_residual and the norms of
 * soda_hip_run_device_norms with the DOMAIN in place of the open box: a run of
 * n iterations on a handle of domain extent N pairs every output with the
 * input it replaces, `cur` the output after n iterations, `prev` the output
 * after n - 1 (the caller's input when n = 1), and counts all N cells of every
 * pair -- under these handles every cell is defined; no ghost cell is counted.
 * Per-cell delta, fields and words are unchanged, so every number is again a
 * sum or a maximum of exact per-cell values and equals the CPU's.
 *
 * Torus, and walls at depth 1: the last chunk of the run takes the residual
 * with the interior [ghost_lo, ghost_lo + N) of the padded arrays as its box,
 * as soda_hip_run_device_residual takes it -- in the twin of the deepest
 * scheduled pass that has one, else by `<app>_residual` behind the
 * one-iteration pass; norms always that second way.
 * Fused walls: the interior launch is wrong near the walls and the strips mend
 * it, so each cell is counted where it is made right, by a partition of the
 * domain that follows from the plan's numbers (T the depth, a / b the reach of
 * one iteration below / above, whatever the last chunk's length):
 *   trusted   [(T-1) a[d], N[d] - (T-1) b[d]) in every wall dimension d, all of
 *             [0, N[d]) in a WRAP dimension: counted by the interior run;
 *   rims      per strip (wall dimension d) the cells it scatters, the low and
 *             the high rim, cut to the trusted interval in every wall
 *             dimension e < d, whole in every other dimension: counted behind
 *             the strip's last iteration by `<app>_residual` / the norms
 *             kernel on the strip's own padded arrays (cur: the strip's
 *             result, prev: its state one iteration earlier), one launch per
 *             non-empty box, added into the same struct.
 * The struct is zeroed once, ahead of the last chunk's gather; then strips
 * (rims behind each), interior, scatter, fill: one stream, no side streams.
 * soda_hip_border_fused_residual_boxes gives the partition (pure function). */
typedef struct soda_hip_border_rims {
  int32_t dim;                         /* the strip's wall dimension d */
  int32_t reserved;
  int32_t lo[2][SODA_HIP_MAX_DIM];     /* [0] the low rim, [1] the high rim: */
  int32_t hi[2][SODA_HIP_MAX_DIM];     /* [lo, hi) per dimension of the STRIP's
                                          padded arrays; lo == hi somewhere: an
                                          empty rim (a one-sided program) */
} soda_hip_border_rims_t;
typedef struct soda_hip_border_fused_boxes {
  int32_t depth;                       /* T as resolved */
  int32_t num_strips;                  /* 0 at depth 1 and on a torus: the
                                          trusted box is the whole domain */
  int32_t trusted_lo[SODA_HIP_MAX_DIM];   /* [lo, hi) per dimension of the */
  int32_t trusted_hi[SODA_HIP_MAX_DIM];   /* domain's padded arrays of P */
  soda_hip_border_rims_t strip[SODA_HIP_MAX_DIM];   /* by rising dimension */
} soda_hip_border_fused_boxes_t;
/* The partition for `plan` and `desc` (desc->border.domain.extent is N).  Pure
 * function (no GPU, no program); refuses what soda_hip_border_fused_plan
 * refuses.  The boxes are pairwise disjoint and their union, each moved back
 * to the domain, is the domain. */
int soda_hip_border_fused_residual_boxes(
    const soda_hip_plan_t* plan, const soda_hip_border_fused_desc_t* desc,
    soda_hip_border_fused_boxes_t* boxes);
/* <handle>_run_padded that also leaves the residual of its last iteration in
 * the caller's 32 device bytes `residual_dev` (8-byte aligned, no byte shared
 * with a padded output) / the norms in the soda_hip_norms_t at `acc_dev`.  The
 * contracts of <handle>_run_padded hold: inputs arrive extended, outputs leave
 * extended, inputs are never written, asynchronous on `stream`; the struct is
 * zeroed inside the call by a kernel node, and the call can be captured after
 * the first eager call -- every replay zeroes and refills the struct.
 * Nothing launched: SODA_HIP_ERR_UNSUPPORTED for a program built without
 * `residual`, and for norms on pairs of another cell kind or size than the
 * norms handle's; SODA_HIP_ERR_INVALID for iterate < 1, iterate > 1 on a
 * program that cannot iterate, a struct that is misaligned or overlaps an
 * output, a norms handle of another dimension count or device. */
int soda_hip_periodic_run_padded_residual(soda_hip_periodic_t* handle,
                                          void* const* outputs,
                                          const void* const* inputs,
                                          int32_t iterate, void* residual_dev,
                                          void* stream);
int soda_hip_periodic_run_padded_norms(soda_hip_periodic_t* handle,
                                       soda_hip_norms_handle_t* norms,
                                       void* const* outputs,
                                       const void* const* inputs,
                                       int32_t iterate, void* acc_dev,
                                       void* stream);
int soda_hip_border_run_padded_residual(soda_hip_border_t* handle,
                                        void* const* outputs,
                                        const void* const* inputs,
                                        int32_t iterate, void* residual_dev,
                                        void* stream);
int soda_hip_border_run_padded_norms(soda_hip_border_t* handle,
                                     soda_hip_norms_handle_t* norms,
                                     void* const* outputs,
                                     const void* const* inputs,
                                     int32_t iterate, void* acc_dev,
                                     void* stream);
int soda_hip_border_fused_run_padded_residual(soda_hip_border_fused_t* handle,
                                              void* const* outputs,
                                              const void* const* inputs,
                                              int32_t iterate,
                                              void* residual_dev, void* stream);
int soda_hip_border_fused_run_padded_norms(soda_hip_border_fused_t* handle,
                                           soda_hip_norms_handle_t* norms,
                                           void* const* outputs,
                                           const void* const* inputs,
                                           int32_t iterate, void* acc_dev,
                                           void* stream);
/* soda_hip_run_device_until / _until_norm on a domain: DENSE device arrays of
 * N, the device entry contract on them, arguments and stop rules of those two
 * entries.  SYNCHRONOUS, not for a stream that is being captured.  The inputs
 * are padded once into the handle's scratch, chunks of `check_every`
 * iterations (the last may be shorter) run on padded scratch through the
 * entries above -- the first from the padded inputs into the padded outputs,
 * every later one back into the set the one before it read, which is free by
 * then -- the struct is fetched after each chunk, and the interior of the
 * final state is cropped into `outputs`.  The handle allocates nothing for it
 * (the struct fetched lives in the program's scratch).  Refusals as above,
 * and max_iterate < 1, check_every < 1, max_iterate > 1 on a program that
 * cannot iterate: SODA_HIP_ERR_INVALID. */
int soda_hip_periodic_run_until(soda_hip_periodic_t* handle,
                                void* const* outputs,
                                const void* const* inputs, int32_t max_iterate,
                                int32_t check_every, double tol,
                                uint64_t int_tol,
                                soda_hip_residual_t* result_host,
                                int32_t* iterations_done, void* stream);
int soda_hip_periodic_run_until_norm(soda_hip_periodic_t* handle,
                                     soda_hip_norms_handle_t* norms,
                                     void* const* outputs,
                                     const void* const* inputs,
                                     int32_t max_iterate, int32_t check_every,
                                     int32_t which, double tol,
                                     soda_hip_norms_t* result_host,
                                     int32_t* iterations_done, void* stream);
int soda_hip_border_run_until(soda_hip_border_t* handle, void* const* outputs,
                              const void* const* inputs, int32_t max_iterate,
                              int32_t check_every, double tol, uint64_t int_tol,
                              soda_hip_residual_t* result_host,
                              int32_t* iterations_done, void* stream);
int soda_hip_border_run_until_norm(soda_hip_border_t* handle,
                                   soda_hip_norms_handle_t* norms,
                                   void* const* outputs,
                                   const void* const* inputs,
                                   int32_t max_iterate, int32_t check_every,
                                   int32_t which, double tol,
                                   soda_hip_norms_t* result_host,
                                   int32_t* iterations_done, void* stream);
int soda_hip_border_fused_run_until(soda_hip_border_fused_t* handle,
                                    void* const* outputs,
                                    const void* const* inputs,
                                    int32_t max_iterate, int32_t check_every,
                                    double tol, uint64_t int_tol,
                                    soda_hip_residual_t* result_host,
                                    int32_t* iterations_done, void* stream);
int soda_hip_border_fused_run_until_norm(soda_hip_border_fused_t* handle,
                                         soda_hip_norms_handle_t* norms,
                                         void* const* outputs,
                                         const void* const* inputs,
                                         int32_t max_iterate,
                                         int32_t check_every, int32_t which,
                                         double tol,
                                         soda_hip_norms_t* result_host,
                                         int32_t* iterations_done,
                                         void* stream);

/* -- bordered domains: a mode and a constant per FACE ------ */
/* The bordered blocks above give a dimension's low and high wall one mode and
 * every `constant` wall of a tensor one value.  This extension lifts both:
 * every dimension d has a mode for its LOW face (desc->mode[d]) and one for its
 * HIGH face (faces->mode_hi[d]), every input tensor a constant per face.  With
 * g = ghost_lo[d], j = i - g and m_X the closed form of mode X as stated under
 * "bordered domains", padded index i takes m_lo(j) where j < 0, m_hi(j) where
 * j >= N, and j elsewhere (the forms are total: a frame wider than the domain
 * bounces as before).  CONSTANT as a face mode means none: the cell takes a
 * constant.  WRAP is served as the pair (WRAP, WRAP) only.
 * The map stays separable, with one rule for the constants: a ghost cell that
 * is outside through a CONSTANT face in one or more dimensions takes the
 * constant of the HIGHEST such dimension, and of that face; every other ghost
 * cell takes the interior cell given by the maps of all dimensions at once.
 * That is what extending the array dimension by dimension gives, dimension 0
 * first, each dimension's two sides taken from the array as it stood before
 * that dimension.
 * A wall dimension is one whose faces are not (WRAP, WRAP): it keeps a frame
 * of one iteration's reach, refilled after every iteration.  The output's
 * ghost takes the constants of the input it replaces.  Bits are moved, never
 * computed with.
 * Only a CONSTANT face ever shows its constant, so a tensor's constants count
 * as equal where those of its CONSTANT faces are.
 * A request whose faces are equal pairwise and whose constants are equal per
 * tensor -- and faces == NULL -- is the request of the blocks above: every
 * `_faces` entry below then IS the entry it is named after, with its
 * launches, its kernels (the extend module's) and its scratch.  Only an
 * asymmetric request loads and launches the FACES module
 * (codegen/hip/faces.py; soda_faces_e<bytes>_d<dim>, `_bt` on a batch). */
typedef struct soda_hip_border_faces {
  int32_t mode_hi[SODA_HIP_MAX_DIM];   /* SODA_HIP_BORDER_* of the HIGH face per
                                          dimension; desc->mode[] is the LOW
                                          face */
  int32_t per_face_constants;          /* 0: desc->constant[] on every face */
  int32_t reserved[3];
  uint64_t constant[SODA_HIP_MAX_TENSORS][SODA_HIP_MAX_DIM][2];
                                       /* [input][dimension][0 low, 1 high]: the
                                          cell's bit pattern in the low bytes */
} soda_hip_border_faces_t;             /* soda_hip_sizeof(22) */
/* soda_hip_extend_host with a mode per face and a constant per (dimension,
 * side): constants[2 * d + side].  With equal pairs and one constant it is
 * soda_hip_extend_host.  SODA_HIP_ERR_INVALID, the array untouched: a mode
 * that is none of SODA_HIP_BORDER_*, a dimension that wraps on one face. */
int soda_hip_extend_faces_host(void* array, int32_t elem_bytes, int32_t dim,
                               const int32_t* extent, const int32_t* ghost_lo,
                               const int32_t* ghost_hi,
                               const int32_t* modes_lo,
                               const int32_t* modes_hi,
                               const uint64_t* constants);
/* The twins.  Each has the signature of the entry it is named after plus
 * `faces` (NULL: that entry) behind the desc and, where that entry takes code
 * objects, faces_code[i] / faces_code_size[i] behind them: the code object of
 * the FACES module of 1 << i byte cells and the program's dimension count (the
 * batched one for _create_batch_faces), needed for every cell size among the
 * program's inputs and outputs when the request is asymmetric, never looked at
 * otherwise (NULL will do); an asymmetric request in turn never looks at
 * `code`, the extend module's.  The handles are those of the blocks above, and
 * _info, _fill, _run_padded, _run_device, _run_padded_residual,
 * _run_padded_norms, _run_until, _run_until_norm and _destroy serve them under
 * their contracts as written.  The geometry -- ghosts, padded extent, chunks,
 * depth, strips, residual boxes -- is that of the symmetric request with the
 * same wall dimensions; a strip of the fused form is a bordered domain with
 * the request's faces and constants.  On top of the refusals of the entries
 * they are named after, nothing launched and nothing allocated:
 *   SODA_HIP_ERR_INVALID      a dimension that wraps on one face only;
 *                             a face mode that is none of SODA_HIP_BORDER_*;
 *                             refill_every > 1 unless every pair is
 *                             (WRAP, WRAP).
 * A batched faces handle refuses residuals, norms and runs until converged
 * like every batched handle (SODA_HIP_ERR_UNSUPPORTED), the fused twins a
 * batched plan. */
int soda_hip_border_plan_faces(const soda_hip_plan_t* plan,
                               const soda_hip_border_desc_t* desc,
                               const soda_hip_border_faces_t* faces,
                               int32_t iterate, soda_hip_periodic_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count);
int soda_hip_border_plan_batch_faces(const soda_hip_plan_t* plan,
                                     const soda_hip_border_desc_t* desc,
                                     const soda_hip_border_faces_t* faces,
                                     int32_t batch, int32_t iterate,
                                     soda_hip_periodic_info_t* info,
                                     int32_t capacity, int32_t* chunks,
                                     int32_t* count);
int soda_hip_border_create_faces(soda_hip_program_t* program,
                                 const soda_hip_border_desc_t* desc,
                                 const soda_hip_border_faces_t* faces,
                                 const void* const* code,
                                 const size_t* code_size,
                                 const void* const* faces_code,
                                 const size_t* faces_code_size,
                                 soda_hip_border_t** handle);
int soda_hip_border_create_batch_faces(soda_hip_program_t* program,
                                       const soda_hip_border_desc_t* desc,
                                       const soda_hip_border_faces_t* faces,
                                       int32_t batch, const void* const* code,
                                       const size_t* code_size,
                                       const void* const* faces_code,
                                       const size_t* faces_code_size,
                                       soda_hip_border_t** handle);
int soda_hip_border_fused_plan_faces(const soda_hip_plan_t* plan,
                                     const soda_hip_border_fused_desc_t* desc,
                                     const soda_hip_border_faces_t* faces,
                                     int32_t iterate,
                                     soda_hip_border_fused_info_t* info,
                                     int32_t capacity, int32_t* chunks,
                                     int32_t* count);
int soda_hip_border_fused_create_faces(
    soda_hip_program_t* program, const soda_hip_border_fused_desc_t* desc,
    const soda_hip_border_faces_t* faces, const void* const* code,
    const size_t* code_size, const void* const* box_code,
    const size_t* box_code_size, const void* const* faces_code,
    const size_t* faces_code_size, soda_hip_border_fused_t** handle);
int soda_hip_border_fused_residual_boxes_faces(
    const soda_hip_plan_t* plan, const soda_hip_border_fused_desc_t* desc,
    const soda_hip_border_faces_t* faces,
    soda_hip_border_fused_boxes_t* boxes);
/* A/B runs only: with SODA_HIP_FACES_FORCE=1 in the environment (read once per
 * handle, when it is made) a `_create*_faces` entry that is given the faces
 * module serves a SYMMETRIC request with the faces kernels as well -- the same
 * bits, the other kernel (tools/faces_ab.py). */

/* Replaces soda::app::<app>(): host arrays described by (ptr, extent, stride,
 * min) per tensor, inputs then outputs; copies in, runs, copies the outputs
 * back, synchronises.  Strides are in elements; every tensor must share one
 * extent. */
typedef struct soda_hip_host_tensor {
  void* ptr;
  const int32_t* extent;
  const int32_t* stride;
  const int32_t* min;      /* accepted, unused (as in the reference) */
} soda_hip_host_tensor_t;
/* `inputs`: the num_inputs tensors, then one entry per param array of which
 * only `ptr` is read (param_elems[k] contiguous elements). */
int soda_hip_run_host(soda_hip_program_t* program,
                      const soda_hip_host_tensor_t* inputs,
                      const soda_hip_host_tensor_t* outputs, int32_t iterate);
/* Same, but only box [valid_lo, valid_hi) of each output (num_outputs x dim
 * values each, NULL = whole array) is written to the caller's array, which is
 * what the reference's gather loop does with its compiled-in stencil offsets
 * (frt/host.py:357-375). */
int soda_hip_run_host_box(soda_hip_program_t* program,
                          const soda_hip_host_tensor_t* inputs,
                          const soda_hip_host_tensor_t* outputs,
                          int32_t iterate, const int32_t* valid_lo,
                          const int32_t* valid_hi);
/* How the two entries above move data (soda_host.cpp): through pinned staging
 * slots the program owns, ~16 MiB chunks along the last dimension
 * (SODA_HIP_HOST_CHUNK_MB), packed / unpacked by a process-wide pool of worker
 * threads (SODA_HIP_HOST_THREADS, default 8 -- the reference's pack and unpack
 * loops carry `#pragma omp parallel for`, frt/host.py:193,357) while the DMA
 * engine moves the neighbouring chunk.  With the program's per-iteration reach
 * in the plan (has_reach) a 2-D / 3-D run is cut into bands along the last
 * dimension -- window runs with iterate x reach ghost rows -- where a timeline
 * estimate of copy-in / kernels / copy-out says the overlap wins
 * (SODA_HIP_HOST_BANDS=0: never, =1: by a fixed rule; SODA_HIP_HOST_TRACE=1
 * prints the estimates and where the host thread's time went).  Slots and
 * worker threads live on the GPU's NUMA node (SODA_HIP_HOST_NUMA=0: wherever
 * the scheduler puts them).  A dense tensor inside a range pinned with
 * soda_hip_host_register skips the slots and the threads: its rows go by DMA
 * from / to the caller's array (an output whose box does not hold whole rows
 * by one strided copy per chunk).  SODA_HIP_HOST_DIRECT=0: never;
 * =attributes: also memory the HIP runtime reports as host-pinned
 * (hipHostMalloc, a hipHostRegister of the caller's) -- at the caller's risk:
 * a registration that is stale or not writable faults the GPU.  Results are
 * the same bits either way.
 * The pack / unpack step alone, exported
 * for callers that stage their own transfers and for tests without a GPU:
 * copies box [lo, hi) between a strided host array (strides in elements) and
 * a dense array that starts at index `row0` of the last dimension (0: holds
 * the whole array); to_dense != 0: strided -> dense.  threads: 1 = the calling
 * thread only, 0 = the pool. */
int soda_hip_host_copy_box(void* strided, const int32_t* stride, void* dense,
                           const int32_t* extent, const int32_t* lo,
                           const int32_t* hi, int32_t dim, int32_t elem,
                           int32_t to_dense, int32_t row0, int32_t threads);
/* The pack / unpack step of a tensor dealt over DRAM banks (the wire format's
 * streams, below: element k in bank k % num_banks at index k / num_banks;
 * reference docs/data-layout.md "Multi-Bank", frt/host.py:241-246,422-424):
 * stream elements [first, first + count) <-> a dense run starting at `dense`;
 * first and count multiples of num_banks.  What soda_hip_stream_run_host does
 * with banked tensors on its way through the staging slots; exported for
 * tests without a GPU.  threads as soda_hip_host_copy_box. */
int soda_hip_host_weave_banks(void* const* banks, int32_t num_banks, void* dense,
                              int64_t first, int64_t count, int32_t elem,
                              int32_t to_dense, int32_t threads);
/* Pins [ptr, ptr + bytes) of the caller's memory (hipHostRegister) so that
 * soda_hip_run_host / soda_hip_run_host_box reach it by DMA where it is -- for
 * hosts that keep their arrays across calls and do not link HIP themselves.
 * `ptr` must start a page (INVALID otherwise): the reference host's buffers
 * do (aligned_alloc(4096, ...), frt/host.py:165-178); ranges inside malloc's
 * heap share pages with other objects and are not accepted.  Meant for
 * memory that lives long: registering costs about as much as one copy of the
 * range -- once per array, not per call.  Unregister before freeing. */
int soda_hip_host_register(void* ptr, size_t bytes);
int soda_hip_host_unregister(void* ptr);

/* Measures one launch of every pass on `extent` (stand-in arrays; two warming
 * rounds, then four rounds of `launches` back-to-back launches per pass inside
 * HIP events on `stream`, the shortest round counts; synchronises) and
 * remembers the times: later runs on exactly this extent schedule their passes
 * by the clock instead of the model.  Costs milliseconds, once; programs with
 * a single pass have nothing to choose and return at once. */
int soda_hip_program_calibrate(soda_hip_program_t* program,
                               const int32_t* extent, int32_t launches,
                               void* stream);
/* Programs calibrate by themselves: the first run of more than one iteration
 * on an extent (any run entry; only the extent the call names, not the
 * trimmed sub-extents of cone runs) first times the passes on it -- it
 * synchronises `stream` once and costs a few milliseconds -- so that every
 * caller, the generated C++ host included, is scheduled by the clock, not by
 * the model (whose error is ~9 % per pass).  on = 0 turns that off for a
 * program; the environment variable SODA_HIP_NO_CALIBRATE=1 for all.
 * Two kinds of run never calibrate by themselves and stay asynchronous on
 * `stream` as documented: a soda_hip_run_device_slab call that is handed an
 * event (other streams are live beside it: the calibration's allocations and
 * its synchronisation would stall the neighbours' exchange), and any run on a
 * stream that is being captured into a graph.  Calibrate such extents
 * beforehand with soda_hip_program_calibrate, or they run by the model. */
int soda_hip_program_set_auto_calibrate(soda_hip_program_t* program, int on);
/* Time of one launch of every pass on `extent` in ns (num_passes values):
 * measured if calibrated (*measured = 1), else the model's. */
int soda_hip_program_pass_times(soda_hip_program_t* program,
                                const int32_t* extent, float* pass_ns,
                                int32_t* measured);

/* The schedule a run of `iterate` iterations on `extent` uses (num_passes
 * counts), from measured times where calibrated. */
int soda_hip_program_schedule(soda_hip_program_t* program,
                              const int32_t* extent, int32_t iterate,
                              int32_t* count);
/* The three above for launches over `batch` grids of `extent`
 * (soda_hip_run_device_batch; batched programs only, batch in
 * 1..SODA_HIP_MAX_BATCH): times and schedules are remembered per (extent,
 * batch), batch = 1 being the entries above.  A batched run calibrates by
 * itself under the same rules as a one-grid run. */
int soda_hip_program_calibrate_batch(soda_hip_program_t* program,
                                     const int32_t* extent, int32_t batch,
                                     int32_t launches, void* stream);
int soda_hip_program_pass_times_batch(soda_hip_program_t* program,
                                      const int32_t* extent, int32_t batch,
                                      float* pass_ns, int32_t* measured);
int soda_hip_program_schedule_batch(soda_hip_program_t* program,
                                    const int32_t* extent, int32_t batch,
                                    int32_t iterate, int32_t* count);

/* Diagnostics: kernels generated with time stamps (sodac --hip-stamps) write
 * four 64-bit words per wavefront -- s_memtime at entry and exit, HW_ID,
 * XCC_ID -- to this device buffer (slot SODA_HIP_MAX_TENSORS - 1 of the kernel
 * arguments; at least 32 bytes x wavefronts of the largest launch).  NULL
 * (the default) for kernels without stamps. */
int soda_hip_program_set_debug_buffer(soda_hip_program_t* program, void* buf);

/* Number of kernel launches the last run_device/run_host call issued and how
 * many of them used the pass with the largest fused_iters. */
int soda_hip_last_launches(soda_hip_program_t* program, int32_t* launches,
                           int32_t* fused_launches);
/* Passes of the last run that were launched in two parts (boundary chunks /
 * interior) around a halo exchange. */
int soda_hip_last_split(soda_hip_program_t* program, int32_t* passes);
/* Device bytes of scratch the program holds now (locals, ping-pong
 * temporaries) and how many times a call has replaced one of these buffers by
 * a larger one so far -- each time a call that waited for the device.  Either
 * may be NULL. */
int soda_hip_program_scratch(soda_hip_program_t* program, int64_t* bytes,
                             int32_t* regrown);

/* -- one host thread, N GPUs: a grid cut into slabs -------------------------
 * The reference's host is one blocking C++ sequence on one device
 * (frt/host.py:319-322: WriteToDevice, Exec, ReadFromDevice, Finish); its only
 * scale-out is host-side tiling with a replicated halo that is recomputed
 * (frt/host.py:124-128,181-249).  A group is the MI355X form of that host
 * (SURVEY.md 8b "one host thread drives N GPUs (one stream each)", 8e): the
 * LAST dimension -- the one SODA streams -- is cut into one contiguous slab
 * per device; every slab keeps `exchange_every x reach` ghost rows per side,
 * runs that many iterations without communication, then fetches its ghosts
 * from the neighbours' own rows by peer-to-peer copies (xGMI) on a stream of
 * its own while the rows that need no fresh ghost keep computing
 * (soda_hip_run_device_slab).  No collective anywhere.  The result on the
 * global valid box is the single-device result bit for bit.
 *
 * `device[]` may name one GPU several times: such slabs are "virtual devices"
 * that share it (copies between them are plain device copies).  This is how a
 * one-GPU box runs the whole N-slab schedule -- streams, events, overlap. */
#define SODA_HIP_MAX_SLABS 64
#define SODA_HIP_GROUP_NO_OVERLAP 1    /* exchange, then compute: for A/B runs */
#define SODA_HIP_GROUP_CALIBRATE 2     /* time every pass on every slab extent
                                          once (soda_hip_program_calibrate) */

#define SODA_HIP_GROUP_THREADS 4       /* one enqueueing thread per slab inside
                                          the library: the caller still sees one
                                          blocking sequence, but a step of
                                          9 launches x 8 GPUs no longer costs
                                          0.3 ms of ONE thread's time, as long
                                          as the GPUs take to run it */

typedef struct soda_hip_group_desc {
  int32_t num_slabs;
  int32_t device[SODA_HIP_MAX_SLABS];
  int32_t extent[SODA_HIP_MAX_DIM];    /* the whole grid */
  int32_t reach_lo, reach_hi;          /* cells along the last dimension one
                                          iteration reads below / above a cell
                                          (the stencil window's extent there:
                                          ref core.py:876-926) */
  int32_t iterate;                     /* iterations of a typical run: what the
                                          exchange interval is chosen for */
  int32_t exchange_every;              /* iterations between exchanges; 0: the
                                          library picks the interval of least
                                          modelled time from its per-extent
                                          pass times and a transfer model */
  int32_t flags;                       /* SODA_HIP_GROUP_* */
} soda_hip_group_desc_t;

typedef struct soda_hip_slab_info {
  int32_t device;
  int32_t begin, end;                  /* global rows held: own + ghosts */
  int32_t own_begin, own_end;
  int32_t ghost_lo, ghost_hi;
  int32_t extent[SODA_HIP_MAX_DIM];    /* of the slab's arrays */
  void* inputs[SODA_HIP_MAX_TENSORS];  /* device arrays holding the state the
                                          next run starts from (num_inputs) */
  void* outputs[SODA_HIP_MAX_TENSORS]; /* ... the last run's results
                                          (num_outputs; for a program that
                                          iterates these ARE `inputs`) */
} soda_hip_slab_info_t;

typedef struct soda_hip_group_stats {   /* of the last soda_hip_group_run */
  int32_t exchange_every;
  int32_t intervals;                   /* runs of <= exchange_every iterations */
  int32_t exchanges;                   /* of them opened by a halo exchange */
  int32_t copies;                      /* peer copies enqueued, all slabs */
  int64_t copy_bytes;
  int32_t launches;                    /* kernel launches, all slabs */
  int32_t split_passes;                /* passes launched in two parts */
  float enqueue_ms;                    /* host time the run took to enqueue */
} soda_hip_group_stats_t;

typedef struct soda_hip_group soda_hip_group_t;        /* opaque */

/* Loads the code object on every device of the group and lays out the slabs.
 * Fails with SODA_HIP_ERR_INVALID if a slab would be thinner than its
 * neighbour's ghost rows. */
int soda_hip_group_create(const void* code, size_t code_size,
                          const soda_hip_plan_t* plan,
                          const soda_hip_group_desc_t* desc,
                          soda_hip_group_t** group);
int soda_hip_group_destroy(soda_hip_group_t* group);
int soda_hip_group_slab(soda_hip_group_t* group, int32_t slab,
                        soda_hip_slab_info_t* info);
/* The exchange interval a group of this description would use (no GPU). */
int soda_hip_group_plan(const soda_hip_plan_t* plan,
                        const soda_hip_group_desc_t* desc,
                        int32_t* exchange_every);
/* Scatters host arrays (inputs, then one entry per param array of which only
 * `ptr` is read -- as soda_hip_run_host) over the slabs, ghost rows included:
 * the state the next run starts from.  Synchronous. */
int soda_hip_group_load(soda_hip_group_t* group,
                        const soda_hip_host_tensor_t* inputs);
/* Tells the group that the caller filled the slabs' `inputs` arrays on the
 * devices itself (soda_hip_slab_info_t), ghost rows included. */
int soda_hip_group_loaded(soda_hip_group_t* group);
/* Advances the state `iterate` iterations.  A program that iterates continues
 * from the previous run's result (its ghost rows are refreshed first).
 * Asynchronous: returns when everything is enqueued. */
int soda_hip_group_run(soda_hip_group_t* group, int32_t iterate);
int soda_hip_group_synchronize(soda_hip_group_t* group);
/* Gathers every slab's own rows of the results into host arrays; only box
 * [valid_lo, valid_hi) of each output is written (NULL: everything), as
 * soda_hip_run_host_box.  Synchronises first. */
int soda_hip_group_store(soda_hip_group_t* group,
                         const soda_hip_host_tensor_t* outputs,
                         const int32_t* valid_lo, const int32_t* valid_hi);
/* Replaces soda::app::<app>() on N GPUs: load, run, store. */
int soda_hip_group_run_host(soda_hip_group_t* group,
                            const soda_hip_host_tensor_t* inputs,
                            const soda_hip_host_tensor_t* outputs,
                            int32_t iterate, const int32_t* valid_lo,
                            const int32_t* valid_hi);
int soda_hip_group_last_stats(soda_hip_group_t* group,
                              soda_hip_group_stats_t* stats);
/* soda_hip_group_run that also takes the residual of the last of `iterate`
 * iterations: every slab's LAST interval goes through
 * soda_hip_run_device_slab_residual into 32 bytes the group owns on that
 * slab's device (allocated at create when plan.residual.present, never inside
 * a run); earlier intervals are those of soda_hip_group_run.  The box is that
 * of all iterations since soda_hip_group_load / _loaded: both reset the
 * count, every run -- plain ones too -- adds to it.  Asynchronous like
 * soda_hip_group_run; threaded or not, overlapped or not.
 * SODA_HIP_ERR_UNSUPPORTED, nothing launched: the plan has no residual;
 * SODA_HIP_ERR_INVALID: no state loaded. */
int soda_hip_group_run_residual(soda_hip_group_t* group, int32_t iterate);
/* Synchronises the group, fetches the slabs' structs and folds them on the
 * host -- counts add, maxima take the larger: the residual of the whole grid,
 * exactly.  per_slab_host: num_slabs structs, or NULL.  SODA_HIP_ERR_INVALID
 * if the group's last run was not a residual run. */
int soda_hip_group_residual(soda_hip_group_t* group,
                            soda_hip_residual_t* result_host,
                            soda_hip_residual_t* per_slab_host);
/* soda_hip_last_residual of one slab's last interval. */
int soda_hip_group_last_residual(soda_hip_group_t* group, int32_t slab,
                                 int32_t* mode, int32_t* fused_iters);
/* Iterates the group's state until converged.  SYNCHRONOUS: `check_every`
 * iterations at a time through soda_hip_group_run_residual (the last chunk may
 * be shorter), after each soda_hip_group_residual, and stops when
 *   unordered == 0 && max_float <= tol && max_int <= int_tol
 * or when `max_iterate` iterations are done -- the rule of
 * soda_hip_run_device_until.  SODA_HIP_OK either way; *iterations_done and
 * *result_host (either may be NULL) tell which.  The state lives in the
 * slabs: nothing is copied, soda_hip_group_store delivers the result. */
int soda_hip_group_run_until(soda_hip_group_t* group, int32_t max_iterate,
                             int32_t check_every, double tol, uint64_t int_tol,
                             soda_hip_residual_t* result_host,
                             int32_t* iterations_done);

/* -- the reference kernel's WIRE format: <app>_kernel on banked streams -----
 * The reference's generated host hands its kernel one linear stream per
 * tensor -- tiles end to end, each padded to whole bursts, elements dealt
 * cyclically over the tensor's DRAM banks, kStencilDistance void elements
 * appended (src/soda/codegen/frt/host.py:124-249, docs/data-layout.md) -- and
 * calls
 *     <app>_kernel(bank_0_<out>..., bank_0_<in>..., coalesced_data_num)
 * (frt/host.py:44-59 declaration, :282-289 call; outputs first).  A stream
 * object runs exactly that contract on the GPU, so the unmodified generated
 * host can link against it under SODA_CPP_BINDING (`sodac --hip-wire-kernel`
 * prints the extern "C" <app>_kernel definition that calls it).  Per call:
 * un-interleave the inputs (skipped for single-bank inputs, read in place),
 * run the program on the de-interleaved stream -- as the original n-D program
 * with the marching kernels when the stream is a dense array of rows, else as
 * the linearised 1-D program -- and write the outputs back shifted by their
 * stencil offset (frt/host.py:400-424) and re-interleaved.  A program built
 * to store its outputs at their wire positions (`sodac --hip-wire-kernel`
 * does: store index moved by the window point of largest linear offset)
 * declares shift 0 for them; such an output on ONE bank is written by the
 * program straight into the caller's bank and has no copy kernel. */
typedef struct soda_hip_stream_desc {
  int32_t dim;                         /* of the original program */
  int32_t num_inputs;
  int32_t num_outputs;
  int32_t iterate;
  int32_t tile[SODA_HIP_MAX_DIM];      /* tile size of dimensions 0..dim-2 */
  int32_t stencil_distance;            /* kStencilDistance (frt/host.py:683-696) =
                                        * max(window distance, stencil offset),
                                        * reference core.py:620-625 */
  /* per tensor, inputs first, then outputs */
  int32_t banks[SODA_HIP_MAX_TENSORS];
  int32_t elem_size[SODA_HIP_MAX_TENSORS];
  int32_t elems_per_cycle[SODA_HIP_MAX_TENSORS];  /* burst width / element
                                          width x banks (frt/host.py:120-122) */
  int32_t shift[SODA_HIP_MAX_TENSORS]; /* inputs: produce offset the host delays
                                          the tensor by (frt/host.py:241-246);
                                          outputs: what is LEFT of the stencil
                                          offset the kernel emits a cell late
                                          by (:401-408) for the copy kernel to
                                          apply; 0 = the program did it */
  int32_t num_linear;                  /* 1-D programs offered, widest first */
  int32_t linear_vec[4];               /* their cells per thread; the last is 1 */
} soda_hip_stream_desc_t;

typedef struct soda_hip_stream soda_hip_stream_t;      /* opaque */

/* `dense`: the original program (NULL: always the linear form); `linear`:
 * num_linear programs of the linearised 1-D form; `unwire[i]` / `wire[o]`: the
 * copy kernels of input i / output o as one-kernel programs (unwire[i] /
 * wire[o] may be NULL for a tensor on one bank with shift 0).  The stream
 * borrows the programs; the caller destroys them after the stream. */
int soda_hip_stream_create(const soda_hip_stream_desc_t* desc,
                           soda_hip_program_t* dense,
                           soda_hip_program_t* const* linear,
                           soda_hip_program_t* const* unwire,
                           soda_hip_program_t* const* wire,
                           soda_hip_stream_t** stream);
int soda_hip_stream_destroy(soda_hip_stream_t* stream);
/* Bank pointers in the order of the reference kernel's ports: all banks of
 * output 0, output 1, ...; then all banks of input 0, input 1, ....  Device
 * pointers, asynchronous on `hip_stream`.  A tensor on ONE bank is read /
 * written in place by the program and must be 16-byte aligned (INVALID
 * otherwise; hipMalloc and the reference host's aligned_alloc(4096) are);
 * banks of a tensor on several may start anywhere (the copy kernels move 16
 * bytes per bank per thread when all are aligned, single elements if not). */
int soda_hip_stream_run_device(soda_hip_stream_t* stream,
                               void* const* out_banks,
                               const void* const* in_banks,
                               uint64_t coalesced_data_num, void* hip_stream);
/* The same on host buffers sized as the reference host allocates them
 * (coalesced_data_num x elems_per_cycle / banks elements per bank): what
 * <app>_kernel receives under SODA_CPP_BINDING.  Synchronous.  Where the
 * program stores its outputs late itself and the stream is a dense array of
 * rows, the banks go through the host-array entry on the n-D program (bands:
 * copy-in, kernels and copy-out overlapped; a banked tensor is
 * (de)interleaved, a delayed single-bank input un-delayed, by the host
 * threads on its way through the staging slots, no copy kernel runs;
 * SODA_HIP_STREAM_NO_BANDS=1: whole banks in, copy kernels, run, copy kernels,
 * whole banks out, as for every other stream). */
int soda_hip_stream_run_host(soda_hip_stream_t* stream, void* const* out_banks,
                             const void* const* in_banks,
                             uint64_t coalesced_data_num);
/* 1: the last run used the dense n-D form, 2: the linear form, 3: the banked
 * form of the dense program (soda_hip_stream_set_banked), 0: none yet */
int soda_hip_stream_last_mode(soda_hip_stream_t* stream);
/* Opt-in: `program` is the BANKED form of the stream's dense program -- ONE
 * marching kernel that runs all `iterate` iterations and, for every tensor t
 * (inputs first, then outputs) with in_kernel[t] != 0, addresses the tensor's
 * banks itself, each through a buffer resource of its own, (de)interleaving
 * in registers.  Its plan is a one-pass, one-iteration plan that lists every
 * bank of such a tensor as a tensor of its own (banks[t] consecutive slots);
 * every other tensor is one dense array to it.  A tensor may be in_kernel if
 * it is on 2 or 4 banks, that count divides tile[0] and its shift (inputs:
 * the kernel starts shift / banks elements into each bank; outputs: shift 0,
 * born at their wire positions).  soda_hip_stream_run_device then takes this
 * program whenever the stream has a dense view, the device-dense tile rule
 * admits it and every bank of every in_kernel tensor is 16-byte aligned: no
 * unwire_ / wire_ kernel and no staging array for those tensors.  Stream
 * elements beyond the dense view (the partial last row, the void tail) stay
 * as the caller left them.  Otherwise the call runs as without it.
 * soda_hip_stream_run_host is unaffected.  The stream borrows the program;
 * NULL unsets it. */
int soda_hip_stream_set_banked(soda_hip_stream_t* stream,
                               soda_hip_program_t* program,
                               const int32_t* in_kernel);
/* Two-iteration programs, after soda_hip_stream_set_banked: `first` is the
 * ONE-iteration kernel with the in_kernel inputs bank by bank (outputs dense),
 * `last` the one with the in_kernel outputs bank by bank (inputs dense), plans
 * as above.  A run on banks takes the launches the dense program's MODEL
 * schedule names for the stream's extent (soda_hip_stream_set_banked turns the
 * clock's calibration of the stream's dense program off, so both paths of the
 * stream are scheduled from one source): one fused launch -> `program`; two
 * one-iteration launches -> `first`, a dense temporary per output, `last`; any
 * other schedule, or that one without a pair, keeps the copy pass.  Border
 * cells no host reads depend on that split; a stream WITHOUT a banked program
 * whose dense program times its passes may split otherwise and then differs
 * on those cells only.
 * NULL, NULL unsets the pair. */
int soda_hip_stream_set_banked_pair(soda_hip_stream_t* stream,
                                    soda_hip_program_t* first,
                                    soda_hip_program_t* last);
/* soda_hip_stream_run_device takes the dense view only for tiles at least this
 * wide in dimension 0 (default 256: narrower ones leave most of a marching
 * strip idle and the linear form is faster on the GPU; 0: whenever there is a
 * dense view).  soda_hip_stream_run_host always prefers the dense view: there
 * the copies dominate, and the dense view lets them overlap in bands. */
int soda_hip_stream_set_device_dense_min_tile(soda_hip_stream_t* stream,
                                              int32_t min_tile0);

/* -- device memory and timing helpers for hosts without their own -------- */
int soda_hip_malloc(int32_t device, size_t bytes, void** ptr);
int soda_hip_free(int32_t device, void* ptr);
int soda_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int soda_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int soda_hip_memcpy_d2d(void* dst, int32_t dst_device, const void* src,
                        int32_t src_device, size_t bytes, void* stream);
int soda_hip_memset(void* dst, int value, size_t bytes, void* stream);
int soda_hip_stream_synchronize(void* stream);
int soda_hip_event_create(soda_hip_event_t** event);
int soda_hip_event_record(soda_hip_event_t* event, void* stream);
int soda_hip_event_elapsed_ms(soda_hip_event_t* start, soda_hip_event_t* stop,
                              float* ms);   /* synchronises on `stop` */
int soda_hip_event_destroy(soda_hip_event_t* event);
/* For callers that run their own halo exchange beside
 * soda_hip_run_device_slab: the hipEvent_t inside an event (what
 * soda_hip_slab_run_t takes), a HIP stream of their own, and ordering a
 * stream behind an event. */
int soda_hip_event_handle(soda_hip_event_t* event, void** hip_event);
int soda_hip_hipstream_create(int32_t device, void** stream);
int soda_hip_hipstream_destroy(void* stream);
int soda_hip_hipstream_wait_event(void* stream, soda_hip_event_t* event);

#ifdef __cplusplus
}
#endif
#endif  /* SODA_HIP_H_ */
