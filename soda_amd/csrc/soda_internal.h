// soda_internal.h -- what the translation units of libsoda_hip.so share
// (soda_hip.cpp: programs, launch geometry, runs; soda_group.cpp: slab groups;
// soda_stream.cpp: the wire-format stream object, with soda_stream.h; ...).
// Nothing here crosses the C ABI (include/soda_hip.h).
#ifndef SODA_INTERNAL_H_
#define SODA_INTERNAL_H_

#include "soda_hip.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace soda_detail {

int fail(int status, const std::string& what);
const std::string& last_error_text();   // of the calling thread
int hip_fail(hipError_t e, const char* what);

#define HIP_TRY(expr)                                              \
  do {                                                             \
    hipError_t e_ = (expr);                                        \
    if (e_ != hipSuccess) return soda_detail::hip_fail(e_, #expr); \
  } while (0)

struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  int32_t regrown = 0;   // times ensure() replaced it by a larger one
};
// At least `bytes` behind b.ptr.  Replacing a buffer synchronises the device
// first: work in flight may still use the old one.
int ensure(DeviceBuffer& b, size_t bytes);
bool too_small(const DeviceBuffer& b, size_t bytes);   // would ensure() allocate?
// SODA_HIP_ERR_INVALID ("... nothing was launched") if `stream` is being
// captured into a graph: asked only by a call that found a buffer too_small,
// before its first launch
int refuse_growth_while_capturing(void* stream, const char* who);

typedef std::array<int32_t, SODA_HIP_MAX_DIM> ExtentKey;

struct Geometry {
  int32_t tile[SODA_HIP_MAX_DIM];
  double ns;          // modelled time of one launch; 0: no model
};

// What a run on one extent uses.  Sizing the chunks of every kernel costs tens
// of microseconds of host time (more on tall grids) and the schedule a
// knapsack over the iteration count: both are remembered per extent, a launch
// must not pay for them again.
struct ExtentPlan {
  std::vector<Geometry> geo;      // per kernel
  std::vector<double> model_ns;   // per pass, from the descriptors' model
  // iterate -> launches of every pass, then their sum (num_passes + 1 values)
  std::map<int32_t, std::vector<int32_t>> sched;
};

// rows (cells along the last dimension) a run must deliver, and how far one
// iteration reaches beyond a row on either side: passes may then skip the rows
// whose results no later iteration of the run can carry into [keep_lo, keep_hi)
struct Cone {
  int32_t keep_lo, keep_hi, reach_lo, reach_hi;
};

// A run between two halo exchanges (include/soda_hip.h, soda_hip_slab_run_t)
struct SlabRun {
  Cone cone;
  int32_t ghost_lo, ghost_hi;   // input rows an exchange in flight refreshes
  int32_t send_lo, send_hi;     // result rows the neighbours fetch next
  hipEvent_t ghosts_ready;      // may be null
  hipEvent_t sendable;          // may be null
};

// Pinned staging slots of the host-array entry (soda_host.cpp): chunk i + 1
// is packed by worker threads while the DMA engine moves chunk i.
struct HostRing {
  static const int kMaxSlots = 4;
  char* base = nullptr;
  size_t slot_bytes = 0;
  int slots = 0;
  hipEvent_t ev[kMaxSlots] = {nullptr, nullptr, nullptr, nullptr};
  // a DMA out of / into the slot may still be in flight (its event recorded):
  // whoever fills the slot next waits for the event first
  bool busy[kMaxSlots] = {false, false, false, false};
  int ensure(size_t slot_bytes, int slots);
  int wait(int slot);      // until the slot's last DMA is done
  void release();
};

}  // namespace soda_detail

struct soda_hip_program {
  soda_hip_plan_t plan;
  int device = 0;
  hipModule_t module = nullptr;
  std::vector<hipFunction_t> functions;
  std::vector<soda_detail::DeviceBuffer> locals;   // one per local tensor
  std::vector<soda_detail::DeviceBuffer> temps;    // one per output: ping-pong
  // ... and its partner in runs trimmed to a cone, which keep their
  // intermediate passes out of the caller's outputs (run_core)
  std::vector<soda_detail::DeviceBuffer> temps2;
  // soda_hip_run_device_until[_norm]: the arrays its chunks ping-pong through
  // beside the caller's outputs (one per output), and the struct it fetches
  // (32 bytes of residual or a soda_hip_norms_t, whichever was asked for)
  std::vector<soda_detail::DeviceBuffer> until_tmp;
  soda_detail::DeviceBuffer until_struct;
  // how the last soda_hip_run_device_residual took its residual (0 none,
  // 1 twin, 2 `<app>_residual`) and the fusion depth of its last pass
  int32_t last_res_mode = 0;
  int32_t last_res_fused = 0;
  std::vector<soda_detail::DeviceBuffer> host_in;  // run_host staging
  std::vector<soda_detail::DeviceBuffer> host_prm; // ... of the param arrays
  std::vector<soda_detail::DeviceBuffer> host_out;
  // ... its streams (copies in / kernels / copies out), pinned slots, the
  // band output arrays and events of the banded way (soda_host.cpp)
  hipStream_t hstream[3] = {nullptr, nullptr, nullptr};
  soda_detail::HostRing ring_in, ring_out;
  std::vector<soda_detail::DeviceBuffer> band_out;
  std::vector<hipEvent_t> hevents;
  bool hbuf_used[2] = {false, false};
  int32_t last_launches = 0;
  int32_t last_fused = 0;
  int32_t last_split = 0;    // passes of the last run launched in two parts
  int64_t last_rows = 0;     // cells along the last dimension, summed over passes
  void* debug = nullptr;     // time-stamp buffer of diagnostic builds
  // kargs.reserved[0] of every launch: the length of the wire stream a banked
  // program runs on (soda_hip_stream_set_banked), 0 for every other program
  int32_t stream_elems = 0;
  // a wire stream's copy kernel or banked program (soda_hip_stream_create,
  // soda_hip_stream_set_banked[_pair]): its tensors are banks -- a fraction of
  // `extent` cells long, at any address, the kernels pick their access width
  // from it -- so run_core's overlap and alignment rules, which take every
  // tensor as one dense array of `extent`, do not apply; the stream layer
  // checks what it hands over itself
  bool bank_tensors = false;
  // time every pass on an extent the first time it is run (a few ms, once):
  // on unless SODA_HIP_NO_CALIBRATE is set or the caller turns it off
  bool auto_calibrate = true;
  bool calibrating = false;
  // measured time of one launch of every pass, per extent (calibrate)
  std::map<soda_detail::ExtentKey, std::vector<double>> measured;
  std::map<soda_detail::ExtentKey, soda_detail::ExtentPlan> extents;
  // the same two for launches over a batch of grids
  // (soda_hip_run_device_batch), per batch size > 1: a plan, a schedule and a
  // measured time hold for one (extent, batch) only.  measured_of /
  // extents_of pick the map of a batch size
  std::map<int32_t, std::map<soda_detail::ExtentKey, std::vector<double>>>
      measured_bt;
  std::map<int32_t,
           std::map<soda_detail::ExtentKey, soda_detail::ExtentPlan>>
      extents_bt;
  // split passes: the chunks next to a slab's ghost rows run on a stream of
  // their own, beside the interior on the caller's stream
  hipStream_t side = nullptr;
  hipEvent_t ev_pre[2] = {nullptr, nullptr};
  hipEvent_t ev_bnd[2] = {nullptr, nullptr};
  int ev_turn = 0;
};

// The kernels of one norms module (codegen/hip/norms.py) on one device: the
// zeroing kernel and one accumulating kernel per fragment width, widest first
struct soda_hip_norms_handle {
  int device = 0;
  int32_t cell = 0, kind = 0, elem = 0, dim = 0;
  hipModule_t module = nullptr;
  hipFunction_t zero = nullptr;
  std::vector<std::pair<int32_t, hipFunction_t>> widths;
};

namespace soda_detail {

// A run that also takes the residual of its last iteration
// (soda_hip_run_device_residual): where the struct goes, and the iterations
// the counted box is that of (soda_hip_run_device_until runs chunk after
// chunk: the box is the one after all iterations done so far; a slab run
// between two exchanges: the iterations since the state was the caller's).
// On a slab (RunRequest's `slab`, `origin`, `global_extent`) the box is the
// global grid's, cut to the slab's kept rows (soda_hip_plan_residual_slab_box)
// `norms` != nullptr (soda_hip_run_device_norms): `dev` is a soda_hip_norms_t,
// the run always ends in the one-iteration pass, and the handle's kernels run
// in place of `<app>_residual_zero` and `<app>_residual`.
// `box` != nullptr (bordered and periodic domains, soda_periodic.cpp): the
// cells counted, in the coordinates of the arrays the run addresses, in place
// of the box after `box_iterate` iterations, which is then not looked at; not
// on a slab.  `accumulate`: do not zero the struct, add to it -- several runs
// and boxes fill one struct that residual_zero zeroed once.
struct ResidualRun {
  void* dev;
  int32_t box_iterate;
  soda_hip_norms_handle* norms = nullptr;
  const soda_hip_resbox_t* box = nullptr;
  bool accumulate = false;
};

// One run of a program on device arrays: `RunRequest rq = {outputs, inputs,
// extent, iterate, stream};`, then whatever else the caller sets, by name.
// origin / global_extent: the window's place in a larger grid (null: the
// window is the grid).  force_pass >= 0: use only that pass (calibration).
// batch > 1: every tensor holds that many grids of `extent`, one launch runs
// them all (a batched plan, no slab: soda_hip_run_device_batch checks)
struct RunRequest {
  void* const* outputs;
  const void* const* inputs;
  const int32_t* extent;
  int32_t iterate;
  void* stream;
  const int32_t* origin = nullptr;
  const int32_t* global_extent = nullptr;
  int force_pass = -1;
  const SlabRun* slab = nullptr;
  int32_t batch = 1;
  const ResidualRun* residual = nullptr;
};
int run_core(soda_hip_program* p, const RunRequest& rq);
// Would a plain run of `iterate` iterations on `ext` grow the scratch of `p`
// (sets *grows, never clears it)?  By the schedule run_core itself would take
// on a capturing stream (measured times where there are any, never a
// calibration).
int program_grows(soda_hip_program* p, const int32_t* ext, int32_t iterate,
                  bool* grows);

// The pieces of a residual that several runs and boxes fill (ResidualRun's
// `accumulate`), each one launch on `stream`.  residual_zero: the struct
// zeroed by `<app>_residual_zero` / the norms handle's kernel.  residual_add:
// the cells `box` of the dense arrays `cur` (one per output) against `prev`
// (one per input), all of `extent`, added by `<app>_residual` / the norms
// kernel per pair; a box that is empty for every pair launches nothing.
int residual_zero(soda_hip_program* p, const ResidualRun& res, void* stream);
int residual_add(soda_hip_program* p, void* const* cur,
                 const void* const* prev, const int32_t* extent,
                 const ResidualRun& res, const soda_hip_resbox_t& box,
                 void* stream);
// What soda_hip_run_device_residual / _norms ask of a program (and a norms
// handle) and of the struct (`dev` null: of the program and handle only),
// for entries that run on other arrays than a program's plain ones.
int check_residual_request(const soda_hip_program* p, void* const* outputs,
                           const int32_t* extent, const void* dev,
                           const char* who);
int check_norms_request(const soda_hip_program* p,
                        const soda_hip_norms_handle* h, void* const* outputs,
                        const int32_t* extent, const void* dev,
                        const char* who);
// the stop rule of a run until a norm is small; false: a struct of no kind
bool norms_converged(const soda_hip_norms_t& acc, int32_t which, double tol,
                     bool* stop);

// What run_core asks of the caller's addresses before anything is launched,
// each tensor taken as the dense array of `cells` x `batch` cells the kernels
// address: no output shares a byte with an input, a param array or another
// output, and every tensor is aligned to min(16, vec x its cell size) for the
// widest `vec` of the plan's kernels (a param array to one cell).  Looks at
// the addresses only, never behind them.  bank_tensors: nothing is asked
// (soda_hip_program::bank_tensors).
int check_run_tensors(const soda_hip_plan_t& plan, bool bank_tensors,
                      void* const* outputs, const void* const* inputs,
                      int64_t cells, int32_t batch);

// Has a run that stops on its residual converged?
inline bool residual_converged(const soda_hip_residual_t& r, double tol,
                               uint64_t int_tol) {
  double max_float;
  memcpy(&max_float, &r.max_float_bits, sizeof max_float);
  return r.unordered == 0 && max_float <= tol && r.max_int <= int_tol;
}

inline std::map<ExtentKey, std::vector<double>>& measured_of(
    soda_hip_program* p, int32_t batch) {
  if (batch <= 1) return p->measured;
  if (p->measured_bt.size() > 64 && !p->measured_bt.count(batch))
    p->measured_bt.clear();
  return p->measured_bt[batch];
}
inline std::map<ExtentKey, ExtentPlan>& extents_of(soda_hip_program* p,
                                                   int32_t batch) {
  if (batch <= 1) return p->extents;
  if (p->extents_bt.size() > 64 && !p->extents_bt.count(batch))
    p->extents_bt.clear();
  return p->extents_bt[batch];
}

// one launch (or, split, one pair of launches) of a run
struct PassLaunch {
  int pass;                  // index into plan.passes
  int32_t lo, hi;            // rows of the last dimension it covers
  bool wait, record, split;  // behind ghosts_ready / ahead of sendable / in two
  int32_t chunk, chunks;     // split: rows per block tile, tiles along the axis
  int32_t bnd_lo, bnd_hi;    // boundary tiles: [0, bnd_lo) U [bnd_hi, chunks)
};
int plan_launches(const soda_hip_plan_t& plan,
                  std::map<ExtentKey, ExtentPlan>* cache, const int32_t* ext,
                  const int32_t* count, int32_t total, int32_t iterate,
                  const SlabRun* slab, std::vector<PassLaunch>* out,
                  int res_pass = -1, bool res_twin = false);

// A residual run keeps the multiset of passes `count` / `total` scheduled for
// `iterate` iterations and names the pass that goes last (*res_pass) and
// whether it runs as its twin: the deepest scheduled pass whose kernel has
// one; else the one-iteration pass, behind which `<app>_residual` runs --
// taken out of a deeper pass's count where the schedule had none (iterate - 1
// iterations rescheduled by `pass_ns`, one added).  `generic_only`: never a
// twin (a run that takes the norms; SODA_HIP_RESIDUAL_GENERIC=1 says the same).
int residual_order(const soda_hip_plan_t& plan,
                   const std::vector<double>& pass_ns, int32_t iterate,
                   int32_t* count, int32_t* total, int* res_pass,
                   bool* res_twin, bool generic_only = false);

// tiles, modelled pass times and schedules of `plan` on `ext` (all
// SODA_HIP_MAX_DIM entries filled) for launches over `batch` grids,
// remembered in `cache` (which holds one batch size's: extents_of)
int extent_plan(const soda_hip_plan_t& plan,
                std::map<ExtentKey, ExtentPlan>* cache, const int32_t* ext,
                ExtentPlan** out, int32_t batch = 1);

// launches of every pass for `iterate` iterations by the given pass times
int schedule(const soda_hip_plan_t& plan, const std::vector<double>& pass_ns,
             int32_t iterate, int32_t* count, int32_t* total);

void copy_box(char* strided, const int32_t* stride, char* dense,
              const int32_t* extent, const int32_t* lo, const int32_t* hi,
              int dim, int elem, bool to_dense);
bool is_dense(const soda_hip_host_tensor_t& t, int dim);
// the same for a dense array that starts at index `row0` of the last
// dimension, on up to `threads` threads (0: the pool's; soda_host.cpp)
// soda_hip_run_host_box, with tensors as the wire format's host streams hold
// them: nbanks (NULL: none) holds, per tensor, inputs then outputs, the number
// of DRAM banks -- where it is > 1 the tensor's `ptr` is the list of its bank
// pointers; lead (NULL: none), per input, the elements the generated host
// delayed a single-bank stream of stream_elems elements by.
int run_host_call(soda_hip_program* p, const soda_hip_host_tensor_t* inputs,
                  const soda_hip_host_tensor_t* outputs, int32_t iterate,
                  const int32_t* valid_lo, const int32_t* valid_hi,
                  const int32_t* nbanks, const int32_t* lead,
                  int64_t stream_elems);
void weave_banks(char* const* banks, int nb, char* dense, int64_t first,
                 int64_t count, int elem, bool to_dense, int threads);
bool host_pinned(const void* ptr, size_t bytes);
void copy_rows(char* strided, const int32_t* stride, char* dense,
               const int32_t* extent, const int32_t* lo, const int32_t* hi,
               int dim, int elem, bool to_dense, int32_t row0, int threads);

// contiguous host <-> device copies through a program's pinned rings and the
// worker pool (soda_host.cpp); ring_fetch returns when the bytes are delivered
int ring_send(soda_hip_program* p, void* dev, const void* host, size_t bytes,
              hipStream_t stream);
int ring_fetch(soda_hip_program* p, void* host, const void* dev, size_t bytes,
               hipStream_t stream);
// rows [a, b) of a host tensor -> device / the part of box [lo, hi) in rows
// [a, b) of a device array -> a host tensor, through the rings (soda_host.cpp);
// `dev` holds the dense array from row `dev_row0` of the last dimension on
int send_rows(soda_hip_program* p, const soda_hip_host_tensor_t& t,
              const int32_t* extent, int dim, int elem, int64_t a, int64_t b,
              void* dev, int64_t dev_row0, hipStream_t stream);
int fetch_rows(soda_hip_program* p, const soda_hip_host_tensor_t& t,
               const int32_t* extent, const int32_t* lo, const int32_t* hi,
               int dim, int elem, int64_t a, int64_t b, const void* dev,
               int64_t dev_row0, hipStream_t stream);
// the program's stream of host-array runs, made on first use
int host_stream(soda_hip_program* p, hipStream_t* stream);

}  // namespace soda_detail

#endif  // SODA_INTERNAL_H_
