// libsoda_hip.so -- C-ABI shim between the Python host and the JIT-built HIP
// stencil kernels (interface and reference citations: include/soda_hip.h).
//
// Owns what the reference's generated C++ host owns at run time (reference
// src/soda/codegen/frt/host.py:62-431): device buffers, the launch sequence
// over all iterations, copy-in / copy-out of the valid box.  What it does NOT
// do, on purpose: no FPGA tiling/burst layout (frt/host.py:181-249) -- the
// kernels read the caller's dense dim-0-fastest arrays directly; no CPU
// fallback of any kind -- without a GPU every run entry fails with
// SODA_HIP_ERR_NODEVICE.
//
// Build: hipcc -O2 -fPIC -shared soda_hip.cpp soda_group.cpp -o libsoda_hip.so
//        -lhiprtc   (__graft_entry__.build_library)
#include "soda_internal.h"

#include <hip/hiprtc.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

namespace soda_detail {

thread_local std::string g_error;

int fail(int status, const std::string& what) {
  g_error = what;
  return status;
}

const std::string& last_error_text() { return g_error; }

int hip_fail(hipError_t e, const char* what) {
  char buf[512];
  snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
  g_error = buf;
  if (e == hipErrorOutOfMemory) return SODA_HIP_ERR_NOMEM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
    return SODA_HIP_ERR_NODEVICE;
  return SODA_HIP_ERR_RUNTIME;
}

int ensure(DeviceBuffer& b, size_t bytes) {
  if (b.bytes >= bytes && b.ptr) return SODA_HIP_OK;
  if (b.ptr) {
    // Earlier asynchronous calls on the handle may still be reading or writing
    // the old buffer on any stream: wait for the device before it goes.  That
    // hipFree waits too is nothing the HIP documentation promises; regrowth is
    // rare and pays for a hipMalloc anyway.
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(b.ptr));
    b.ptr = nullptr;
    b.bytes = 0;
    ++b.regrown;
  }
  HIP_TRY(hipMalloc(&b.ptr, bytes));
  b.bytes = bytes;
  return SODA_HIP_OK;
}

bool too_small(const DeviceBuffer& b, size_t bytes) {
  return !b.ptr || b.bytes < bytes;
}

int refuse_growth_while_capturing(void* stream, const char* who) {
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(static_cast<hipStream_t>(stream), &capture) !=
      hipSuccess) {
    (void)hipGetLastError();
    return SODA_HIP_OK;
  }
  if (capture == hipStreamCaptureStatusNone) return SODA_HIP_OK;
  return fail(SODA_HIP_ERR_INVALID,
              std::string(who) +
                  ": scratch buffers must grow for this call and the stream is "
                  "being captured into a graph, where allocating is illegal; "
                  "run the same call once eagerly before the capture; nothing "
                  "was launched");
}

}  // namespace soda_detail

using namespace soda_detail;

struct soda_hip_event {
  hipEvent_t ev;
};

extern "C" {

int soda_hip_abi_version(void) { return SODA_HIP_ABI_VERSION; }

const char* soda_hip_status_string(int status) {
  switch (status) {
    case SODA_HIP_OK: return "ok";
    case SODA_HIP_ERR_INVALID: return "invalid argument";
    case SODA_HIP_ERR_COMPILE: return "kernel compilation failed";
    case SODA_HIP_ERR_RUNTIME: return "HIP runtime error";
    case SODA_HIP_ERR_NOMEM: return "out of memory";
    case SODA_HIP_ERR_NODEVICE: return "no usable GPU";
    case SODA_HIP_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
  }
}

size_t soda_hip_last_error(char* buf, size_t cap) {
  if (buf && cap) {
    size_t n = g_error.size() < cap - 1 ? g_error.size() : cap - 1;
    memcpy(buf, g_error.data(), n);
    buf[n] = 0;
  }
  return g_error.size();
}

int soda_hip_device_count(int* count) {
  if (!count) return fail(SODA_HIP_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  *count = n;
  return SODA_HIP_OK;
}

size_t soda_hip_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(soda_hip_kargs_t);
    case 1: return sizeof(soda_hip_kernel_desc_t);
    case 2: return sizeof(soda_hip_pass_desc_t);
    case 3: return sizeof(soda_hip_plan_t);
    case 4: return sizeof(soda_hip_host_tensor_t);
    case 5: return sizeof(soda_hip_stream_desc_t);
    case 6: return sizeof(soda_hip_slab_run_t);
    case 7: return sizeof(soda_hip_group_desc_t);
    case 8: return sizeof(soda_hip_slab_info_t);
    case 9: return sizeof(soda_hip_group_stats_t);
    case 10: return sizeof(soda_hip_launch_info_t);
    case 11: return sizeof(soda_hip_residual_t);
    case 14: return sizeof(soda_hip_norms_t);
    case 12: return sizeof(soda_hip_resbox_t);
    case 15: return sizeof(soda_hip_periodic_desc_t);
    case 16: return sizeof(soda_hip_periodic_info_t);
    case 17: return sizeof(soda_hip_border_desc_t);
    case 18: return sizeof(soda_hip_border_fused_desc_t);
    case 19: return sizeof(soda_hip_border_strip_t);
    case 20: return sizeof(soda_hip_border_fused_info_t);
    case 21: return sizeof(soda_hip_border_fused_boxes_t);
    case 22: return sizeof(soda_hip_border_faces_t);
    default: return 0;
  }
}

int soda_hip_compile(const char* source, const char* name,
                     const char* const* options, int32_t num_options,
                     void** code, size_t* code_size) {
  if (!source || !code || !code_size || num_options < 0)
    return fail(SODA_HIP_ERR_INVALID, "soda_hip_compile: NULL argument");
  *code = nullptr;
  *code_size = 0;
  hiprtcProgram prog;
  hiprtcResult r = hiprtcCreateProgram(&prog, source, name ? name : "soda.hip",
                                       0, nullptr, nullptr);
  if (r != HIPRTC_SUCCESS)
    return fail(SODA_HIP_ERR_COMPILE,
                std::string("hiprtcCreateProgram: ") + hiprtcGetErrorString(r));
  r = hiprtcCompileProgram(prog, num_options, const_cast<const char**>(options));
  size_t log_size = 0;
  hiprtcGetProgramLogSize(prog, &log_size);
  std::string log(log_size, '\0');
  if (log_size) hiprtcGetProgramLog(prog, &log[0]);
  if (r != HIPRTC_SUCCESS) {
    hiprtcDestroyProgram(&prog);
    return fail(SODA_HIP_ERR_COMPILE,
                std::string("hiprtcCompileProgram: ") + hiprtcGetErrorString(r) +
                    "\n" + log);
  }
  size_t size = 0;
  r = hiprtcGetCodeSize(prog, &size);
  if (r != HIPRTC_SUCCESS || size == 0) {
    hiprtcDestroyProgram(&prog);
    return fail(SODA_HIP_ERR_COMPILE, "hiprtcGetCodeSize failed");
  }
  void* out = malloc(size);
  if (!out) {
    hiprtcDestroyProgram(&prog);
    return fail(SODA_HIP_ERR_NOMEM, "malloc(code)");
  }
  r = hiprtcGetCode(prog, static_cast<char*>(out));
  hiprtcDestroyProgram(&prog);
  if (r != HIPRTC_SUCCESS) {
    free(out);
    return fail(SODA_HIP_ERR_COMPILE, "hiprtcGetCode failed");
  }
  *code = out;
  *code_size = size;
  g_error = log;  // warnings, if any
  return SODA_HIP_OK;
}

void soda_hip_free_code(void* code) { free(code); }

int soda_hip_compiler_version(int32_t* major, int32_t* minor) {
  if (!major || !minor) return fail(SODA_HIP_ERR_INVALID, "compiler_version: NULL");
  int a = 0, b = 0;
  if (hiprtcVersion(&a, &b) != HIPRTC_SUCCESS)
    return fail(SODA_HIP_ERR_COMPILE, "hiprtcVersion failed");
  *major = a;
  *minor = b;
  return SODA_HIP_OK;
}

static int check_plan(const soda_hip_plan_t* p);
static int plan_geometry_c(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t* tiles, float* pass_ns, int32_t batch = 1);
static int plan_schedule_c(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, int32_t* count, int32_t batch = 1);

int soda_hip_plan_geometry(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t* tiles, float* pass_ns) {
  return plan_geometry_c(plan, extent, tiles, pass_ns);
}

int soda_hip_plan_schedule(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, int32_t* count) {
  return plan_schedule_c(plan, extent, iterate, count);
}

static int check_batch(int32_t batch, const char* who) {
  if (batch >= 1 && batch <= SODA_HIP_MAX_BATCH) return SODA_HIP_OK;
  char buf[160];
  snprintf(buf, sizeof buf, "%s: batch = %d, must be 1 to %d (the grid's y "
           "dimension)", who, batch, SODA_HIP_MAX_BATCH);
  return fail(SODA_HIP_ERR_INVALID, buf);
}

int soda_hip_plan_geometry_batch(const soda_hip_plan_t* plan,
                                 const int32_t* extent, int32_t batch,
                                 int32_t* tiles, float* pass_ns) {
  if (int rc = check_batch(batch, "plan_geometry_batch")) return rc;
  return plan_geometry_c(plan, extent, tiles, pass_ns, batch);
}

int soda_hip_plan_schedule_batch(const soda_hip_plan_t* plan,
                                 const int32_t* extent, int32_t batch,
                                 int32_t iterate, int32_t* count) {
  if (int rc = check_batch(batch, "plan_schedule_batch")) return rc;
  return plan_schedule_c(plan, extent, iterate, count, batch);
}

static int check_plan(const soda_hip_plan_t* p) {
  if (p->abi_version != SODA_HIP_ABI_VERSION)
    return fail(SODA_HIP_ERR_INVALID, "plan: ABI version mismatch");
  if (p->dim < 1 || p->dim > SODA_HIP_MAX_DIM)
    return fail(SODA_HIP_ERR_INVALID, "plan: bad dim");
  if (p->num_inputs < 1 || p->num_outputs < 1 || p->num_locals < 0 ||
      p->num_params < 0 || p->num_params > SODA_HIP_MAX_PARAMS ||
      p->num_inputs + p->num_outputs + p->num_locals + p->num_params >
          SODA_HIP_MAX_TENSORS)
    return fail(SODA_HIP_ERR_INVALID, "plan: bad tensor counts");
  for (int k = 0; k < p->num_params; ++k)
    if (p->param_elems[k] < 1)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad param size");
  if (p->num_kernels < 1 || p->num_kernels > SODA_HIP_MAX_KERNELS)
    return fail(SODA_HIP_ERR_INVALID, "plan: bad kernel count");
  if (p->num_passes < 1 || p->num_passes > SODA_HIP_MAX_PASSES)
    return fail(SODA_HIP_ERR_INVALID, "plan: bad pass count");
  int slots = p->num_inputs + p->num_outputs + p->num_locals + p->num_params;
  for (int s = 0; s < slots; ++s)
    if (p->elem_size[s] < 1 || p->elem_size[s] > 16)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad element size");
  for (int k = 0; k < p->num_kernels; ++k) {
    const soda_hip_kernel_desc_t& d = p->kernels[k];
    if (!memchr(d.name, 0, SODA_HIP_NAME_LEN) || !d.name[0])
      return fail(SODA_HIP_ERR_INVALID, "plan: bad kernel name");
    int64_t threads = 1;
    for (int i = 0; i < 3; ++i) {
      if (d.block[i] < 1) return fail(SODA_HIP_ERR_INVALID, "plan: bad block");
      threads *= d.block[i];
    }
    if (threads > 1024) return fail(SODA_HIP_ERR_INVALID, "plan: block > 1024");
    for (int i = 0; i < p->dim; ++i)
      if (d.tile[i] < 1) return fail(SODA_HIP_ERR_INVALID, "plan: bad tile");
    if (d.lds_bytes < 0 || d.lds_bytes > 160 * 1024)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad lds_bytes");
    if (d.vec < 0 || d.march_dim < 0 || d.march_dim > p->dim ||
        d.waves_along < 0 || d.warm < 0 || d.vgprs < 0 || d.pipe < 0 ||
        d.step_ns < 0 || d.bytes_per_cell < 0 || d.warm_saved < 0)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad launch-geometry field");
  }
  int prev = 1 << 30;
  for (int i = 0; i < p->num_passes; ++i) {
    const soda_hip_pass_desc_t& q = p->passes[i];
    if (q.fused_iters < 1 || q.fused_iters >= prev)
      return fail(SODA_HIP_ERR_INVALID,
                  "plan: passes must be sorted by fused_iters, descending");
    prev = q.fused_iters;
    if (q.num_kernels < 1 || q.num_kernels > SODA_HIP_MAX_PASS_KERNELS)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad pass kernel count");
    for (int k = 0; k < q.num_kernels; ++k)
      if (q.kernel[k] < 0 || q.kernel[k] >= p->num_kernels)
        return fail(SODA_HIP_ERR_INVALID, "plan: bad pass kernel index");
  }
  if (p->passes[p->num_passes - 1].fused_iters != 1)
    return fail(SODA_HIP_ERR_INVALID, "plan: last pass must advance 1 iteration");
  if (p->has_reach && (p->reach_lo < 0 || p->reach_hi < 0))
    return fail(SODA_HIP_ERR_INVALID, "plan: negative reach");
  if (p->residual.present) {
    // residual kernels belong to no pass; twins are read only here
    if (p->num_inputs != p->num_outputs ||
        p->num_outputs > SODA_HIP_MAX_RES_PAIRS || p->batched)
      return fail(SODA_HIP_ERR_INVALID,
                  "plan: a residual needs as many outputs as inputs, at most "
                  "SODA_HIP_MAX_RES_PAIRS, and no batch");
    if (p->residual.kernel < 0 || p->residual.kernel >= p->num_kernels ||
        p->residual.zero_kernel < 0 ||
        p->residual.zero_kernel >= p->num_kernels ||
        p->residual.zero_kernel == p->residual.kernel)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad residual kernel index");
    for (int k = 0; k < p->num_kernels; ++k)
      if (p->kernels[k].twin < -1 || p->kernels[k].twin >= p->num_kernels ||
          p->kernels[k].twin == k)
        return fail(SODA_HIP_ERR_INVALID, "plan: bad twin index");
    for (int i = 0; i < p->num_passes; ++i)
      for (int k = 0; k < p->passes[i].num_kernels; ++k) {
        const int kk = p->passes[i].kernel[k];
        if (kk == p->residual.kernel || kk == p->residual.zero_kernel)
          return fail(SODA_HIP_ERR_INVALID,
                      "plan: the residual kernel belongs to no pass");
        for (int q = 0; q < p->num_kernels; ++q)
          if (p->kernels[q].twin == kk)
            return fail(SODA_HIP_ERR_INVALID,
                        "plan: a twin belongs to no pass");
      }
  }
  return SODA_HIP_OK;
}

int soda_hip_program_create(const void* code, size_t code_size,
                            const soda_hip_plan_t* plan, int32_t device,
                            soda_hip_program_t** program) {
  if (!code || !code_size || !plan || !program)
    return fail(SODA_HIP_ERR_INVALID, "program_create: NULL argument");
  *program = nullptr;
  int rc = check_plan(plan);
  if (rc) return rc;
  int n = 0;
  rc = soda_hip_device_count(&n);
  if (rc) return rc;
  if (n < 1) return fail(SODA_HIP_ERR_NODEVICE, "no GPU visible");
  if (device < 0 || device >= n)
    return fail(SODA_HIP_ERR_INVALID, "program_create: no such device");
  HIP_TRY(hipSetDevice(device));
  soda_hip_program* p = new (std::nothrow) soda_hip_program;
  if (!p) return fail(SODA_HIP_ERR_NOMEM, "new program");
  p->plan = *plan;
  p->device = device;
  hipError_t e = hipModuleLoadData(&p->module, code);
  if (e != hipSuccess) {
    delete p;
    return hip_fail(e, "hipModuleLoadData");
  }
  p->functions.resize(plan->num_kernels);
  for (int k = 0; k < plan->num_kernels; ++k) {
    e = hipModuleGetFunction(&p->functions[k], p->module, plan->kernels[k].name);
    if (e != hipSuccess) {
      std::string what = std::string("hipModuleGetFunction(") +
                         plan->kernels[k].name + ")";
      (void)hipModuleUnload(p->module);
      delete p;
      return hip_fail(e, what.c_str());
    }
  }
  p->auto_calibrate = !getenv("SODA_HIP_NO_CALIBRATE");
  p->locals.resize(plan->num_locals);
  p->temps.resize(plan->num_outputs);
  p->temps2.resize(plan->num_outputs);
  p->until_tmp.resize(plan->num_outputs);
  p->host_in.resize(plan->num_inputs);
  p->host_prm.resize(plan->num_params);
  p->host_out.resize(plan->num_outputs);
  *program = p;
  return SODA_HIP_OK;
}

int soda_hip_program_destroy(soda_hip_program_t* p) {
  if (!p) return SODA_HIP_OK;
  (void)hipSetDevice(p->device);
  for (auto* v : {&p->locals, &p->temps, &p->temps2, &p->until_tmp,
                  &p->host_in, &p->host_out, &p->host_prm})
    for (auto& b : *v)
      if (b.ptr) (void)hipFree(b.ptr);
  if (p->until_struct.ptr) (void)hipFree(p->until_struct.ptr);
  for (int i = 0; i < 2; ++i) {
    if (p->ev_pre[i]) (void)hipEventDestroy(p->ev_pre[i]);
    if (p->ev_bnd[i]) (void)hipEventDestroy(p->ev_bnd[i]);
  }
  if (p->side) (void)hipStreamDestroy(p->side);
  for (auto& st : p->hstream)
    if (st) (void)hipStreamDestroy(st);
  p->ring_in.release();
  p->ring_out.release();
  for (auto& b : p->band_out)
    if (b.ptr) (void)hipFree(b.ptr);
  for (auto& e : p->hevents) (void)hipEventDestroy(e);
  if (p->module) (void)hipModuleUnload(p->module);
  delete p;
  return SODA_HIP_OK;
}

// ---- launch geometry --------------------------------------------------------
// MI355X: 256 CUs x 4 SIMDs; 512 VGPRs per lane per SIMD in granules of 8
// (MI355X_MICROARCH.md, Register files); sustained HBM rate of a streaming
// kernel of this family ~6.3 TB/s (profiles/).
namespace {

const int kSimds = 1024;
// Constants of the launch-time model, fitted (tools/fit_model.py, least squares
// on the log ratio) to 128 measured pass times -- jacobi2d T = 1..12 on eight
// extents from 8192 x 600 to 8192^2, with DPP and with mixed DPP / swizzle
// lane shifts, heat3d T = 1, 2 on four (profiles/r03_model_data.jsonl,
// r03_model_data2.jsonl): rms error 9 % (15-17 % with round 2's hand fits), and
// the schedules the model picks for 100 iterations cost at most 6 % more than
// the ones picked by the clock on every one of those extents (the hand fits:
// +19-20 % on the 1120- and 1224-row slabs of an 8-GPU run).
// tests/test_hip_parity.py::test_model_schedule_is_close_to_the_calibrated_one
// re-checks that on the GPU.
const double kHbmBytesPerNs = 6369.0;
const double kLaunchNs = 2547.0;
const double kWaveNs = 391.0;          // per wave per SIMD of the grid
const double kNormP = 2.708;           // time = (issue^p + memory^p)^(1/p)
const int64_t kBufWindowMax = 1ll << 30;      // SODA_BUF_WINDOW_MAX, soda_rt.h

int waves_per_simd(int vgprs) {
  int alloc = vgprs < 8 ? 8 : (vgprs + 7) / 8 * 8;
  int w = 512 / alloc;
  return w < 1 ? 1 : w > 8 ? 8 : w;
}

// issue time a wave costs its SIMD, relative to one of >= 3 resident waves
// (the chunk rule's own weights: they rank chunk lengths of ONE kernel, were
// tuned by kernel sweeps, and stay as they are)
double issue_share(int64_t k) { return k == 1 ? 2.0 : k == 2 ? 1.2 : 1.0; }
// the same for the time model, fitted together with the constants above
double time_share(int64_t k) {
  return k == 1 ? 1.312 : k == 2 ? 1.475 : k == 3 ? 1.365 : 1.046;
}

// Length (cells along the marched dimension) one wave should own.  The waves
// of a launch are dealt evenly over the SIMDs, a SIMD's waves share its issue
// slots, and every wave pays `warm` pipeline warm-up steps on top of its
// chunk, so  time ~ k * eff(k) * (chunk + warm),  k = waves per SIMD.  One
// wave alone on a SIMD issues at half rate, two still leave bubbles; a kernel
// that fuses few iterations is latency-bound and wants >= 4 waves per SIMD.
// A register-limited grid that fills the last 2-3 % of its wave slots runs
// slower than one a row longer that leaves them free (measured).
int32_t tuned_chunk(const soda_hip_kernel_desc_t& d, const int32_t* tile,
                    const int32_t* extent, int dim, int64_t others) {
  const int axis = d.march_dim - 1;
  const int32_t n = extent[axis];
  const int wpb = (d.block[0] * d.block[1] * d.block[2] + 63) / 64;
  const int along = d.waves_along > 0 ? d.waves_along : 1;
  // Peeled warm-up steps compute little but still LOAD their rows.  Where
  // peeling saves (nearly) ALL of a long warm-up -- a one-iteration kernel with
  // a tall window, whose stages all start at the end of it: xcorr, 18 of 18
  // steps -- "warm-up costs nothing" would shorten the chunks to 8 rows, each
  // row read 3.25 times (measured: 123 us against 59 at 64 rows, 72 at 128,
  // profiles/r03_sweep_xcorr_slide_chunk.json).  Such a kernel is bound by its
  // loads: its warm-up counts in full, and like the other load-bound kernels
  // it gets many short waves.
  const bool load_only_warm = d.warm > 12 && d.warm_saved >= 0.75 * d.warm;
  const double warm = load_only_warm ? d.warm : d.warm - d.warm_saved;
  (void)tile; (void)dim;
  const int cap = waves_per_simd(d.vgprs);
  if (d.pipe > 1) {
    // stage-pipelined blocks: the warm-up is paid once per block; ~3.5x the
    // warm-up is best on every grid -- but never a grid that needs a second,
    // nearly empty round of blocks (a block holds one wave slot on `pipe`
    // SIMDs; measured: 2592 blocks on 1792 slots cost 15 %)
    int32_t target = (int32_t)(3.5 * d.warm) > 64 ? (int32_t)(3.5 * d.warm) : 64;
    int64_t chunks = (n + target - 1) / target;
    if (chunks < 1) chunks = 1;
    const int64_t slots = (int64_t)kSimds * cap / d.pipe;
    int64_t blocks = others * chunks;
    if (blocks > slots * 0.975 && blocks < slots * 1.6) {
      chunks = (int64_t)(slots * 0.975) / others;
      if (chunks < 1) chunks = 1;
    }
    return (int32_t)((n + chunks - 1) / chunks);
  }
  const int k_min = d.warm <= 12 ? 4 : 2;
  double best_cost = 0;
  int32_t best = 0;
  // Candidates: the cost below grows with the chunk length while the number of
  // chunks stays the same, so only the shortest chunk of every chunk COUNT can
  // win -- O(sqrt n) candidates instead of n (a 2M-row stream took 59 ms of
  // host time per run this way, a launch must not)
  for (int32_t chunk = n < 8 ? n : 8; chunk <= n;) {
    int64_t chunks = (n + chunk - 1) / chunk;
    int64_t blocks = others * ((chunks + along - 1) / along);
    int64_t waves = blocks * wpb;
    double cost;
    const int64_t slots = (int64_t)cap * kSimds;
    if (waves <= slots) {
      int64_t k = (waves + kSimds - 1) / kSimds;
      // (one wave per SIMD has nothing to pack: a full grid is fine there --
      // heat3d T = 2 at 260 VGPRs, 1024 waves of 128 planes: 195 us, two
      // rounds of 64-plane waves 205)
      if (cap > 1) {
        if (k >= cap && waves > 0.975 * k * kSimds) ++k;
        if (k < k_min) k = k_min;
      }
      cost = k * issue_share(k) * (chunk + warm);
    } else {
      // more waves than fit at once: whole rounds of `cap` waves per SIMD,
      // then a ragged one whose few waves issue at a lone wave's rate
      // (heat3d T = 2, 2-wave blocks, 245 VGPRs: 19 chunks = 2.4 rounds took
      // 243 us, 16 chunks = 2 rounds 218 us)
      const int64_t full = waves / slots, rem = waves - full * slots;
      cost = full * cap * issue_share(cap) * (chunk + warm);
      if (rem > 0) {
        const int64_t rk = (rem + kSimds - 1) / kSimds;
        cost += rk * issue_share(rk) * (chunk + warm);
      }
    }
    if (!best || cost < best_cost || (cost == best_cost && chunk > best)) {
      best_cost = cost;
      best = chunk;
    }
    if (chunks <= 1) break;
    // the shortest chunk that makes one chunk fewer
    const int64_t next = (n + chunks - 2) / (chunks - 1);
    chunk = next > chunk ? (int32_t)next : chunk + 1;
  }
  // latency-bound: more, shorter waves (not for a kernel the registers allow
  // one wave per SIMD of: it has no second wave to hide anything behind)
  if ((d.warm <= 12 || load_only_warm) && best > 64 && cap > 1) best = 64;
  int64_t chunks = (n + best - 1) / best;
  return (int32_t)((n + chunks - 1) / chunks);   // same count, equal lengths
}

// `batch` grids of `extent` in one launch (soda_hip_run_device_batch): as many
// times the independent tiles for the chunk rule, the cells and the waves for
// the time model; what a kernel can run at all -- row lengths, the buffer
// window, which is relative to an item's own base -- is judged per item
int kernel_geometry(const soda_hip_kernel_desc_t& d, const int32_t* extent,
                    int dim, int32_t batch, Geometry* g) {
  char buf[384];
  int64_t cells = batch;
  for (int i = 0; i < SODA_HIP_MAX_DIM; ++i) {
    g->tile[i] = i < dim ? d.tile[i] : 1;
    if (i < dim) cells *= extent[i];
  }
  g->ns = 0;
  if (d.vec > 1 && extent[0] % d.vec) {
    snprintf(buf, sizeof buf,
             "%s was built for rows that are a multiple of %d cells; extent[0] "
             "= %d is not (rebuild the program for this extent)", d.name, d.vec,
             extent[0]);
    return fail(SODA_HIP_ERR_INVALID, buf);
  }
  if (d.max_extent0 > 0 && extent[0] > d.max_extent0) {
    snprintf(buf, sizeof buf,
             "%s was built for rows of at most %d cells (one block covers the "
             "row); extent[0] = %d (rebuild the program for this extent)",
             d.name, d.max_extent0, extent[0]);
    return fail(SODA_HIP_ERR_INVALID, buf);
  }
  double rows_factor = 1.0;
  double valu_ns = 0, wave_ns = 0;
  if (d.march_dim > 0) {
    if (d.march_dim > dim)
      return fail(SODA_HIP_ERR_INVALID, "plan: bad march_dim");
    const int axis = d.march_dim - 1;
    const int along = d.waves_along > 0 ? d.waves_along : 1;
    const int wpb = (d.block[0] * d.block[1] * d.block[2] + 63) / 64;
    int64_t others = batch;
    for (int i = 0; i < dim; ++i)
      if (i != axis) others *= (extent[i] + g->tile[i] - 1) / g->tile[i];
    int32_t per_wave = g->tile[axis] / along;
    if (per_wave < 1) per_wave = 1;
    if (!d.chunk_fixed && d.vgprs > 0)
      per_wave = tuned_chunk(d, g->tile, extent, dim, others);
    if (d.window_extra >= 0) {
      int64_t plane = d.max_elem > 0 ? d.max_elem : 8;
      for (int i = 0; i < axis; ++i) plane *= extent[i];
      int64_t limit = kBufWindowMax / plane - d.window_extra;
      if (limit < 1) {
        snprintf(buf, sizeof buf,
                 "%s: one plane of this extent (%lld bytes) exceeds the 1 GiB "
                 "buffer window of the marching kernels; use the `direct` "
                 "strategy", d.name, (long long)plane);
        return fail(SODA_HIP_ERR_INVALID, buf);
      }
      if (d.chunk_fixed) {
        // a fixed chunk keeps its length.  The kernels clip a chunk's windows
        // to the grid (m_end, in_end <= nm): on a grid shorter than the chunk
        // it is the grid's length that has to fit
        const int64_t span = per_wave < extent[axis] ? per_wave : extent[axis];
        if (span > limit) {
          snprintf(buf, sizeof buf,
                   "%s: chunks of %d planes exceed the 1 GiB buffer window on "
                   "this extent (at most %lld)", d.name, per_wave,
                   (long long)limit);
          return fail(SODA_HIP_ERR_INVALID, buf);
        }
      } else if (per_wave > limit) {
        per_wave = (int32_t)limit;
      }
    }
    g->tile[axis] = per_wave * along;
    const int32_t n = extent[axis];
    const int64_t chunks = (n + per_wave - 1) / per_wave;
    const int64_t waves = others * ((chunks + along - 1) / along) * wpb;
    const int pipe = d.pipe > 0 ? d.pipe : 1;
    double steps = per_wave + d.warm - d.warm_saved;
    if (steps < 1) steps = 1;
    // SIMD issue time in units of one wave's row step: whole rounds of as
    // many waves as the registers allow, then the ragged rest (tuned_chunk)
    const int64_t slots = (int64_t)(d.vgprs > 0 ? waves_per_simd(d.vgprs) : 8) *
                          kSimds;
    const int64_t full = waves / slots, rem = waves - full * slots;
    double share = full * (double)(slots / kSimds) * time_share(slots / kSimds);
    if (rem > 0 || full == 0) {
      int64_t rk = (rem + kSimds - 1) / kSimds;
      if (rk < 1) rk = 1;
      share += rk * time_share(rk);
    }
    valu_ns = share * steps * d.step_ns / pipe;
    rows_factor = (per_wave + (double)d.warm) / per_wave;
    wave_ns = kWaveNs * (double)waves / kSimds;
  }
  if (d.step_ns > 0 || d.bytes_per_cell > 0) {
    const double lanes = d.lane_redundancy > 1 ? d.lane_redundancy : 1.0;
    // reads are re-fetched for halo lanes and warm-up rows, writes are not
    const double bytes = cells * (double)d.bytes_per_cell *
                         (0.5 * lanes * rows_factor + 0.5);
    const double mem_ns = bytes / kHbmBytesPerNs;
    g->ns = pow(pow(valu_ns, kNormP) + pow(mem_ns, kNormP), 1.0 / kNormP) +
            kLaunchNs + wave_ns;
  }
  return SODA_HIP_OK;
}

// tiles of every kernel and time of every pass for `extent`
int plan_geometry(const soda_hip_plan_t& plan, const int32_t* extent,
                  int32_t batch, std::vector<Geometry>* geo,
                  std::vector<double>* pass_ns) {
  geo->resize(plan.num_kernels);
  for (int k = 0; k < plan.num_kernels; ++k)
    if (int rc = kernel_geometry(plan.kernels[k], extent, plan.dim, batch,
                                 &(*geo)[k]))
      return rc;
  pass_ns->assign(plan.num_passes, 0.0);
  for (int i = 0; i < plan.num_passes; ++i) {
    double t = 0;
    bool modelled = true;
    for (int j = 0; j < plan.passes[i].num_kernels; ++j) {
      const Geometry& g = (*geo)[plan.passes[i].kernel[j]];
      if (g.ns <= 0) modelled = false;
      t += g.ns;
    }
    (*pass_ns)[i] = modelled ? t : 0.0;
  }
  return SODA_HIP_OK;
}

}  // namespace

}  // extern "C"

namespace {

// A launch may cover a marching kernel's chunks with a run of them left out
// (kargs skip_from / skip_count): `count` block tiles along dimension `ax`.
struct TileRange {
  int ax;
  int32_t skip_from, skip_count, count;
};

// a residual kernel's arguments: `k(soda_hip_kargs_t a, soda_hip_residual_t* r,
// soda_hip_resbox_t box)`, laid out as the kernel-argument segment lays them
// out (each at its natural alignment: 8, 8, 4)
struct ResidualArgs {
  soda_hip_kargs_t a;
  void* r;
  soda_hip_resbox_t box;
};

// res_dev != nullptr: kernel k is a twin and takes the residual arguments
int launch(soda_hip_program* p, int k, const soda_hip_kargs_t& base,
           const int32_t* tile, hipStream_t stream,
           const TileRange* range = nullptr, int32_t batch = 1,
           void* res_dev = nullptr, const soda_hip_resbox_t* box = nullptr) {
  const soda_hip_kernel_desc_t& d = p->plan.kernels[k];
  ResidualArgs all;
  soda_hip_kargs_t& args = all.a;
  args = base;
  int64_t blocks = 1;
  for (int i = 0; i < SODA_HIP_MAX_DIM; ++i) {
    int32_t t = i < p->plan.dim ? tile[i] : 1;
    args.tile[i] = t;
    args.ntile[i] = (args.extent[i] + t - 1) / t;
    if (range && range->ax == i) args.ntile[i] = range->count;
    blocks *= args.ntile[i];
  }
  args.skip_from = range ? range->skip_from : 0;
  args.skip_count = range ? range->skip_count : 0;
  if (blocks < 1 || blocks > 0x7fffffffLL)
    return fail(SODA_HIP_ERR_INVALID, "grid does not fit a 1-D launch");
  size_t size = sizeof args;
  if (res_dev) {
    all.r = res_dev;
    all.box = *box;
    size = sizeof all;
  }
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &all,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  // (a batched kernel takes blockIdx.y as the item; every other kernel is
  // launched with batch = 1 and never looks)
  HIP_TRY(hipModuleLaunchKernel(p->functions[k], (unsigned)blocks,
                                (unsigned)batch, 1,
                                d.block[0], d.block[1], d.block[2],
                                d.lds_bytes, stream, nullptr, extra));
  return SODA_HIP_OK;
}

// `<app>_residual` over the dense arrays of `base` (outputs: cur, inputs:
// prev)
int launch_residual(soda_hip_program* p, const soda_hip_kargs_t& base,
                    hipStream_t stream, void* res_dev,
                    const soda_hip_resbox_t& box) {
  const int k = p->plan.residual.kernel;
  const soda_hip_kernel_desc_t& d = p->plan.kernels[k];
  ResidualArgs all;
  all.a = base;
  all.r = res_dev;
  all.box = box;
  // grid: the segments of block x vec cells a row has, times as many rows in
  // flight as fill the GPU a few times over (the kernel strides over the
  // rest): a whole number of rows' worth of blocks, which is what lets the
  // kernel find its segment without a division per fragment
  const int64_t seg = (int64_t)d.block[0] * (d.vec > 0 ? d.vec : 1);
  const int64_t nx = (base.extent[0] + seg - 1) / seg;
  int64_t rows = 1;
  for (int i = 1; i < p->plan.dim; ++i) rows *= base.extent[i];
  if (rows > 0x7fffffffLL || nx > 0x7fffffLL)
    return fail(SODA_HIP_ERR_INVALID, "residual: grid does not fit a launch");
  // (about a thousand blocks: every wave ends in up to four atomics on the
  // one struct, and tens of thousands of those cost more than the arrays'
  // bytes -- jacobi2d 8192^2: 918 us over a plain run on 8192 blocks, 306 on
  // 1024)
  int64_t in_flight = 1024 / nx;
  if (in_flight < 1) in_flight = 1;
  if (in_flight > rows) in_flight = rows;
  const int64_t blocks = nx * in_flight;
  size_t size = sizeof all;
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &all,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(p->functions[k], (unsigned)blocks, 1, 1,
                                d.block[0], d.block[1], d.block[2],
                                d.lds_bytes, stream, nullptr, extra));
  return SODA_HIP_OK;
}

// ---- exact norms (soda_hip_norms_t; the kernels: soda_rt_norms.h) -----------
// the kernels' one argument, as soda_rt_norms.h declares it
struct NormsArgs {
  const void* cur;
  const void* prev;
  void* acc;
  int32_t extent[SODA_HIP_MAX_DIM];
  int32_t lo[SODA_HIP_MAX_DIM];
  int32_t hi[SODA_HIP_MAX_DIM];
};

int norms_zero(soda_hip_norms_handle* h, void* acc_dev, hipStream_t stream) {
  struct {
    void* acc;
    uint64_t kind;     // word 0 of the struct: kind | reserved = 0
  } args = {acc_dev, (uint64_t)h->kind};
  size_t size = sizeof args;
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(h->zero, 1, 1, 1, 256, 1, 1, 0, stream,
                                nullptr, extra));
  return SODA_HIP_OK;
}

// the cells [lo, hi) of dense `cur` against dense `prev`, added to *acc_dev
int norms_accumulate(soda_hip_norms_handle* h, const void* cur,
                     const void* prev, const int32_t* extent,
                     const int32_t* lo, const int32_t* hi, void* acc_dev,
                     hipStream_t stream) {
  NormsArgs args;
  memset(&args, 0, sizeof args);
  args.cur = cur;
  args.prev = prev;
  args.acc = acc_dev;
  int64_t rows = 1;
  bool empty = false;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    const bool in = d < h->dim;
    args.extent[d] = in ? extent[d] : 1;
    args.lo[d] = in ? lo[d] : 0;
    args.hi[d] = in ? hi[d] : 1;
    if (args.extent[d] < 1 || args.lo[d] < 0 || args.hi[d] > args.extent[d])
      return fail(SODA_HIP_ERR_INVALID,
                  "norms_accumulate: the box does not lie in the arrays; "
                  "nothing was launched");
    if (args.hi[d] <= args.lo[d]) empty = true;
    if (d > 0) rows *= args.extent[d];
  }
  if (empty) return SODA_HIP_OK;
  // the widest fragment that divides the row length and that both arrays are
  // aligned to (the narrowest is one cell: always there)
  const uintptr_t both = reinterpret_cast<uintptr_t>(cur) |
                         reinterpret_cast<uintptr_t>(prev);
  if (both % (uintptr_t)h->elem)
    return fail(SODA_HIP_ERR_INVALID,
                "norms_accumulate: an array is not aligned to its cell size; "
                "nothing was launched");
  hipFunction_t fn = nullptr;
  int32_t vec = 1;
  for (const auto& w : h->widths)
    if (args.extent[0] % w.first == 0 &&
        both % ((uintptr_t)w.first * h->elem) == 0) {
      vec = w.first;
      fn = w.second;
      break;
    }
  if (!fn) return fail(SODA_HIP_ERR_INVALID, "norms_accumulate: no kernel");
  // grid: as launch_residual -- the segments of 256 fragments a row has, times
  // as many rows in flight as make about a thousand blocks
  // (a block takes `rpb` whole rows at a time where a row has fewer fragments
  // than the block has lanes: soda_rt_norms.h computes the same two numbers)
  const int64_t frags = args.extent[0] / vec;
  const int64_t rpb = frags < 256 ? 256 / frags : 1;
  const int64_t nx = rpb > 1 ? 1 : (frags + 255) / 256;
  if (rows > 0x7fffffffLL || nx > 0x7fffffLL)
    return fail(SODA_HIP_ERR_INVALID,
                "norms_accumulate: grid does not fit a launch");
  const int64_t groups = (rows + rpb - 1) / rpb;
  int64_t in_flight = 1024 / nx;
  if (in_flight < 1) in_flight = 1;
  if (in_flight > groups) in_flight = groups;
  size_t size = sizeof args;
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)(nx * in_flight), 1, 1, 256, 1, 1,
                                0, stream, nullptr, extra));
  return SODA_HIP_OK;
}

// What follows the one-iteration pass of a residual run that no twin serves:
// `<app>_residual`, or the norms kernel once per pair (cur: the output slot,
// prev: the input slot of the launch's arrays)
int launch_generic(soda_hip_program* p, const soda_hip_kargs_t& args,
                   hipStream_t stream, const soda_detail::ResidualRun& res,
                   const soda_hip_resbox_t& box) {
  if (!res.norms) return launch_residual(p, args, stream, res.dev, box);
  const int out0 = p->plan.num_inputs;
  for (int o = 0; o < p->plan.num_outputs; ++o)
    if (int rc = norms_accumulate(res.norms, args.buf[out0 + o], args.buf[o],
                                  args.extent, box.lo[o], box.hi[o], res.dev,
                                  stream))
      return rc;
  return SODA_HIP_OK;
}

// The cells a residual over `iterate` iterations counts (soda_hip.h,
// soda_hip_residual_plan_t): the plan's recurrence run `iterate` times from
// zero windows, the box the array less the window, clipped like every valid
// box (lo inside the array, hi >= lo).  A round costs pairs^2 x dim steps.
void residual_box(const soda_hip_plan_t& plan, const int32_t* ext,
                  int32_t iterate, soda_hip_resbox_t* box) {
  const soda_hip_residual_plan_t& r = plan.residual;
  const int n = plan.num_outputs, dim = plan.dim;
  int64_t lo[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM] = {};
  int64_t hi[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM] = {};
  const int64_t cap = (int64_t)1 << 40;    // far beyond any extent
  for (int32_t it = 0; it < iterate && !r.whole; ++it) {
    int64_t nlo[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
    int64_t nhi[SODA_HIP_MAX_RES_PAIRS][SODA_HIP_MAX_DIM];
    for (int o = 0; o < n; ++o)
      for (int d = 0; d < dim; ++d) {
        int64_t l = r.base_lo[o][d], h = r.base_hi[o][d];
        for (int i = 0; i < n; ++i) {
          if (r.dep_lo[o][i][d] != SODA_HIP_RES_NONE) {
            const int64_t v = r.dep_lo[o][i][d] + (lo[i][d] < 0 ? lo[i][d] : 0);
            if (v < l) l = v;
          }
          if (r.dep_hi[o][i][d] != SODA_HIP_RES_NONE) {
            const int64_t v = r.dep_hi[o][i][d] + (hi[i][d] > 0 ? hi[i][d] : 0);
            if (v > h) h = v;
          }
        }
        nlo[o][d] = l < -cap ? -cap : l;
        nhi[o][d] = h > cap ? cap : h;
      }
    memcpy(lo, nlo, sizeof lo);
    memcpy(hi, nhi, sizeof hi);
  }
  memset(box, 0, sizeof *box);
  for (int o = 0; o < n; ++o)
    for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
      const int64_t e = d < dim ? ext[d] : 1;
      int64_t l = d < dim && !r.whole && lo[o][d] < 0 ? -lo[o][d] : 0;
      int64_t h = e - (d < dim && !r.whole && hi[o][d] > 0 ? hi[o][d] : 0);
      if (l > e) l = e;
      if (h < l) h = l;
      box->lo[o][d] = (int32_t)l;
      box->hi[o][d] = (int32_t)h;
    }
}

// The same for a slab of a larger grid (soda_hip.h,
// soda_hip_plan_residual_slab_box): the box of the GLOBAL grid, of which the
// slab counts the rows [keep_lo, keep_hi) of its last dimension, in the
// coordinates of the slab's arrays (cell 0 at `origin`) and clipped to them.
// Slabs whose kept rows partition the global rows partition the global box.
void residual_slab_box(const soda_hip_plan_t& plan, const int32_t* gext,
                       const int32_t* origin, const int32_t* ext,
                       int32_t keep_lo, int32_t keep_hi, int32_t iterate,
                       soda_hip_resbox_t* box) {
  residual_box(plan, gext, iterate, box);
  const int dim = plan.dim;
  for (int o = 0; o < plan.num_outputs; ++o)
    for (int d = 0; d < dim; ++d) {
      int64_t l = (int64_t)box->lo[o][d] - origin[d];
      int64_t h = (int64_t)box->hi[o][d] - origin[d];
      int64_t a = 0, b = ext[d];
      if (d == dim - 1) {
        if (keep_lo > a) a = keep_lo;
        if (keep_hi < b) b = keep_hi;
        if (b < a) b = a;
      }
      if (l < a) l = a;
      if (l > b) l = b;
      if (h > b) h = b;
      if (h < l) h = l;
      box->lo[o][d] = (int32_t)l;
      box->hi[o][d] = (int32_t)h;
    }
}

// The box for a launch on rows [row0, row0 + rows) of the last dimension:
// kernels count in the coordinates of the arrays their launch addresses.
soda_hip_resbox_t shifted_box(const soda_hip_plan_t& plan,
                              const soda_hip_resbox_t& box, int32_t row0,
                              int32_t rows) {
  soda_hip_resbox_t out = box;
  const int ax = plan.dim - 1;
  for (int o = 0; o < plan.num_outputs; ++o) {
    int64_t l = (int64_t)box.lo[o][ax] - row0, h = (int64_t)box.hi[o][ax] - row0;
    if (l < 0) l = 0;
    if (l > rows) l = rows;
    if (h > rows) h = rows;
    if (h < l) h = l;
    out.lo[o][ax] = (int32_t)l;
    out.hi[o][ax] = (int32_t)h;
  }
  return out;
}

int64_t ceil_div(int64_t a, int64_t b) { return a <= 0 ? 0 : (a + b - 1) / b; }
int64_t floor_div(int64_t a, int64_t b) { return a <= 0 ? 0 : a / b; }

}  // namespace

namespace soda_detail {

int schedule(const soda_hip_plan_t& plan, const std::vector<double>& pass_ns,
             int32_t iterate, int32_t* count, int32_t* total) {
  // modelled times for this extent where every pass has one, else the plan's
  // static relative costs, else greedy
  std::vector<double> cost(plan.num_passes, 0.0);
  bool modelled = true;
  for (int i = 0; i < plan.num_passes; ++i)
    modelled = modelled && pass_ns[i] > 0;
  bool costed = modelled;
  for (int i = 0; i < plan.num_passes; ++i) {
    cost[i] = modelled ? pass_ns[i] : plan.passes[i].cost;
    costed = costed || cost[i] > 0;
  }
  *total = 0;
  if (!costed || iterate > (1 << 20)) {      // greedy, deepest first
    int32_t remaining = iterate;
    for (int i = 0; i < plan.num_passes; ++i) {
      count[i] = remaining / plan.passes[i].fused_iters;
      remaining -= count[i] * plan.passes[i].fused_iters;
      *total += count[i];
    }
    return remaining ? fail(SODA_HIP_ERR_INVALID, "iterate not schedulable")
                     : SODA_HIP_OK;
  }
  // unbounded knapsack over the iteration count: best[n] = least cost of n
  // iterations, pick[n] = the pass used last
  std::vector<double> best(iterate + 1, 1e300);
  std::vector<int8_t> pick(iterate + 1, -1);
  best[0] = 0.0;
  for (int32_t n = 1; n <= iterate; ++n)
    for (int i = 0; i < plan.num_passes; ++i) {
      const int32_t t = plan.passes[i].fused_iters;
      const double c = cost[i] > 0 ? cost[i] : 1e12;
      if (t <= n && best[n - t] < 1e299 && best[n - t] + c < best[n]) {
        best[n] = best[n - t] + c;
        pick[n] = (int8_t)i;
      }
    }
  if (pick[iterate] < 0)
    return fail(SODA_HIP_ERR_INVALID, "iterate not schedulable");
  for (int i = 0; i < plan.num_passes; ++i) count[i] = 0;
  for (int32_t n = iterate; n > 0; n -= plan.passes[pick[n]].fused_iters) {
    ++count[pick[n]];
    ++*total;
  }
  return SODA_HIP_OK;
}

int residual_order(const soda_hip_plan_t& plan,
                   const std::vector<double>& pass_ns, int32_t iterate,
                   int32_t* count, int32_t* total, int* res_pass,
                   bool* res_twin, bool generic_only) {
  const char* g = getenv("SODA_HIP_RESIDUAL_GENERIC");
  const bool generic = generic_only || (g && !strcmp(g, "1"));
  *res_pass = -1;
  *res_twin = false;
  for (int i = 0; i < plan.num_passes && !generic && *res_pass < 0; ++i)
    if (count[i] > 0 && plan.passes[i].num_kernels == 1 &&
        plan.kernels[plan.passes[i].kernel[0]].twin >= 0) {
      *res_pass = i;
      *res_twin = true;
    }
  if (*res_pass >= 0) return SODA_HIP_OK;
  const int one = plan.num_passes - 1;   // fused_iters 1 (check_plan)
  if (!count[one]) {
    for (int i = 0; i < plan.num_passes; ++i) count[i] = 0;
    *total = 0;
    if (iterate > 1)
      if (int rc = schedule(plan, pass_ns, iterate - 1, count, total)) return rc;
    ++count[one];
    ++*total;
  }
  *res_pass = one;
  return SODA_HIP_OK;
}

int extent_plan(const soda_hip_plan_t& plan,
                std::map<ExtentKey, ExtentPlan>* cache, const int32_t* ext,
                ExtentPlan** out, int32_t batch) {
  ExtentKey key;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) key[d] = ext[d];
  auto it = cache->find(key);
  if (it == cache->end()) {
    ExtentPlan ep;
    if (int rc = plan_geometry(plan, ext, batch, &ep.geo, &ep.model_ns))
      return rc;
    if (cache->size() > 4096) cache->clear();
    it = cache->emplace(key, std::move(ep)).first;
  }
  *out = &it->second;
  return SODA_HIP_OK;
}

}  // namespace soda_detail

static int plan_geometry_c(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t* tiles, float* pass_ns, int32_t batch) {
  if (!plan || !extent) return fail(SODA_HIP_ERR_INVALID, "geometry: NULL argument");
  if (int rc = check_plan(plan)) return rc;
  int32_t ext[SODA_HIP_MAX_DIM];
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    ext[d] = d < plan->dim ? extent[d] : 1;
    if (ext[d] < 1) return fail(SODA_HIP_ERR_INVALID, "geometry: extent < 1");
  }
  std::vector<Geometry> geo;
  std::vector<double> ns;
  if (int rc = plan_geometry(*plan, ext, batch, &geo, &ns)) return rc;
  if (tiles)
    for (int k = 0; k < plan->num_kernels; ++k)
      for (int d = 0; d < SODA_HIP_MAX_DIM; ++d)
        tiles[k * SODA_HIP_MAX_DIM + d] = geo[k].tile[d];
  if (pass_ns)
    for (int i = 0; i < plan->num_passes; ++i) pass_ns[i] = (float)ns[i];
  return SODA_HIP_OK;
}

static int plan_schedule_c(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, int32_t* count, int32_t batch) {
  if (!plan || !extent || !count)
    return fail(SODA_HIP_ERR_INVALID, "schedule: NULL argument");
  if (iterate < 1) return fail(SODA_HIP_ERR_INVALID, "cannot iterate < 1 times");
  if (int rc = check_plan(plan)) return rc;
  int32_t ext[SODA_HIP_MAX_DIM];
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    ext[d] = d < plan->dim ? extent[d] : 1;
    if (ext[d] < 1) return fail(SODA_HIP_ERR_INVALID, "schedule: extent < 1");
  }
  std::vector<Geometry> geo;
  std::vector<double> ns;
  if (int rc = plan_geometry(*plan, ext, batch, &geo, &ns)) return rc;
  int32_t total = 0;
  return schedule(*plan, ns, iterate, count, &total);
}

namespace soda_detail {

// The launches of a run in order: which rows every pass covers (all of them,
// or the cone that can still reach the kept range) and, next to a halo
// exchange, how the first and the last pass are cut in two.
//
// A pass is launched in two parts when it is ONE marching kernel streaming
// along the last dimension: the chunks whose inputs include ghost rows still
// in flight (first pass of the run) or whose rows the neighbours fetch next
// (last pass) form the boundary [0, bnd_lo) U [bnd_hi, chunks), the rest the
// interior.  Any other pass waits, runs whole, and signals.
int plan_launches(const soda_hip_plan_t& plan,
                  std::map<ExtentKey, ExtentPlan>* cache, const int32_t* ext,
                  const int32_t* count, int32_t total, int32_t iterate,
                  const SlabRun* slab, std::vector<PassLaunch>* out,
                  int res_pass, bool res_twin) {
  const int ax = plan.dim - 1;
  const int32_t rows = ext[ax];
  const Cone* cone = slab ? &slab->cone : nullptr;
  out->clear();
  out->reserve(total);
  // the order launched: deepest first -- and, in a run that takes a residual,
  // one launch of the pass that takes it moved to the end.  The cone below is
  // that of THIS order: a deep pass that goes last reads further than the
  // shallow one it displaced, so the passes before it must cover more rows.
  std::vector<int> order;
  order.reserve(total);
  for (int i = 0; i < plan.num_passes; ++i)
    for (int c = 0; c < count[i] - (i == res_pass ? 1 : 0); ++c)
      order.push_back(i);
  if (res_pass >= 0 && res_pass < plan.num_passes && count[res_pass] > 0)
    order.push_back(res_pass);
  int done = 0, done_iters = 0;
  {
    for (; done < (int)order.size(); ++done) {
      const int i = order[done];
      PassLaunch L;
      memset(&L, 0, sizeof L);
      L.pass = i;
      // Rows this pass has to touch.  With a cone: the rows it must DELIVER
      // are those the iterations still to come can carry into the kept range;
      // it is launched on these plus the rows its own iterations read beyond
      // them (their results are written too, and are wrong where the launch
      // saw zeros instead of neighbours -- nothing reads them again).
      int32_t lo = 0, hi = rows;
      const int32_t fused = plan.passes[i].fused_iters;
      done_iters += fused;
      if (cone) {
        const int64_t after = iterate - done_iters;        // iterations to come
        const int64_t a = cone->keep_lo - (after + fused) * (int64_t)cone->reach_lo;
        const int64_t b = cone->keep_hi + (after + fused) * (int64_t)cone->reach_hi;
        if (cone->keep_lo > 0 && a > 0) lo = (int32_t)a;
        if (cone->keep_hi < rows && b < rows) hi = (int32_t)b;
      }
      L.lo = lo;
      L.hi = hi;
      const bool first = done == 0, last = done + 1 == total;
      L.wait = first && slab && slab->ghosts_ready;
      L.record = last && slab && slab->sendable;
      // (a last pass that runs as its twin is cut by the twin's chunks)
      int k0 = plan.passes[i].kernel[0];
      if (last && res_twin && i == res_pass && plan.passes[i].num_kernels == 1 &&
          plan.kernels[k0].twin >= 0)
        k0 = plan.kernels[k0].twin;
      if ((L.wait || L.record) && plan.passes[i].num_kernels == 1 &&
          plan.kernels[k0].march_dim == plan.dim) {
        int32_t sub[SODA_HIP_MAX_DIM];
        for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) sub[d] = ext[d];
        sub[ax] = hi - lo;
        ExtentPlan* use = nullptr;
        if (int rc = extent_plan(plan, cache, sub, &use)) return rc;
        const int64_t lb = use->geo[k0].tile[ax];
        const int64_t nchunk = (hi - lo + lb - 1) / lb;
        int64_t bnd_lo = 0, bnd_hi = nchunk;
        if (L.wait) {
          // chunk c reads rows [c lb - fused reach_lo, (c + 1) lb + fused reach_hi)
          if (slab->ghost_lo > 0)
            bnd_lo = ceil_div(slab->ghost_lo - lo + (int64_t)fused * cone->reach_lo, lb);
          if (slab->ghost_hi > 0)
            bnd_hi = floor_div(rows - slab->ghost_hi - lo -
                               (int64_t)fused * cone->reach_hi, lb);
        }
        if (L.record) {
          // `sendable` promises two things to the exchange that is ordered
          // behind it: the rows the neighbours fetch are complete, and NOTHING
          // launched later in this run writes the result's ghost rows (the
          // exchange overwrites them next).  So the boundary holds the chunks
          // that deliver send rows ...
          if (slab->send_lo > 0) {
            const int64_t v = ceil_div(cone->keep_lo + slab->send_lo - lo, lb);
            if (v > bnd_lo) bnd_lo = v;
          }
          if (slab->send_hi > 0) {
            const int64_t v = floor_div(cone->keep_hi - slab->send_hi - lo, lb);
            if (v < bnd_hi) bnd_hi = v;
          }
          // ... AND every chunk that writes a row outside the kept range, on
          // either side, whether or not that side sends anything.  With a
          // symmetric reach the send rule above already covers them (a side
          // with ghosts is a side that sends); with a one-sided reach (upwind
          // taps: ghosts above, sends below) it does not, and when the run
          // also has nothing to wait for (fresh ghosts: the wait rule is off)
          // the top chunk -- which writes the upper ghost rows -- used to
          // count as interior and could overwrite the rows the next exchange
          // had just received (tools/flake_loop.py, round 4: 2 of 400 skewed
          // trials of the upwind case).
          if (cone->keep_lo > lo) {
            const int64_t v = ceil_div(cone->keep_lo - lo, lb);
            if (v > bnd_lo) bnd_lo = v;
          }
          if (cone->keep_hi < hi) {
            const int64_t v = floor_div(cone->keep_hi - lo, lb);
            if (v < bnd_hi) bnd_hi = v;
          }
        }
        if (bnd_lo > nchunk) bnd_lo = nchunk;
        if (bnd_hi > nchunk) bnd_hi = nchunk;
        L.chunk = (int32_t)lb;
        L.chunks = (int32_t)nchunk;
        L.bnd_lo = (int32_t)bnd_lo;
        L.bnd_hi = (int32_t)bnd_hi;
        L.split = bnd_lo < bnd_hi && (bnd_lo > 0 || bnd_hi < nchunk);
      }
      out->push_back(L);
    }
  }
  return SODA_HIP_OK;
}

// The two parts of a split pass go out on the caller's stream one after the
// other (the part that does not depend on the exchange first).  Measured on
// the middle slab of an 8-GPU run alone on an MI355X
// (profiles/r03_slab_overlap.jsonl): jacobi2d 8192 x 1224, 100 iterations,
// two split passes per step -- 0.333 ms unsplit, 0.367 ms this way, 0.384-0.390
// ms with the boundary part on a stream of its own (SODA_HIP_SPLIT=side: the
// parts then share the GPU, but two hand-overs between hardware queues cost
// more than that buys).
// (read per split pass, not once per process: a host may switch between runs,
// and tests/test_async.py runs both orders in one process)
static bool split_in_order() {
  const char* v = getenv("SODA_HIP_SPLIT");
  return !(v && !strcmp(v, "side"));
}

// the stream and events of split passes, made on first use
static int side_stream(soda_hip_program* p) {
  if (p->side) return SODA_HIP_OK;
  HIP_TRY(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&p->ev_pre[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_bnd[i], hipEventDisableTiming));
  }
  return SODA_HIP_OK;
}

// scratch for the local tensors is needed only if a scheduled pass keeps them
// in memory (marching kernels hold them in registers)
static bool locals_in_memory(const soda_hip_plan_t& plan, const int32_t* count) {
  for (int i = 0; i < plan.num_passes; ++i)
    for (int k = 0; count[i] && k < plan.passes[i].num_kernels; ++k)
      if (plan.kernels[plan.passes[i].kernel[k]].march_dim == 0) return true;
  return false;
}

// Would a run of `total` launches on `cells` x `batch` cells allocate: the
// locals, the ping-pong temporaries, their partners of a trimmed run?
static bool scratch_grows(const soda_hip_program* p, bool need_locals,
                          int32_t total, bool own_pingpong, int64_t cells,
                          int32_t batch) {
  const soda_hip_plan_t& plan = p->plan;
  const int out0 = plan.num_inputs, loc0 = out0 + plan.num_outputs;
  for (int l = 0; need_locals && l < plan.num_locals; ++l)
    if (too_small(p->locals[l],
                  (size_t)cells * batch * plan.elem_size[loc0 + l]))
      return true;
  for (int o = 0; total > 1 && o < plan.num_outputs; ++o) {
    const size_t bytes = (size_t)cells * batch * plan.elem_size[out0 + o];
    if (too_small(p->temps[o], bytes) ||
        (own_pingpong && too_small(p->temps2[o], bytes)))
      return true;
  }
  return false;
}

int program_grows(soda_hip_program* p, const int32_t* ext, int32_t iterate,
                  bool* grows) {
  int32_t count[SODA_HIP_MAX_PASSES];
  if (int rc = soda_hip_program_schedule(p, ext, iterate, count)) return rc;
  int32_t total = 0;
  int64_t cells = 1;
  for (int i = 0; i < p->plan.num_passes; ++i) total += count[i];
  for (int d = 0; d < p->plan.dim; ++d) cells *= ext[d];
  if (scratch_grows(p, locals_in_memory(p->plan, count), total, false, cells, 1))
    *grows = true;
  return SODA_HIP_OK;
}

// ---- a run, step by step (run_core below) -----------------------------------

// The kernel arguments that hold for every launch of the run -- extent,
// strides, the window's place in the global grid -- and the cells of one grid.
static int run_geometry(const soda_hip_plan_t& plan, const RunRequest& rq,
                        soda_hip_kargs_t* base, int64_t* cells) {
  memset(base, 0, sizeof *base);
  *cells = 1;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    int32_t e = d < plan.dim ? rq.extent[d] : 1;
    if (e < 1) return fail(SODA_HIP_ERR_INVALID, "run_device: extent < 1");
    base->extent[d] = e;
    base->stride[d] = *cells;
    *cells *= e;
    base->origin[d] = (rq.origin && d < plan.dim) ? rq.origin[d] : 0;
    base->gextent[d] =
        (rq.global_extent && d < plan.dim) ? rq.global_extent[d] : e;
    if (base->origin[d] < 0 || base->origin[d] + e > base->gextent[d])
      return fail(SODA_HIP_ERR_INVALID,
                  "run_device: the window does not lie in the global grid");
  }
  for (int i = 0; i < plan.num_inputs + plan.num_params; ++i)
    if (!rq.inputs[i])
      return fail(SODA_HIP_ERR_INVALID, "run_device: NULL input");
  for (int i = 0; i < plan.num_outputs; ++i)
    if (!rq.outputs[i])
      return fail(SODA_HIP_ERR_INVALID, "run_device: NULL output");
  return SODA_HIP_OK;
}

int check_run_tensors(const soda_hip_plan_t& plan, bool bank_tensors,
                      void* const* outputs, const void* const* inputs,
                      int64_t cells, int32_t batch) {
  if (bank_tensors) return SODA_HIP_OK;
  const int out0 = plan.num_inputs;
  const int prm0 = out0 + plan.num_outputs + plan.num_locals;
  // Overlap: passes read their inputs while they write their outputs, and
  // ping-pong through the outputs.
  auto bytes_of = [&](int slot) {
    return (uint64_t)cells * (uint64_t)batch * (uint64_t)plan.elem_size[slot];
  };
  auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
  };
  for (int o = 0; o < plan.num_outputs; ++o) {
    for (int i = 0; i < plan.num_inputs; ++i)
      if (overlap(outputs[o], bytes_of(out0 + o), inputs[i], bytes_of(i)))
        return fail(SODA_HIP_ERR_INVALID,
                    std::string("run_device: an output ") +
                        (outputs[o] == inputs[i] ? "aliases" : "overlaps") +
                        " an input (in-place runs are not supported: inputs "
                        "are read while outputs are written); nothing was "
                        "launched");
    for (int k = 0; k < plan.num_params; ++k)
      if (overlap(outputs[o], bytes_of(out0 + o), inputs[plan.num_inputs + k],
                  (uint64_t)plan.param_elems[k] * plan.elem_size[prm0 + k]))
        return fail(SODA_HIP_ERR_INVALID,
                    "run_device: an output overlaps a param array; nothing "
                    "was launched");
    for (int q = 0; q < o; ++q)
      if (overlap(outputs[o], bytes_of(out0 + o), outputs[q],
                  bytes_of(out0 + q)))
        return fail(SODA_HIP_ERR_INVALID,
                    "run_device: two outputs overlap; nothing was launched");
  }
  // Alignment (the geometry makes sure that the row length is a multiple of
  // every kernel's cells per lane: a row, a plane, a slab window or a band
  // then starts on a fragment boundary iff the array does).  A kernel moves a
  // tensor in fragments of `vec` cells, with one instruction of up to 16
  // bytes each -- marching and tile3d kernels through buffer resources
  // (soda_rt.h soda_buf_load_frag / soda_buf_store_frag), direct and ldswin
  // kernels through vector pointers (soda_load_frag / soda_store_frag;
  // ldswin's quads are four 4-byte cells) -- so every tensor must be aligned
  // to min(16, vec x its cell size) for the widest `vec` of the plan; param
  // arrays are read cell by cell.
  int32_t vec = 1;
  for (int k = 0; k < plan.num_kernels; ++k)
    if (plan.kernels[k].vec > vec) vec = plan.kernels[k].vec;
  char buf[256];
  for (int t = 0; t < plan.num_inputs + plan.num_outputs + plan.num_params;
       ++t) {
    const bool prm = t >= plan.num_inputs + plan.num_outputs;
    const int k = t - plan.num_inputs - plan.num_outputs;
    const void* ptr = prm ? inputs[plan.num_inputs + k]
                          : t < out0 ? inputs[t] : outputs[t - out0];
    const int64_t elem = plan.elem_size[prm ? prm0 + k : t];
    int64_t align = prm ? elem : (int64_t)vec * elem;
    if (align > 16) align = 16;
    if (align > 1 && reinterpret_cast<uintptr_t>(ptr) % (uintptr_t)align) {
      snprintf(buf, sizeof buf,
               "run_device: %s %d at %p is not aligned to %d bytes (%d cells "
               "per lane x %d-byte cells, at most 16; params: one cell); "
               "nothing was launched",
               prm ? "param array" : t < out0 ? "input" : "output",
               prm ? k : t < out0 ? t : t - out0, ptr, (int)align,
               prm ? 1 : (int)vec, (int)elem);
      return fail(SODA_HIP_ERR_INVALID, buf);
    }
  }
  return SODA_HIP_OK;
}

// Launches of every pass, their sum, and -- in a residual run -- the pass that
// goes last and whether it runs as its twin.
struct Schedule {
  int32_t count[SODA_HIP_MAX_PASSES];
  int32_t total = 0;
  int res_pass = -1;
  bool res_twin = false;
};

// The multiset of passes that adds up to `iterate` at least total cost (100
// iterations with passes of 12 / 8 / 4 / 1: 7 x 12 + 2 x 8 beats 8 x 12 + 4);
// without costs, as many of the deepest kind as fit, then the next...
// Remembered per (extent, iterate).
static int choose_schedule(soda_hip_program* p, const RunRequest& rq,
                           const int32_t* ext, Schedule* s) {
  const soda_hip_plan_t& plan = p->plan;
  const int32_t iterate = rq.iterate;
  // plans, schedules and measured times of this batch size
  std::map<ExtentKey, ExtentPlan>& extents = extents_of(p, rq.batch);
  std::map<ExtentKey, std::vector<double>>& measured =
      measured_of(p, rq.batch);
  ExtentPlan* ep = nullptr;
  if (int rc = extent_plan(plan, &extents, ext, &ep, rq.batch)) return rc;
  if (rq.force_pass >= 0) {
    if (rq.force_pass >= plan.num_passes ||
        iterate % plan.passes[rq.force_pass].fused_iters)
      return fail(SODA_HIP_ERR_INVALID, "run_core: bad forced pass");
    for (int i = 0; i < plan.num_passes; ++i) s->count[i] = 0;
    s->count[rq.force_pass] = s->total =
        iterate / plan.passes[rq.force_pass].fused_iters;
    return SODA_HIP_OK;   // (never a residual run: run_core checks)
  }
  ExtentKey key;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) key[d] = ext[d];
  auto known = measured.find(key);
  // Never next to a halo exchange (the caller's events say other streams
  // are live: a calibration allocates, frees and synchronises -- it would
  // stall the neighbours and make every rank's schedule depend on who ran
  // beside it), never on a capturing stream (synchronising is illegal
  // there): such runs are scheduled by the model unless the caller
  // calibrated the extent beforehand (soda_hip_program_calibrate).
  const bool beside_exchange =
      rq.slab && (rq.slab->ghosts_ready || rq.slab->sendable);
  const bool may_calibrate =
      p->auto_calibrate && !p->calibrating && !beside_exchange;
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (may_calibrate &&
      hipStreamIsCapturing(static_cast<hipStream_t>(rq.stream), &capture) !=
          hipSuccess) {
    (void)hipGetLastError();
    capture = hipStreamCaptureStatusNone;
  }
  if (may_calibrate && capture == hipStreamCaptureStatusNone && iterate > 1 &&
      plan.num_passes > 1 && plan.num_inputs == plan.num_outputs &&
      known == measured.end()) {
    // first run on this extent: let the clock rank the passes
    p->calibrating = true;
    int rc = soda_hip_program_calibrate_batch(p, ext, rq.batch, 4, rq.stream);
    p->calibrating = false;
    if (rc) return rc;
    if (int rc2 = extent_plan(plan, &extents, ext, &ep, rq.batch)) return rc2;
    known = measured.find(key);
  }
  // measured launch times of this very extent (soda_hip_program_calibrate)
  // outrank the model
  const std::vector<double>& pass_ns =
      known != measured.end() ? known->second : ep->model_ns;
  auto& memo = ep->sched;
  auto hit = memo.find(iterate);
  if (hit == memo.end()) {
    if (int rc = schedule(plan, pass_ns, iterate, s->count, &s->total))
      return rc;
    std::vector<int32_t> row(s->count, s->count + plan.num_passes);
    row.push_back(s->total);
    if (memo.size() > 256) memo.clear();
    hit = memo.emplace(iterate, std::move(row)).first;
  }
  for (int i = 0; i < plan.num_passes; ++i) s->count[i] = hit->second[i];
  s->total = hit->second[plan.num_passes];
  // A residual run keeps the multiset of passes and changes their order: the
  // pass that takes the residual goes last.  That is the deepest scheduled
  // pass whose kernel has a twin (the residual costs a launch the same work
  // whatever its depth); if none has one, the one-iteration pass,
  // behind which `<app>_residual` compares the outputs with that pass's
  // inputs -- taken out of a deeper pass's count where the schedule had none
  // (iterate - 1 iterations scheduled, one added).
  if (rq.residual)
    return residual_order(plan, pass_ns, iterate, s->count, &s->total,
                          &s->res_pass, &s->res_twin,
                          rq.residual->norms != nullptr);
  return SODA_HIP_OK;
}

// Scratch of a run of `s` on `cells` x `batch` cells, ahead of its first
// launch: the locals (into `base`) and the ping-pong temporaries.
static int ensure_scratch(soda_hip_program* p, const RunRequest& rq,
                          const Schedule& s, bool own_pingpong, int64_t cells,
                          soda_hip_kargs_t* base) {
  const soda_hip_plan_t& plan = p->plan;
  const int out0 = plan.num_inputs, loc0 = out0 + plan.num_outputs;
  // scratch for the local tensors -- only if a scheduled pass keeps them in
  // memory (marching kernels hold them in registers)
  const bool need_locals = locals_in_memory(plan, s.count);
  // Growing scratch allocates and synchronises (ensure): illegal on a stream
  // that is being captured.  Known here, before the first launch; the stream
  // is asked only when something must grow.
  if (scratch_grows(p, need_locals, s.total, own_pingpong, cells, rq.batch))
    if (int rc = refuse_growth_while_capturing(rq.stream, "run_device"))
      return rc;
  // (all of it for the whole batch: item i of a local or a temporary lies i
  // grids behind its start, like the caller's tensors; a larger batch regrows)
  for (int l = 0; need_locals && l < plan.num_locals; ++l) {
    int rc = ensure(p->locals[l],
                    (size_t)cells * rq.batch * plan.elem_size[loc0 + l]);
    if (rc) return rc;
    base->buf[loc0 + l] = p->locals[l].ptr;
  }
  if (s.total > 1)
    for (int o = 0; o < plan.num_outputs; ++o) {
      const size_t bytes = (size_t)cells * rq.batch * plan.elem_size[out0 + o];
      if (int rc = ensure(p->temps[o], bytes)) return rc;
      if (own_pingpong)
        if (int rc = ensure(p->temps2[o], bytes)) return rc;
    }
  return SODA_HIP_OK;
}

// The residual of a run, as its last pass takes it: as the pass's twin (both
// parts of a split pass -- one struct, one box, every chunk in exactly one
// part), or by `<app>_residual` / the norms kernels behind the pass.  `box`:
// in the coordinates of the rows that launch addresses.
struct ResidualTake {
  const ResidualRun* run;
  bool twin;
  soda_hip_resbox_t box;
};

// One pass of a run on `args`, by the tiles of `use`.  `take`: null for every
// pass but the last of a residual run.
static int launch_pass(soda_hip_program* p, const RunRequest& rq,
                       const PassLaunch& L, const soda_hip_kargs_t& args,
                       const ExtentPlan& use, const ResidualTake* take) {
  const soda_hip_plan_t& plan = p->plan;
  const auto& pass = plan.passes[L.pass];
  hipStream_t stream = static_cast<hipStream_t>(rq.stream);
  const SlabRun* slab = rq.slab;
  const bool twin = take && take->twin;
  void* const rdev = twin ? take->run->dev : nullptr;
  const soda_hip_resbox_t* box = take ? &take->box : nullptr;
  auto kernel_of = [&](int k) {
    const int kk = pass.kernel[k];
    return twin ? plan.kernels[kk].twin : kk;
  };
  if (L.split) {
    // (a split pass is one marching kernel: plan_launches)
    const int k0 = kernel_of(0);
    const int32_t hole = L.bnd_hi - L.bnd_lo;
    const TileRange boundary = {plan.dim - 1, L.bnd_lo, hole, L.chunks - hole};
    const TileRange interior = {plan.dim - 1, 0, L.bnd_lo, hole};
    auto part = [&](const TileRange& range, hipStream_t on) {
      return launch(p, k0, args, use.geo[k0].tile, on, &range, 1, rdev, box);
    };
    const bool in_order = split_in_order();
    if (in_order && !L.record) {
      // both parts on the caller's stream, the part that does not depend on
      // the exchange first: no hand-over between streams, but the two launches
      // do not share the GPU.  First pass: interior, wait, boundary
      if (int rc = part(interior, stream)) return rc;
      HIP_TRY(hipStreamWaitEvent(stream, slab->ghosts_ready, 0));
      if (int rc = part(boundary, stream)) return rc;
    } else if (in_order) {
      // last pass: (wait,) boundary, signal, interior
      if (L.wait) HIP_TRY(hipStreamWaitEvent(stream, slab->ghosts_ready, 0));
      if (int rc = part(boundary, stream)) return rc;
      HIP_TRY(hipEventRecord(slab->sendable, stream));
      if (int rc = part(interior, stream)) return rc;
    } else {
      // the boundary chunks on the program's side stream, the interior on the
      // caller's: the two share the GPU, the copies run underneath
      if (int rc = side_stream(p)) return rc;
      const int turn = p->ev_turn;
      p->ev_turn ^= 1;
      HIP_TRY(hipEventRecord(p->ev_pre[turn], stream));
      HIP_TRY(hipStreamWaitEvent(p->side, p->ev_pre[turn], 0));
      if (L.wait) HIP_TRY(hipStreamWaitEvent(p->side, slab->ghosts_ready, 0));
      if (int rc = part(boundary, p->side)) return rc;
      if (L.record) HIP_TRY(hipEventRecord(slab->sendable, p->side));
      HIP_TRY(hipEventRecord(p->ev_bnd[turn], p->side));
      if (int rc = part(interior, stream)) return rc;
      HIP_TRY(hipStreamWaitEvent(stream, p->ev_bnd[turn], 0));
    }
    ++p->last_split;
  } else {
    if (L.wait) HIP_TRY(hipStreamWaitEvent(stream, slab->ghosts_ready, 0));
    for (int k = 0; k < pass.num_kernels; ++k) {
      const int kk = kernel_of(k);
      if (int rc = launch(p, kk, args, use.geo[kk].tile, stream, nullptr,
                          rq.batch, rdev, box))
        return rc;
    }
  }
  p->last_launches += L.split ? 2 : pass.num_kernels;
  if (L.pass == 0) p->last_fused += pass.num_kernels;
  if (take && !take->twin) {
    // cur: what the pass just wrote; prev: what it read.  Behind both parts
    // of a split pass: it reads all of what the pass wrote and writes the
    // struct only, so `sendable` need not wait for it
    if (int rc = launch_generic(p, args, stream, *take->run, take->box))
      return rc;
    ++p->last_launches;
  }
  if (!L.split && L.record) HIP_TRY(hipEventRecord(slab->sendable, stream));
  return SODA_HIP_OK;
}

// zeroed inside the call, on the caller's stream, by a kernel of the program:
// a captured call zeroes and refills the struct at every replay (as a 32-byte
// memset node the zeroing did not survive a replay)
int residual_zero(soda_hip_program* p, const ResidualRun& res, void* stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (res.norms) return norms_zero(res.norms, res.dev, stream);
  const int zk = p->plan.residual.zero_kernel;
  void* dev = res.dev;
  size_t size = sizeof dev;
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &dev,
                   HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  HIP_TRY(hipModuleLaunchKernel(p->functions[zk], 1, 1, 1, 64, 1, 1, 0, stream,
                                nullptr, extra));
  return SODA_HIP_OK;
}

int residual_add(soda_hip_program* p, void* const* cur,
                 const void* const* prev, const int32_t* extent,
                 const ResidualRun& res, const soda_hip_resbox_t& box,
                 void* stream) {
  const soda_hip_plan_t& plan = p->plan;
  bool any = false;
  for (int o = 0; o < plan.num_outputs; ++o) {
    bool empty = false;
    for (int d = 0; d < plan.dim; ++d) {
      if (box.lo[o][d] < 0 || box.hi[o][d] > extent[d])
        return fail(SODA_HIP_ERR_INVALID,
                    "residual: the box does not lie in the arrays; nothing "
                    "was launched");
      if (box.hi[o][d] <= box.lo[o][d]) empty = true;
    }
    if (!empty) any = true;
  }
  if (!any) return SODA_HIP_OK;
  // (prev holds no param arrays: the residual kernels read none)
  std::vector<const void*> in(plan.num_inputs + plan.num_params, prev[0]);
  for (int i = 0; i < plan.num_inputs; ++i) in[i] = prev[i];
  soda_hip_kargs_t args;
  int64_t cells;
  if (int rc = run_geometry(plan, {cur, in.data(), extent, 1, stream}, &args,
                            &cells))
    return rc;
  for (int i = 0; i < plan.num_inputs; ++i)
    args.buf[i] = const_cast<void*>(prev[i]);
  for (int o = 0; o < plan.num_outputs; ++o)
    args.buf[plan.num_inputs + o] = cur[o];
  return launch_generic(p, args, static_cast<hipStream_t>(stream), res, box);
}

int run_core(soda_hip_program_t* p, const RunRequest& rq) {
  if (!p || !rq.outputs || !rq.inputs || !rq.extent)
    return fail(SODA_HIP_ERR_INVALID, "run_device: NULL argument");
  const soda_hip_plan_t& plan = p->plan;
  const ResidualRun* res = rq.residual;
  const int32_t iterate = rq.iterate, batch = rq.batch;
  if (res && (batch != 1 || rq.force_pass >= 0 || !plan.residual.present ||
              !res->dev || (res->box ? rq.slab != nullptr
                                     : res->box_iterate < iterate)))
    return fail(SODA_HIP_ERR_INVALID, "run_core: bad residual run");
  if (batch < 1 || (batch > 1 && (!plan.batched || rq.slab)))
    return fail(SODA_HIP_ERR_INVALID, "run_core: bad batch");
  if (iterate < 1) return fail(SODA_HIP_ERR_INVALID, "cannot iterate < 1 times");
  if (iterate > 1 && plan.num_inputs != plan.num_outputs)
    return fail(SODA_HIP_ERR_INVALID,
                "number of input tensors must be the same as output if "
                "iterate > 1 times");
  hipStream_t stream = static_cast<hipStream_t>(rq.stream);
  HIP_TRY(hipSetDevice(p->device));
  const Cone* cone = rq.slab ? &rq.slab->cone : nullptr;

  soda_hip_kargs_t base;
  int64_t cells;
  if (int rc = run_geometry(plan, rq, &base, &cells)) return rc;
  if (int rc = check_run_tensors(plan, p->bank_tensors, rq.outputs, rq.inputs,
                                 cells, batch))
    return rc;
  Schedule s;
  if (int rc = choose_schedule(p, rq, base.extent, &s)) return rc;
  const int32_t total = s.total;

  if (p->debug) base.buf[SODA_HIP_MAX_TENSORS - 1] = p->debug;
  // the banked form of a wire stream's program: the stream's length, beyond
  // which a delayed input reads as zero (0 for every other program).  Such a
  // program's plan is not truthful in two fields, which is why it only ever
  // comes here with iterate = 1 and no slab: its one pass says fused_iters = 1
  // for a kernel that runs all of the stream's iterations, and num_locals = 0
  // (the marching kernel holds them in registers; its a.buf[] slots end with
  // the output banks) -- stream.py `banked_spec`
  base.reserved[0] = p->stream_elems;
  const int in0 = 0, out0 = plan.num_inputs;
  const int prm0 = out0 + plan.num_outputs + plan.num_locals;
  for (int k = 0; k < plan.num_params; ++k)   // the same in every iteration
    base.buf[prm0 + k] = const_cast<void*>(rq.inputs[plan.num_inputs + k]);
  // A run that trims its passes to a cone promises to leave the rows of the
  // caller's outputs beyond the LAST pass's reach as they were (soda_hip.h,
  // soda_hip_run_device_cone).  The earlier passes cover more rows than the
  // last one, so with three passes or more they may not ping-pong through
  // the caller's outputs: they alternate between two temporaries instead.
  const bool own_pingpong =
      cone && total > 2 &&
      (cone->keep_lo > 0 || cone->keep_hi < base.extent[plan.dim - 1]);
  if (int rc = ensure_scratch(p, rq, s, own_pingpong, cells, &base)) return rc;

  std::map<ExtentKey, ExtentPlan>& extents = extents_of(p, batch);
  std::vector<PassLaunch> launches;
  if (int rc = plan_launches(plan, &extents, base.extent, s.count, total,
                             iterate, rq.slab, &launches, s.res_pass,
                             s.res_twin))
    return rc;
  soda_hip_resbox_t res_box;
  if (res) {
    // (the pass that takes the residual is the last of `launches`, and the
    // cone of every pass before it is that of this order: plan_launches.)
    // The cells counted: the global grid's box, of which a slab takes its
    // kept rows -- the ghost rows of the result, which the last pass writes
    // too, lie outside and are not counted.
    // A domain hands its own box in (ResidualRun): its interior.
    if (res->box)
      res_box = *res->box;
    else
      residual_slab_box(plan, base.gextent, base.origin, base.extent,
                        cone ? cone->keep_lo : 0,
                        cone ? cone->keep_hi : base.extent[plan.dim - 1],
                        res->box_iterate, &res_box);
    if (!res->accumulate)
      if (int rc = residual_zero(p, *res, rq.stream)) return rc;
    p->last_res_mode = s.res_twin ? 1 : 2;
    p->last_res_fused = plan.passes[s.res_pass].fused_iters;
  }
  p->last_launches = 0;
  p->last_fused = 0;
  p->last_split = 0;
  p->last_rows = 0;
  std::vector<const void*> src(rq.inputs, rq.inputs + plan.num_inputs);
  const int ax = plan.dim - 1;
  const int32_t rows = base.extent[ax];
  for (size_t done = 0; done < launches.size(); ++done) {
    const PassLaunch& L = launches[done];
    // the last pass writes the caller's outputs; before that alternate
    // between the program's temporaries and the caller's outputs
    const bool to_out = ((total - 1 - (int)done) % 2) == 0;
    const bool last_pass = (int)done + 1 == total;
    for (int j = 0; j < plan.num_inputs; ++j)
      base.buf[in0 + j] = const_cast<void*>(src[j]);
    for (int o = 0; o < plan.num_outputs; ++o)
      base.buf[out0 + o] = !own_pingpong ? (to_out ? rq.outputs[o]
                                                   : p->temps[o].ptr)
                           : last_pass   ? rq.outputs[o]
                           : to_out      ? p->temps2[o].ptr
                                         : p->temps[o].ptr;
    soda_hip_kargs_t args = base;
    if (L.lo > 0 || L.hi < rows) {
      args.extent[ax] = L.hi - L.lo;
      args.origin[ax] = base.origin[ax] + L.lo;
      for (int t = 0; t < plan.num_inputs + plan.num_outputs; ++t)
        args.buf[t] = static_cast<char*>(base.buf[t]) +
                      (int64_t)L.lo * base.stride[ax] * plan.elem_size[t];
    }
    ExtentPlan* use = nullptr;
    if (int rc = extent_plan(plan, &extents, args.extent, &use, batch))
      return rc;
    p->last_rows += L.hi - L.lo;
    ResidualTake take;
    if (res && last_pass)
      take = {res, s.res_twin,
              shifted_box(plan, res_box, L.lo, L.hi - L.lo)};
    if (int rc = launch_pass(p, rq, L, args, *use,
                             res && last_pass ? &take : nullptr))
      return rc;
    if (!last_pass)
      for (int j = 0; j < plan.num_inputs; ++j) src[j] = base.buf[out0 + j];
  }
  return SODA_HIP_OK;
}

// Runs `check_every` iterations at a time until `converged(&stop)` says so by
// the struct of the last chunk -- `host_bytes` fetched into `host`; `norms`
// null: the residual struct -- or `max_iterate` iterations are done.  The
// chunks ping-pong between the caller's outputs and p->until_tmp: the first
// reads the caller's inputs, every later one the result before it.
// Synchronous.
template <class Converged>
static int run_until(soda_hip_program* p, const char* who,
                     void* const* outputs, const void* const* inputs,
                     const int32_t* extent, int32_t max_iterate,
                     int32_t check_every, soda_hip_norms_handle* norms,
                     void* host, size_t host_bytes, Converged converged,
                     int32_t* iterations_done, void* stream_) {
  const soda_hip_plan_t& plan = p->plan;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipSetDevice(p->device));
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capture) != hipSuccess) {
    (void)hipGetLastError();
    capture = hipStreamCaptureStatusNone;
  }
  if (capture != hipStreamCaptureStatusNone)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) +
                    ": synchronous, not for a stream that is being captured; "
                    "nothing was launched");
  int64_t cells = 1;
  for (int d = 0; d < plan.dim; ++d) {
    if (extent[d] < 1)
      return fail(SODA_HIP_ERR_INVALID, std::string(who) + ": extent < 1");
    cells *= extent[d];
  }
  if (int rc = ensure(p->until_struct, host_bytes)) return rc;
  const int out0 = plan.num_inputs;
  std::vector<const void*> in(inputs,
                              inputs + plan.num_inputs + plan.num_params);
  std::vector<void*> tmp(plan.num_outputs, nullptr);
  std::vector<void*> own(outputs, outputs + plan.num_outputs);
  memset(host, 0, host_bytes);
  int32_t done = 0;
  bool in_tmp = false;
  for (int32_t chunk = 0; done < max_iterate; ++chunk) {
    const int32_t n =
        max_iterate - done < check_every ? max_iterate - done : check_every;
    in_tmp = chunk % 2 == 1;
    if (in_tmp && !tmp[0])
      for (int o = 0; o < plan.num_outputs; ++o) {
        if (int rc = ensure(p->until_tmp[o],
                            (size_t)cells * plan.elem_size[out0 + o]))
          return rc;
        tmp[o] = p->until_tmp[o].ptr;
      }
    void* const* dst = in_tmp ? tmp.data() : own.data();
    const ResidualRun run = {p->until_struct.ptr, done + n, norms};
    RunRequest rq = {dst, in.data(), extent, n, stream_};
    rq.residual = &run;
    if (int rc = run_core(p, rq)) return rc;
    HIP_TRY(hipMemcpyAsync(host, p->until_struct.ptr, host_bytes,
                           hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    done += n;
    // the next chunk continues from this one's result; the caller's inputs
    // were read by the first chunk only
    for (int j = 0; j < plan.num_inputs; ++j) in[j] = dst[j];
    bool stop = false;
    if (int rc = converged(&stop)) return rc;
    if (stop) break;
  }
  if (in_tmp) {
    for (int o = 0; o < plan.num_outputs; ++o)
      HIP_TRY(hipMemcpyAsync(outputs[o], tmp[o],
                             (size_t)cells * plan.elem_size[out0 + o],
                             hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  if (iterations_done) *iterations_done = done;
  return SODA_HIP_OK;
}

}  // namespace soda_detail

// a call that may be refused before run_core reads as zero launches
static void reset_last_run(soda_hip_program* p) {
  p->last_res_mode = 0;
  p->last_res_fused = 0;
  p->last_launches = 0;
  p->last_fused = 0;
}

// a box per output as the C entries hand it out: lo[o * dim + d], hi likewise
static void flatten_box(const soda_hip_plan_t& plan,
                        const soda_hip_resbox_t& box, int32_t* lo,
                        int32_t* hi) {
  for (int o = 0; o < plan.num_outputs; ++o)
    for (int d = 0; d < plan.dim; ++d) {
      lo[o * plan.dim + d] = box.lo[o][d];
      hi[o * plan.dim + d] = box.hi[o][d];
    }
}

static int check_struct_aligned(const void* dev, const char* what,
                                const char* who) {
  if (reinterpret_cast<uintptr_t>(dev) % 8)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": the " + what +
                    " struct is not 8-byte aligned; nothing was launched");
  return SODA_HIP_OK;
}

// The struct of `bytes` a run fills (`what`: "residual" / "norms"): 8-byte
// aligned, and no byte of it in an output of `extent`.
static int check_run_struct(const soda_hip_plan_t& plan, void* const* outputs,
                            const int32_t* extent, const void* dev,
                            size_t bytes, const char* what, const char* who) {
  if (int rc = check_struct_aligned(dev, what, who)) return rc;
  uint64_t cells = 1;
  for (int d = 0; d < plan.dim; ++d)
    cells *= (uint64_t)(extent[d] > 0 ? extent[d] : 0);
  const uintptr_t r0 = reinterpret_cast<uintptr_t>(dev);
  for (int o = 0; o < plan.num_outputs; ++o) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(outputs[o]);
    if (outputs[o] && r0 < o0 + cells * plan.elem_size[plan.num_inputs + o] &&
        o0 < r0 + bytes)
      return fail(SODA_HIP_ERR_INVALID,
                  std::string(who) + ": the " + what +
                      " struct overlaps an output; nothing was launched");
  }
  return SODA_HIP_OK;
}

extern "C" {

int soda_hip_run_device(soda_hip_program_t* p, void* const* outputs,
                        const void* const* inputs, const int32_t* extent,
                        int32_t iterate, void* stream_) {
  return run_core(p, {outputs, inputs, extent, iterate, stream_});
}

int soda_hip_plan_residual_box(const soda_hip_plan_t* plan,
                               const int32_t* extent, int32_t iterate,
                               int32_t* lo, int32_t* hi) {
  if (!plan || !extent || !lo || !hi)
    return fail(SODA_HIP_ERR_INVALID, "plan_residual_box: NULL argument");
  if (int rc = check_plan(plan)) return rc;
  if (!plan->residual.present)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                "plan_residual_box: the plan has no residual");
  if (iterate < 1)
    return fail(SODA_HIP_ERR_INVALID, "plan_residual_box: iterate < 1");
  for (int d = 0; d < plan->dim; ++d)
    if (extent[d] < 1)
      return fail(SODA_HIP_ERR_INVALID, "plan_residual_box: extent < 1");
  soda_hip_resbox_t box;
  residual_box(*plan, extent, iterate, &box);
  flatten_box(*plan, box, lo, hi);
  return SODA_HIP_OK;
}

// what the residual entries ask of a program and of the 32 bytes
// (residual_dev null: of the program only)
static int check_residual(const soda_hip_program* p, void* const* outputs,
                          const int32_t* extent, const void* residual_dev,
                          const char* who) {
  if (!p->plan.residual.present)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                std::string(who) +
                    ": the program has no residual kernels (build it with "
                    "LowerOptions.residual / sodac --hip-residual); nothing "
                    "was launched");
  if (!residual_dev) return SODA_HIP_OK;
  return check_run_struct(p->plan, outputs, extent, residual_dev,
                          sizeof(soda_hip_residual_t), "residual", who);
}

int soda_hip_run_device_residual(soda_hip_program_t* p, void* const* outputs,
                                 const void* const* inputs,
                                 const int32_t* extent, int32_t iterate,
                                 void* residual_dev, void* stream_) {
  if (!p || !outputs || !inputs || !extent || !residual_dev)
    return fail(SODA_HIP_ERR_INVALID, "run_device_residual: NULL argument");
  reset_last_run(p);
  if (int rc = check_residual(p, outputs, extent, residual_dev,
                              "run_device_residual"))
    return rc;
  const ResidualRun run = {residual_dev, iterate};
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.residual = &run;
  return run_core(p, rq);
}

int soda_hip_run_device_until(soda_hip_program_t* p, void* const* outputs,
                              const void* const* inputs, const int32_t* extent,
                              int32_t max_iterate, int32_t check_every,
                              double tol, uint64_t int_tol,
                              soda_hip_residual_t* result_host,
                              int32_t* iterations_done, void* stream_) {
  if (!p || !outputs || !inputs || !extent)
    return fail(SODA_HIP_ERR_INVALID, "run_device_until: NULL argument");
  if (max_iterate < 1 || check_every < 1)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_until: max_iterate and check_every must be >= 1");
  if (int rc = check_residual(p, outputs, extent, nullptr, "run_device_until"))
    return rc;
  soda_hip_residual_t host;
  auto converged = [&](bool* stop) {
    *stop = residual_converged(host, tol, int_tol);
    return SODA_HIP_OK;
  };
  if (int rc = run_until(p, "run_device_until", outputs, inputs, extent,
                         max_iterate, check_every, nullptr, &host, sizeof host,
                         converged, iterations_done, stream_))
    return rc;
  if (result_host) *result_host = host;
  return SODA_HIP_OK;
}

int soda_hip_last_residual(soda_hip_program_t* p, int32_t* mode,
                           int32_t* fused_iters) {
  if (!p || !mode) return fail(SODA_HIP_ERR_INVALID, "last_residual: NULL");
  *mode = p->last_res_mode;
  if (fused_iters) *fused_iters = p->last_res_fused;
  return SODA_HIP_OK;
}

// ---- exact norms: the handle and its entries ---------------------------------
int soda_hip_norms_create(const void* code, size_t code_size, int32_t cell,
                          int32_t dim, int32_t device,
                          soda_hip_norms_handle_t** handle) {
  static const char* const kCType[10] = {
      "float", "double", "int8_t", "uint8_t", "int16_t", "uint16_t",
      "int32_t", "uint32_t", "int64_t", "uint64_t"};
  if (!code || !code_size || !handle)
    return fail(SODA_HIP_ERR_INVALID, "norms_create: NULL argument");
  *handle = nullptr;
  int32_t elem = 0;
  const int kind = soda_hip_norms_kind_of(cell, &elem);
  if (!kind || dim < 1 || dim > SODA_HIP_MAX_DIM)
    return fail(SODA_HIP_ERR_INVALID, "norms_create: bad cell type or dim");
  int n = 0;
  if (int rc = soda_hip_device_count(&n)) return rc;
  if (n < 1) return fail(SODA_HIP_ERR_NODEVICE, "no GPU visible");
  if (device < 0 || device >= n)
    return fail(SODA_HIP_ERR_INVALID, "norms_create: no such device");
  HIP_TRY(hipSetDevice(device));
  soda_hip_norms_handle* h = new (std::nothrow) soda_hip_norms_handle;
  if (!h) return fail(SODA_HIP_ERR_NOMEM, "new norms handle");
  h->device = device;
  h->cell = cell;
  h->kind = kind;
  h->elem = elem;
  h->dim = dim;
  hipError_t e = hipModuleLoadData(&h->module, code);
  if (e != hipSuccess) {
    delete h;
    return hip_fail(e, "hipModuleLoadData");
  }
  e = hipModuleGetFunction(&h->zero, h->module, "soda_norms_zero");
  for (int32_t v = 16 / elem; e == hipSuccess && v >= 1; v /= 2) {
    const std::string name = std::string("soda_norms_") + kCType[cell] + "_v" +
                             std::to_string(v);
    hipFunction_t fn = nullptr;
    e = hipModuleGetFunction(&fn, h->module, name.c_str());
    h->widths.emplace_back(v, fn);
  }
  if (e != hipSuccess) {
    (void)hipModuleUnload(h->module);
    delete h;
    return hip_fail(e, "norms_create: hipModuleGetFunction (is this the norms "
                       "module of that cell type?)");
  }
  *handle = h;
  return SODA_HIP_OK;
}

int soda_hip_norms_destroy(soda_hip_norms_handle_t* h) {
  if (!h) return SODA_HIP_OK;
  (void)hipSetDevice(h->device);
  if (h->module) (void)hipModuleUnload(h->module);
  delete h;
  return SODA_HIP_OK;
}

int soda_hip_norms_zero(soda_hip_norms_handle_t* h, void* acc_dev,
                        void* stream) {
  if (!h || !acc_dev)
    return fail(SODA_HIP_ERR_INVALID, "norms_zero: NULL argument");
  if (int rc = check_struct_aligned(acc_dev, "norms", "norms_zero"))
    return rc;
  HIP_TRY(hipSetDevice(h->device));
  return norms_zero(h, acc_dev, static_cast<hipStream_t>(stream));
}

int soda_hip_norms_accumulate(soda_hip_norms_handle_t* h, const void* cur,
                              const void* prev, const int32_t* extent,
                              const int32_t* lo, const int32_t* hi,
                              void* acc_dev, void* stream) {
  if (!h || !cur || !prev || !extent || !lo || !hi || !acc_dev)
    return fail(SODA_HIP_ERR_INVALID, "norms_accumulate: NULL argument");
  if (int rc = check_struct_aligned(acc_dev, "norms", "norms_accumulate"))
    return rc;
  HIP_TRY(hipSetDevice(h->device));
  return norms_accumulate(h, cur, prev, extent, lo, hi, acc_dev,
                          static_cast<hipStream_t>(stream));
}

// what both norms runs ask of a program, a handle and the struct
// (acc_dev null: of the program and the handle only)
static int check_norms_run(const soda_hip_program* p,
                           const soda_hip_norms_handle* h,
                           void* const* outputs, const int32_t* extent,
                           const void* acc_dev, const char* who) {
  if (int rc = check_residual(p, outputs, extent, nullptr, who)) return rc;
  const soda_hip_plan_t& plan = p->plan;
  if (h->dim != plan.dim || h->device != p->device)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": the norms handle is of another dimension "
                                   "count or device; nothing was launched");
  for (int o = 0; o < plan.num_outputs; ++o)
    if (plan.elem_size[o] != h->elem ||
        plan.elem_size[plan.num_inputs + o] != h->elem)
      return fail(SODA_HIP_ERR_UNSUPPORTED,
                  std::string(who) + ": a pair's cells are not of the handle's "
                                     "type (one struct holds one kind of "
                                     "units); nothing was launched");
  if (!acc_dev) return SODA_HIP_OK;
  return check_run_struct(plan, outputs, extent, acc_dev,
                          sizeof(soda_hip_norms_t), "norms", who);
}

int soda_hip_run_device_norms(soda_hip_program_t* p,
                              soda_hip_norms_handle_t* h, void* const* outputs,
                              const void* const* inputs, const int32_t* extent,
                              int32_t iterate, void* acc_dev, void* stream_) {
  if (!p || !h || !outputs || !inputs || !extent || !acc_dev)
    return fail(SODA_HIP_ERR_INVALID, "run_device_norms: NULL argument");
  reset_last_run(p);
  if (int rc = check_norms_run(p, h, outputs, extent, acc_dev,
                               "run_device_norms"))
    return rc;
  const ResidualRun run = {acc_dev, iterate, h};
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.residual = &run;
  return run_core(p, rq);
}

int soda_hip_run_device_until_norm(soda_hip_program_t* p,
                                   soda_hip_norms_handle_t* h,
                                   void* const* outputs,
                                   const void* const* inputs,
                                   const int32_t* extent, int32_t max_iterate,
                                   int32_t check_every, int32_t which,
                                   double tol, soda_hip_norms_t* result_host,
                                   int32_t* iterations_done, void* stream_) {
  if (!p || !h || !outputs || !inputs || !extent)
    return fail(SODA_HIP_ERR_INVALID, "run_device_until_norm: NULL argument");
  if (max_iterate < 1 || check_every < 1)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_until_norm: max_iterate and check_every must be "
                ">= 1");
  if (which != SODA_HIP_NORMS_WHICH_L1 && which != SODA_HIP_NORMS_WHICH_L2)
    return fail(SODA_HIP_ERR_INVALID, "run_device_until_norm: bad `which`");
  if (int rc = check_norms_run(p, h, outputs, extent, nullptr,
                               "run_device_until_norm"))
    return rc;
  soda_hip_norms_t host;
  auto converged = [&](bool* stop) {
    if (!norms_converged(host, which, tol, stop))
      return fail(SODA_HIP_ERR_RUNTIME,
                  "run_device_until_norm: the struct fetched is of no kind");
    return (int)SODA_HIP_OK;
  };
  if (int rc = run_until(p, "run_device_until_norm", outputs, inputs, extent,
                         max_iterate, check_every, h, &host, sizeof host,
                         converged, iterations_done, stream_))
    return rc;
  if (result_host) *result_host = host;
  return SODA_HIP_OK;
}

int soda_hip_run_device_batch(soda_hip_program_t* p, void* const* outputs,
                              const void* const* inputs, const int32_t* extent,
                              int32_t batch, int32_t iterate, void* stream_) {
  if (!p || !outputs || !inputs || !extent)
    return fail(SODA_HIP_ERR_INVALID, "run_device_batch: NULL argument");
  if (int rc = check_batch(batch, "run_device_batch")) return rc;
  if (!p->plan.batched)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_batch: the program's kernels are not batched "
                "(build it with LowerOptions.batch / sodac --hip-batch); "
                "nothing was launched");
  // (no tensor may overlap another, each `batch` items long: run_core checks)
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.batch = batch;
  return run_core(p, rq);
}

int soda_hip_run_device_window(soda_hip_program_t* p, void* const* outputs,
                               const void* const* inputs,
                               const int32_t* extent, const int32_t* origin,
                               const int32_t* global_extent, int32_t iterate,
                               void* stream_) {
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.origin = origin;
  rq.global_extent = global_extent;
  return run_core(p, rq);
}

static int slab_run(const soda_hip_slab_run_t* run, const int32_t* extent,
                    int ax, SlabRun* out) {
  if (run->keep_lo < 0 || run->keep_hi > extent[ax] ||
      run->keep_lo >= run->keep_hi || run->reach_lo < 0 || run->reach_hi < 0)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_slab: [keep_lo, keep_hi) must be a non-empty range "
                "of the last dimension, the reaches non-negative");
  if (run->ghost_lo < 0 || run->ghost_hi < 0 || run->send_lo < 0 ||
      run->send_hi < 0 || run->ghost_lo + run->ghost_hi > extent[ax] ||
      run->send_lo > run->keep_hi - run->keep_lo ||
      run->send_hi > run->keep_hi - run->keep_lo)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_slab: ghost / send rows out of range");
  SlabRun& s = *out;
  s.cone = {run->keep_lo, run->keep_hi, run->reach_lo, run->reach_hi};
  s.ghost_lo = run->ghost_lo;
  s.ghost_hi = run->ghost_hi;
  s.send_lo = run->send_lo;
  s.send_hi = run->send_hi;
  s.ghosts_ready = static_cast<hipEvent_t>(run->ghosts_ready);
  s.sendable = static_cast<hipEvent_t>(run->sendable);
  return SODA_HIP_OK;
}

int soda_hip_run_device_cone(soda_hip_program_t* p, void* const* outputs,
                             const void* const* inputs, const int32_t* extent,
                             const int32_t* origin,
                             const int32_t* global_extent, int32_t iterate,
                             int32_t keep_lo, int32_t keep_hi,
                             int32_t reach_lo, int32_t reach_hi,
                             void* stream_) {
  soda_hip_slab_run_t run;
  memset(&run, 0, sizeof run);
  run.keep_lo = keep_lo;
  run.keep_hi = keep_hi;
  run.reach_lo = reach_lo;
  run.reach_hi = reach_hi;
  return soda_hip_run_device_slab(p, outputs, inputs, extent, origin,
                                  global_extent, iterate, &run, stream_);
}

int soda_hip_run_device_slab(soda_hip_program_t* p, void* const* outputs,
                             const void* const* inputs, const int32_t* extent,
                             const int32_t* origin,
                             const int32_t* global_extent, int32_t iterate,
                             const soda_hip_slab_run_t* run, void* stream_) {
  if (!p || !extent || !run)
    return fail(SODA_HIP_ERR_INVALID, "run_device_slab: NULL argument");
  SlabRun s;
  if (int rc = slab_run(run, extent, p->plan.dim - 1, &s)) return rc;
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.origin = origin;
  rq.global_extent = global_extent;
  rq.slab = &s;
  return run_core(p, rq);
}

int soda_hip_run_device_slab_residual(
    soda_hip_program_t* p, void* const* outputs, const void* const* inputs,
    const int32_t* extent, const int32_t* origin, const int32_t* global_extent,
    int32_t iterate, int32_t box_iterate, const soda_hip_slab_run_t* run,
    void* residual_dev, void* stream_) {
  if (!p || !outputs || !inputs || !extent || !run || !residual_dev)
    return fail(SODA_HIP_ERR_INVALID, "run_device_slab_residual: NULL argument");
  reset_last_run(p);
  if (int rc = check_residual(p, outputs, extent, residual_dev,
                              "run_device_slab_residual"))
    return rc;
  if (box_iterate < iterate)
    return fail(SODA_HIP_ERR_INVALID,
                "run_device_slab_residual: box_iterate counts the iterations "
                "the state has seen, this call's included: it cannot be less "
                "than iterate; nothing was launched");
  SlabRun s;
  if (int rc = slab_run(run, extent, p->plan.dim - 1, &s)) return rc;
  const ResidualRun res = {residual_dev, box_iterate};
  RunRequest rq = {outputs, inputs, extent, iterate, stream_};
  rq.origin = origin;
  rq.global_extent = global_extent;
  rq.slab = &s;
  rq.residual = &res;
  return run_core(p, rq);
}

int soda_hip_plan_residual_slab_box(const soda_hip_plan_t* plan,
                                    const int32_t* global_extent,
                                    const int32_t* origin,
                                    const int32_t* extent, int32_t keep_lo,
                                    int32_t keep_hi, int32_t iterate,
                                    int32_t* lo, int32_t* hi) {
  if (!plan || !global_extent || !origin || !extent || !lo || !hi)
    return fail(SODA_HIP_ERR_INVALID, "plan_residual_slab_box: NULL argument");
  if (int rc = check_plan(plan)) return rc;
  if (!plan->residual.present)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                "plan_residual_slab_box: the plan has no residual");
  if (iterate < 1)
    return fail(SODA_HIP_ERR_INVALID, "plan_residual_slab_box: iterate < 1");
  for (int d = 0; d < plan->dim; ++d)
    if (extent[d] < 1 || origin[d] < 0 ||
        (int64_t)origin[d] + extent[d] > global_extent[d])
      return fail(SODA_HIP_ERR_INVALID,
                  "plan_residual_slab_box: the slab does not lie in the "
                  "global grid");
  if (keep_lo < 0 || keep_hi > extent[plan->dim - 1] || keep_lo > keep_hi)
    return fail(SODA_HIP_ERR_INVALID,
                "plan_residual_slab_box: [keep_lo, keep_hi) must be a range of "
                "the slab's last dimension");
  soda_hip_resbox_t box;
  residual_slab_box(*plan, global_extent, origin, extent, keep_lo, keep_hi,
                    iterate, &box);
  flatten_box(*plan, box, lo, hi);
  return SODA_HIP_OK;
}

// residual_mode != NULL: the launches of a run that takes a residual
static int plan_launches_c(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, const soda_hip_slab_run_t* run,
                           int32_t capacity, soda_hip_launch_info_t* launches,
                           int32_t* count, int32_t* residual_mode) {
  if (!plan || !extent || !count || capacity < 0 || (capacity && !launches))
    return fail(SODA_HIP_ERR_INVALID, "plan_launches: bad argument");
  if (iterate < 1) return fail(SODA_HIP_ERR_INVALID, "cannot iterate < 1 times");
  if (int rc = check_plan(plan)) return rc;
  int32_t ext[SODA_HIP_MAX_DIM];
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    ext[d] = d < plan->dim ? extent[d] : 1;
    if (ext[d] < 1) return fail(SODA_HIP_ERR_INVALID, "plan_launches: extent < 1");
  }
  SlabRun s;
  if (run)
    if (int rc = slab_run(run, ext, plan->dim - 1, &s)) return rc;
  std::map<ExtentKey, ExtentPlan> cache;
  ExtentPlan* ep = nullptr;
  if (int rc = extent_plan(*plan, &cache, ext, &ep)) return rc;
  int32_t per_pass[SODA_HIP_MAX_PASSES], total = 0;
  if (int rc = schedule(*plan, ep->model_ns, iterate, per_pass, &total)) return rc;
  int res_pass = -1;
  bool res_twin = false;
  if (residual_mode) {
    if (int rc = residual_order(*plan, ep->model_ns, iterate, per_pass, &total,
                                &res_pass, &res_twin))
      return rc;
    *residual_mode = res_twin ? 1 : 2;
  }
  std::vector<PassLaunch> list;
  if (int rc = plan_launches(*plan, &cache, ext, per_pass, total, iterate,
                             run ? &s : nullptr, &list, res_pass, res_twin))
    return rc;
  *count = (int32_t)list.size();
  for (int32_t i = 0; i < *count && i < capacity; ++i) {
    const PassLaunch& L = list[i];
    launches[i] = {plan->passes[L.pass].fused_iters, L.lo, L.hi, L.wait,
                   L.record, L.split, L.chunk, L.chunks, L.bnd_lo, L.bnd_hi};
  }
  return SODA_HIP_OK;
}

int soda_hip_plan_launches(const soda_hip_plan_t* plan, const int32_t* extent,
                           int32_t iterate, const soda_hip_slab_run_t* run,
                           int32_t capacity, soda_hip_launch_info_t* launches,
                           int32_t* count) {
  return plan_launches_c(plan, extent, iterate, run, capacity, launches, count,
                         nullptr);
}

int soda_hip_plan_launches_residual(const soda_hip_plan_t* plan,
                                    const int32_t* extent, int32_t iterate,
                                    const soda_hip_slab_run_t* run,
                                    int32_t capacity,
                                    soda_hip_launch_info_t* launches,
                                    int32_t* count, int32_t* mode) {
  if (!mode) return fail(SODA_HIP_ERR_INVALID, "plan_launches: bad argument");
  if (plan && !plan->residual.present)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                "plan_launches_residual: the plan has no residual");
  return plan_launches_c(plan, extent, iterate, run, capacity, launches, count,
                         mode);
}

int soda_hip_program_calibrate(soda_hip_program_t* p, const int32_t* extent,
                               int32_t launches, void* stream_) {
  return soda_hip_program_calibrate_batch(p, extent, 1, launches, stream_);
}

// a program handle's batch argument: in range, and > 1 only for batched plans
static int check_program_batch(const soda_hip_program* p, int32_t batch,
                               const char* who) {
  if (int rc = check_batch(batch, who)) return rc;
  if (batch > 1 && !p->plan.batched)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": the program's kernels are not batched");
  return SODA_HIP_OK;
}

int soda_hip_program_calibrate_batch(soda_hip_program_t* p,
                                     const int32_t* extent, int32_t batch,
                                     int32_t launches, void* stream_) {
  if (!p || !extent) return fail(SODA_HIP_ERR_INVALID, "calibrate: NULL argument");
  if (int rc = check_program_batch(p, batch, "calibrate")) return rc;
  const soda_hip_plan_t& plan = p->plan;
  std::map<ExtentKey, ExtentPlan>& extents = extents_of(p, batch);
  std::map<ExtentKey, std::vector<double>>& measured = measured_of(p, batch);
  if (launches < 2) launches = 4;
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipSetDevice(p->device));
  std::array<int32_t, SODA_HIP_MAX_DIM> key;
  int64_t cells = 1;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    key[d] = d < plan.dim ? extent[d] : 1;
    if (key[d] < 1) return fail(SODA_HIP_ERR_INVALID, "calibrate: extent < 1");
    cells *= key[d];
  }
  if (plan.num_passes < 2 || plan.num_inputs != plan.num_outputs) {
    measured.erase(key);          // nothing to choose between
    auto it = extents.find(key);
    if (it != extents.end()) it->second.sched.clear();
    return SODA_HIP_OK;
  }
  // stand-in arrays: inputs (a byte pattern that reads as ~0.75 in fp32, small
  // positive integers otherwise), outputs, params
  std::vector<DeviceBuffer> bufs(plan.num_inputs + plan.num_outputs +
                                 plan.num_params);
  std::vector<const void*> ins;
  std::vector<void*> outs;
  int rc = SODA_HIP_OK;
  const int prm0 = plan.num_inputs + plan.num_outputs + plan.num_locals;
  for (size_t b = 0; b < bufs.size() && rc == SODA_HIP_OK; ++b) {
    size_t bytes;
    if ((int)b < plan.num_inputs + plan.num_outputs)
      bytes = (size_t)cells * batch * plan.elem_size[b];
    else
      bytes = (size_t)plan.param_elems[b - plan.num_inputs - plan.num_outputs] *
              plan.elem_size[prm0 + (b - plan.num_inputs - plan.num_outputs)];
    rc = ensure(bufs[b], bytes);
    if (rc == SODA_HIP_OK &&
        hipMemsetAsync(bufs[b].ptr, 0x3f, bytes, stream) != hipSuccess)
      rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipMemsetAsync");
  }
  std::vector<double> ns(plan.num_passes, 0.0);
  // Two rounds over all the passes bring the clocks up (a burst of launches a
  // millisecond after idle reads 20-30 % slow, and not equally per pass: the
  // issue-bound deep passes follow the core clock, the memory-bound shallow
  // ones do not); then kTimedRounds rounds in which every pass runs once
  // untimed and `launches` times inside an event pair -- a schedule runs a
  // pass many times in a row, and the first launch behind a different kernel
  // is not representative (jacobi2d T = 12 right behind the memory-bound
  // T = 1: 167 us, sustained 146).  A pass's time is the SHORTEST of its
  // rounds: the clocks keep rising through the first milliseconds, and one
  // round alone priced T = 13 at 161-173 us (sustained 144), enough to flip
  // the schedule of 100 iterations between 4 x 13 + 4 x 12 and 7 x 12 + 2 x 8
  // from run to run.  Nothing synchronises in between, so the GPU never idles.
  constexpr int kTimedRounds = 4;
  std::vector<hipEvent_t> ev(2 * plan.num_passes * kTimedRounds, nullptr);
  for (auto& e : ev)
    if (rc == SODA_HIP_OK && hipEventCreate(&e) != hipSuccess)
      rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipEventCreate");
  if (rc == SODA_HIP_OK) {
    for (int i = 0; i < plan.num_inputs; ++i) ins.push_back(bufs[i].ptr);
    for (int k = 0; k < plan.num_params; ++k)
      ins.push_back(bufs[plan.num_inputs + plan.num_outputs + k].ptr);
    for (int o = 0; o < plan.num_outputs; ++o)
      outs.push_back(bufs[plan.num_inputs + o].ptr);
    // `n` iterations by launches of pass i alone
    auto run_pass = [&](int i, int32_t n) {
      RunRequest rq = {outs.data(), ins.data(), key.data(), n, stream_};
      rq.force_pass = i;
      rq.batch = batch;
      return run_core(p, rq);
    };
    for (int round = 0; round < 2 && rc == SODA_HIP_OK; ++round)
      for (int i = 0; i < plan.num_passes && rc == SODA_HIP_OK; ++i)
        rc = run_pass(i, plan.passes[i].fused_iters * launches);
    for (int round = 0; round < kTimedRounds && rc == SODA_HIP_OK; ++round)
      for (int i = 0; i < plan.num_passes && rc == SODA_HIP_OK; ++i) {
        const int32_t one = plan.passes[i].fused_iters;
        hipEvent_t* pair = &ev[2 * (round * plan.num_passes + i)];
        rc = run_pass(i, one);
        if (rc != SODA_HIP_OK) break;
        if (hipEventRecord(pair[0], stream) != hipSuccess)
          rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipEventRecord");
        if (rc != SODA_HIP_OK) break;
        rc = run_pass(i, one * launches);
        if (rc == SODA_HIP_OK && hipEventRecord(pair[1], stream) != hipSuccess)
          rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipEventRecord");
      }
    if (rc == SODA_HIP_OK && hipStreamSynchronize(stream) != hipSuccess)
      rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipStreamSynchronize");
    for (int i = 0; i < plan.num_passes && rc == SODA_HIP_OK; ++i)
      for (int round = 0; round < kTimedRounds && rc == SODA_HIP_OK; ++round) {
        float ms = 0;
        hipEvent_t* pair = &ev[2 * (round * plan.num_passes + i)];
        if (hipEventElapsedTime(&ms, pair[0], pair[1]) != hipSuccess)
          rc = fail(SODA_HIP_ERR_RUNTIME, "calibrate: hipEventElapsedTime");
        const double t = ms * 1e6 / launches;
        if (round == 0 || t < ns[i]) ns[i] = t;
      }
  }
  for (auto& e : ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& b : bufs)
    if (b.ptr) (void)hipFree(b.ptr);
  if (rc == SODA_HIP_OK) {
    measured[key] = ns;
    auto it = extents.find(key);        // schedules made from the model
    if (it != extents.end()) it->second.sched.clear();
  }
  return rc;
}

int soda_hip_program_set_auto_calibrate(soda_hip_program_t* p, int on) {
  if (!p) return fail(SODA_HIP_ERR_INVALID, "NULL program");
  p->auto_calibrate = on != 0;
  return SODA_HIP_OK;
}

int soda_hip_program_pass_times(soda_hip_program_t* p, const int32_t* extent,
                                float* pass_ns, int32_t* measured) {
  return soda_hip_program_pass_times_batch(p, extent, 1, pass_ns, measured);
}

int soda_hip_program_pass_times_batch(soda_hip_program_t* p,
                                      const int32_t* extent, int32_t batch,
                                      float* pass_ns, int32_t* measured) {
  if (!p || !extent || !pass_ns)
    return fail(SODA_HIP_ERR_INVALID, "pass_times: NULL argument");
  if (int rc = check_program_batch(p, batch, "pass_times")) return rc;
  const soda_hip_plan_t& plan = p->plan;
  std::array<int32_t, SODA_HIP_MAX_DIM> key;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) key[d] = d < plan.dim ? extent[d] : 1;
  const std::map<ExtentKey, std::vector<double>>& known = measured_of(p, batch);
  auto it = known.find(key);
  if (measured) *measured = it != known.end();
  if (it != known.end()) {
    for (int i = 0; i < plan.num_passes; ++i) pass_ns[i] = (float)it->second[i];
    return SODA_HIP_OK;
  }
  return plan_geometry_c(&plan, key.data(), nullptr, pass_ns, batch);
}

int soda_hip_program_schedule(soda_hip_program_t* p, const int32_t* extent,
                              int32_t iterate, int32_t* count) {
  return soda_hip_program_schedule_batch(p, extent, 1, iterate, count);
}

int soda_hip_program_schedule_batch(soda_hip_program_t* p,
                                    const int32_t* extent, int32_t batch,
                                    int32_t iterate, int32_t* count) {
  if (!p || !extent || !count)
    return fail(SODA_HIP_ERR_INVALID, "program_schedule: NULL argument");
  if (iterate < 1) return fail(SODA_HIP_ERR_INVALID, "cannot iterate < 1 times");
  std::vector<float> ns(p->plan.num_passes);
  if (int rc = soda_hip_program_pass_times_batch(p, extent, batch, ns.data(),
                                                 nullptr))
    return rc;
  std::vector<double> t(ns.begin(), ns.end());
  int32_t total = 0;
  return schedule(p->plan, t, iterate, count, &total);
}

int soda_hip_program_set_debug_buffer(soda_hip_program_t* p, void* buf) {
  if (!p) return fail(SODA_HIP_ERR_INVALID, "NULL program");
  p->debug = buf;
  return SODA_HIP_OK;
}

int soda_hip_last_launches(soda_hip_program_t* p, int32_t* launches,
                           int32_t* fused_launches) {
  if (!p) return fail(SODA_HIP_ERR_INVALID, "NULL program");
  if (launches) *launches = p->last_launches;
  if (fused_launches) *fused_launches = p->last_fused;
  return SODA_HIP_OK;
}

int soda_hip_last_split(soda_hip_program_t* p, int32_t* passes) {
  if (!p || !passes) return fail(SODA_HIP_ERR_INVALID, "NULL argument");
  *passes = p->last_split;
  return SODA_HIP_OK;
}

int soda_hip_last_rows(soda_hip_program_t* p, int64_t* rows) {
  if (!p || !rows) return fail(SODA_HIP_ERR_INVALID, "NULL argument");
  *rows = p->last_rows;
  return SODA_HIP_OK;
}

static void add_scratch(const std::vector<DeviceBuffer>& bufs, int64_t* bytes,
                        int32_t* regrown) {
  for (const DeviceBuffer& b : bufs) {
    if (bytes && b.ptr) *bytes += (int64_t)b.bytes;
    if (regrown) *regrown += b.regrown;
  }
}

int soda_hip_program_scratch(soda_hip_program_t* p, int64_t* bytes,
                             int32_t* regrown) {
  if (!p) return fail(SODA_HIP_ERR_INVALID, "NULL program");
  if (bytes) *bytes = 0;
  if (regrown) *regrown = 0;
  for (const auto* v : {&p->locals, &p->temps, &p->temps2, &p->until_tmp})
    add_scratch(*v, bytes, regrown);
  return SODA_HIP_OK;
}

// -- memory / timing helpers ---------------------------------------------------

int soda_hip_malloc(int32_t device, size_t bytes, void** ptr) {
  if (!ptr) return fail(SODA_HIP_ERR_INVALID, "malloc: NULL ptr");
  *ptr = nullptr;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1));
  return SODA_HIP_OK;
}

int soda_hip_free(int32_t device, void* ptr) {
  if (!ptr) return SODA_HIP_OK;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipFree(ptr));
  return SODA_HIP_OK;
}

int soda_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice,
                         static_cast<hipStream_t>(stream)));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost,
                         static_cast<hipStream_t>(stream)));
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_memcpy_d2d(void* dst, int32_t dst_device, const void* src,
                        int32_t src_device, size_t bytes, void* stream) {
  if (dst_device == src_device)
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice,
                           static_cast<hipStream_t>(stream)));
  else
    HIP_TRY(hipMemcpyPeerAsync(dst, dst_device, src, src_device, bytes,
                               static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_memset(void* dst, int value, size_t bytes, void* stream) {
  HIP_TRY(hipMemsetAsync(dst, value, bytes, static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_stream_synchronize(void* stream) {
  HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_event_create(soda_hip_event_t** event) {
  if (!event) return fail(SODA_HIP_ERR_INVALID, "event_create: NULL");
  soda_hip_event* e = new (std::nothrow) soda_hip_event;
  if (!e) return fail(SODA_HIP_ERR_NOMEM, "new event");
  hipError_t err = hipEventCreate(&e->ev);
  if (err != hipSuccess) {
    delete e;
    return hip_fail(err, "hipEventCreate");
  }
  *event = e;
  return SODA_HIP_OK;
}

int soda_hip_event_record(soda_hip_event_t* event, void* stream) {
  if (!event) return fail(SODA_HIP_ERR_INVALID, "event_record: NULL");
  HIP_TRY(hipEventRecord(event->ev, static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_event_elapsed_ms(soda_hip_event_t* start, soda_hip_event_t* stop,
                              float* ms) {
  if (!start || !stop || !ms)
    return fail(SODA_HIP_ERR_INVALID, "event_elapsed: NULL");
  HIP_TRY(hipEventSynchronize(stop->ev));
  HIP_TRY(hipEventElapsedTime(ms, start->ev, stop->ev));
  return SODA_HIP_OK;
}

int soda_hip_event_handle(soda_hip_event_t* event, void** hip_event) {
  if (!event || !hip_event) return fail(SODA_HIP_ERR_INVALID, "event_handle: NULL");
  *hip_event = event->ev;
  return SODA_HIP_OK;
}

int soda_hip_hipstream_create(int32_t device, void** stream) {
  if (!stream) return fail(SODA_HIP_ERR_INVALID, "hipstream_create: NULL");
  *stream = nullptr;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = s;
  return SODA_HIP_OK;
}

int soda_hip_hipstream_destroy(void* stream) {
  if (stream) HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
  return SODA_HIP_OK;
}

int soda_hip_hipstream_wait_event(void* stream, soda_hip_event_t* event) {
  if (!event) return fail(SODA_HIP_ERR_INVALID, "hipstream_wait_event: NULL");
  HIP_TRY(hipStreamWaitEvent(static_cast<hipStream_t>(stream), event->ev, 0));
  return SODA_HIP_OK;
}

int soda_hip_event_destroy(soda_hip_event_t* event) {
  if (!event) return SODA_HIP_OK;
  (void)hipEventDestroy(event->ev);
  delete event;
  return SODA_HIP_OK;
}

}  // extern "C"

namespace soda_detail {

int check_residual_request(const soda_hip_program* p, void* const* outputs,
                           const int32_t* extent, const void* dev,
                           const char* who) {
  return check_residual(p, outputs, extent, dev, who);
}

int check_norms_request(const soda_hip_program* p,
                        const soda_hip_norms_handle* h, void* const* outputs,
                        const int32_t* extent, const void* dev,
                        const char* who) {
  return check_norms_run(p, h, outputs, extent, dev, who);
}

bool norms_converged(const soda_hip_norms_t& acc, int32_t which, double tol,
                     bool* stop) {
  double norm = 0.0;
  if (soda_hip_norms_value(&acc, which, &norm)) return false;
  if (which == SODA_HIP_NORMS_WHICH_L2) norm = sqrt(norm);
  *stop = acc.unordered == 0 && acc.infinite == 0 && norm <= tol;
  return true;
}

}  // namespace soda_detail
