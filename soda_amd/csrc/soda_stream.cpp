// soda_stream.cpp -- the wire format: <app>_kernel on banked streams
// (include/soda_hip.h, "the reference kernel's WIRE format").  A call on device
// banks is routed once (stream_route); its look-ahead, its refusals and its
// launches all walk that route.
#include "soda_stream.h"

#include <algorithm>
#include <cstdlib>
#include <new>

using namespace soda_detail;

namespace {

// one launch of a marching kernel along the last dimension, of `dim` dimensions
bool one_kernel(const soda_hip_plan_t& plan, int dim) {
  return plan.dim == dim && plan.num_passes == 1 &&
         plan.passes[0].num_kernels == 1 &&
         plan.kernels[plan.passes[0].kernel[0]].march_dim == plan.dim;
}

// stream length in elements; false: out of range
bool stream_length(const soda_hip_stream_desc_t& d, uint64_t coalesced_data_num,
                   int32_t* n) {
  const uint64_t n64 = coalesced_data_num * (uint64_t)d.elems_per_cycle[0];
  *n = (int32_t)n64;
  return n64 >= 1 && n64 < (1ull << 31);
}

// the tensor's banks in the caller's lists
const void* const* banks_of(const StreamTensor& t, void* const* out_banks,
                            const void* const* in_banks) {
  return t.input ? in_banks + t.first : out_banks + t.first;
}

bool any_null(const StreamTensor& t, const void* const* banks) {
  for (int b = 0; b < t.banks; ++b)
    if (!banks[b]) return true;
  return false;
}

bool misaligned(const void* bank) {
  return reinterpret_cast<uintptr_t>(bank) & 15;
}

// Dense view: a stream of n elements is an array of extent (tile..., rows) iff
// every tile starts on a row-block boundary -- a tile occupies
// round_up(block * extent_last, epc) elements (frt/host.py:137-142), so for any
// extent iff block % epc == 0 -- and the void tail (kStencilDistance elements,
// :151-162) covers the partial last row the view drops.
bool dense_view(const soda_hip_stream* s, int64_t n, int32_t* ext) {
  const soda_hip_stream_desc_t& d = s->desc;
  if (s->dense_failed || d.dim < 2) return false;
  int64_t block = 1;
  for (int t = 0; t < d.dim - 1; ++t) block *= d.tile[t];
  const int64_t rows = n / block;
  if (rows < 1 || d.stencil_distance < block ||
      block % d.elems_per_cycle[0] != 0)
    return false;
  for (int t = 0; t < SODA_HIP_MAX_DIM; ++t) ext[t] = 1;
  for (int t = 0; t < d.dim - 1; ++t) ext[t] = d.tile[t];
  ext[d.dim - 1] = (int32_t)rows;
  return true;
}

// Does this call run the banked form of the dense program, on the dense view
// `ext`?  Every reason not to is found HERE: an extent the kernels refuse, a
// schedule of the dense program that the banked programs do not cover, a bank
// of an in_kernel tensor that is NULL or not 16-byte aligned.  *launches: 0 =
// no (the call runs as without a banked program), 1 = `banked`, 2 =
// `banked_first` then `banked_last`.
//
// The schedule is the MODEL's (soda_hip_stream_set_banked turns the clock's
// calibration of the stream's dense program off, so the copy path of the same
// stream is scheduled from the same source): the one fused launch, or -- two
// iterations -- two launches of the one-iteration kernel.
int banked_launches(const soda_hip_stream* s, void* const* out_banks,
                    const void* const* in_banks, const int32_t* ext,
                    int* launches) {
  const soda_hip_stream_desc_t& d = s->desc;
  *launches = 0;
  int want = 1;
  if (d.iterate > 1) {
    if (!s->dense) return SODA_HIP_OK;
    int32_t count[SODA_HIP_MAX_PASSES];
    const int rc = soda_hip_program_schedule(s->dense, ext, d.iterate, count);
    if (rc == SODA_HIP_ERR_INVALID) return SODA_HIP_OK;   // no dense run either
    if (rc) return rc;
    const soda_hip_plan_t& dp = s->dense->plan;
    int total = 0, deepest = 0;
    for (int i = 0; i < dp.num_passes; ++i) {
      total += count[i];
      if (count[i] && !deepest) deepest = dp.passes[i].fused_iters;
    }
    if (total == 1 && deepest == d.iterate)
      want = 1;
    else if (total == 2 && deepest == 1 && s->banked_first && s->banked_last)
      want = 2;
    else
      return SODA_HIP_OK;
  }
  for (const soda_hip_program* p : {want == 1 ? s->banked : s->banked_first,
                                    want == 1 ? s->banked : s->banked_last}) {
    const int rc = soda_hip_plan_geometry(&p->plan, ext, nullptr, nullptr);
    if (rc == SODA_HIP_ERR_INVALID) return SODA_HIP_OK;
    if (rc) return rc;
  }
  for (size_t t = 0; t < s->tensors.size(); ++t) {
    const void* const* banks = banks_of(s->tensors[t], out_banks, in_banks);
    for (int b = 0; s->in_kernel[t] && b < s->tensors[t].banks; ++b)
      if (!banks[b] || misaligned(banks[b])) return SODA_HIP_OK;
  }
  *launches = want;
  return SODA_HIP_OK;
}

void add_launch(StreamRoute* r, soda_hip_program* program, const int32_t* ext,
                int32_t iterate, int32_t stream_elems, int tensor) {
  RouteLaunch& l = r->launches[r->num_launches++];
  l.program = program;
  for (int t = 0; t < SODA_HIP_MAX_DIM; ++t) l.extent[t] = ext[t];
  l.iterate = iterate;
  l.stream_elems = stream_elems;
  l.tensor = tensor;
}

}  // namespace

namespace soda_detail {

int stream_route(soda_hip_stream* s, void* const* out_banks,
                 const void* const* in_banks, int32_t n, StreamRoute* r) {
  const soda_hip_stream_desc_t& d = s->desc;
  const int nt = (int)s->tensors.size();
  const int32_t ext1[SODA_HIP_MAX_DIM] = {n, 1, 1, 1};
  r->n = n;
  r->num_buffers = r->num_launches = 0;
  r->linear_pick = d.num_linear - 1;
  for (int k = d.num_linear - 1; k >= 0; --k)
    if (n % d.linear_vec[k] == 0) r->linear_pick = k;      // the widest that fits
  // the form: dense view, else linear; the banked form of the dense program
  // where there is one and nothing speaks against it
  r->form = kLinear;
  if (d.tile[0] >= s->device_dense_min_tile0 && dense_view(s, n, r->extent)) {
    int banked = 0;
    if (s->banked)
      if (int rc = banked_launches(s, out_banks, in_banks, r->extent, &banked))
        return rc;
    if (banked) {
      r->form = banked == 1 ? kBankedOne : kBankedTwo;
    } else {
      // an extent that does not suit the dense kernels goes linear
      ExtentPlan* ep = nullptr;
      const int rc = extent_plan(s->dense->plan, &extents_of(s->dense, 1),
                                 r->extent, &ep);
      if (rc && rc != SODA_HIP_ERR_INVALID) return rc;
      if (!rc) r->form = kDenseView;
    }
  }
  // the tensors: their roles, the staging arrays and copy kernels of the
  // staged ones (a banked form takes its in_kernel tensors bank by bank -- no
  // copy kernel, no staging array -- every other tensor as always)
  for (int t = 0; t < nt; ++t) {
    const StreamTensor& st = s->tensors[t];
    soda_hip_program* copy =
        st.input ? s->unwire[t] : s->wire[t - d.num_inputs];
    r->staging[t] = -1;
    if (r->banked() && s->in_kernel[t]) {
      r->role[t] = kByBank;
    } else if (st.input ? st.banks == 1 && st.shift == 0 : !copy) {
      r->role[t] = kInPlace;
    } else {
      r->role[t] = kStaged;
      r->staging[t] = r->num_buffers;
      // (a new dense_out: the dense view drops the partial last row, whose
      // bytes would otherwise reach the caller's banks uninitialised through
      // wire_<out>)
      r->buffers[r->num_buffers++] = {
          st.input ? &s->dense_in[t] : &s->dense_out[t - d.num_inputs],
          (size_t)n * st.elem, !st.input};
      if (st.input) add_launch(r, copy, ext1, 1, 0, t);
    }
  }
  // the program, on the dense view where there is one
  if (r->form == kBankedTwo) {
    // two one-iteration launches, a dense temporary per output between them
    for (int o = 0; o < d.num_outputs; ++o)
      r->buffers[r->num_buffers++] = {
          &s->banked_tmp[o], (size_t)n * s->tensors[d.num_inputs + o].elem,
          false};
    add_launch(r, s->banked_first, r->extent, 1, n, -1);
    add_launch(r, s->banked_last, r->extent, 1, n, -1);
  } else if (r->form == kBankedOne) {
    add_launch(r, s->banked, r->extent, 1, n, -1);
  } else if (r->form == kDenseView) {
    add_launch(r, s->dense, r->extent, d.iterate, 0, -1);
  } else {
    add_launch(r, s->linear[r->linear_pick], ext1, d.iterate, 0, -1);
  }
  // outputs: shifted by the stencil offset, re-interleaved
  for (int t = d.num_inputs; t < nt; ++t)
    if (r->role[t] == kStaged)
      add_launch(r, s->wire[t - d.num_inputs], ext1, 1, 0, t);
  return SODA_HIP_OK;
}

int route_grows(const StreamRoute& r, bool* grows,
                std::vector<const void*>* asked) {
  *grows = false;
  for (int b = 0; b < r.num_buffers; ++b) {
    if (asked) asked->push_back(r.buffers[b].buf);
    if (too_small(*r.buffers[b].buf, r.buffers[b].bytes)) *grows = true;
  }
  for (int k = 0; k < r.num_launches; ++k) {
    const RouteLaunch& l = r.launches[k];
    if (asked) asked->push_back(l.program);
    if (int rc = program_grows(l.program, l.extent, l.iterate, grows)) return rc;
  }
  return SODA_HIP_OK;
}

int route_refusal(const soda_hip_stream* s, const StreamRoute& r,
                  void* const* out_banks, const void* const* in_banks) {
  for (size_t t = 0; t < s->tensors.size(); ++t) {
    const StreamTensor& st = s->tensors[t];
    const void* const* banks = banks_of(st, out_banks, in_banks);
    if (any_null(st, banks))
      return fail(SODA_HIP_ERR_INVALID, st.input ? "stream_run: NULL input bank"
                                                 : "stream_run: NULL output bank");
    if (r.role[t] == kInPlace && misaligned(banks[0]))
      return fail(SODA_HIP_ERR_INVALID,
                  st.input ? "stream_run: a bank the program reads in place "
                             "must be 16-byte aligned"
                           : "stream_run: a bank the program writes in place "
                             "must be 16-byte aligned");
  }
  return SODA_HIP_OK;
}

}  // namespace soda_detail

extern "C" {

int soda_hip_stream_create(const soda_hip_stream_desc_t* desc,
                           soda_hip_program_t* dense,
                           soda_hip_program_t* const* linear,
                           soda_hip_program_t* const* unwire,
                           soda_hip_program_t* const* wire,
                           soda_hip_stream_t** stream) {
  if (!desc || !linear || !wire || !stream)
    return fail(SODA_HIP_ERR_INVALID, "stream_create: NULL argument");
  *stream = nullptr;
  const int nt = desc->num_inputs + desc->num_outputs;
  if (desc->dim < 1 || desc->dim > SODA_HIP_MAX_DIM || desc->num_inputs < 1 ||
      desc->num_outputs < 1 || nt > SODA_HIP_MAX_TENSORS || desc->iterate < 1 ||
      desc->num_linear < 1 || desc->num_linear > 4 ||
      desc->linear_vec[desc->num_linear - 1] != 1)
    return fail(SODA_HIP_ERR_INVALID, "stream_create: bad description");
  for (int t = 0; t < nt; ++t)
    if (desc->banks[t] < 1 || desc->elem_size[t] < 1 ||
        desc->elems_per_cycle[t] < 1 || desc->shift[t] < 0)
      return fail(SODA_HIP_ERR_INVALID, "stream_create: bad tensor entry");
  for (int t = 1; t < nt; ++t)
    if (desc->elems_per_cycle[t] != desc->elems_per_cycle[0])
      return fail(SODA_HIP_ERR_UNSUPPORTED,
                  "stream mode needs every tensor to move the same number of "
                  "elements per cycle (burst width / element width x banks)");
  for (int i = 0; i < desc->num_inputs; ++i)
    if ((desc->banks[i] > 1 || desc->shift[i]) && (!unwire || !unwire[i]))
      return fail(SODA_HIP_ERR_INVALID, "stream_create: missing unwire kernel");
  for (int k = 0; k < desc->num_linear; ++k)
    if (!linear[k]) return fail(SODA_HIP_ERR_INVALID, "stream_create: NULL linear");
  // an output on one bank that the program stores at its wire position (shift
  // 0) needs no copy kernel: the program writes the caller's bank
  for (int o = 0; o < desc->num_outputs; ++o) {
    const int t = desc->num_inputs + o;
    if (!wire[o] && (desc->banks[t] > 1 || desc->shift[t]))
      return fail(SODA_HIP_ERR_INVALID, "stream_create: missing wire kernel");
  }
  soda_hip_stream* s = new (std::nothrow) soda_hip_stream;
  if (!s) return fail(SODA_HIP_ERR_NOMEM, "new stream");
  s->desc = *desc;
  int32_t first = 0;
  for (int t = 0; t < nt; first += desc->banks[t], ++t) {
    if (t == desc->num_inputs) first = 0;    // outputs: a list of their own
    s->tensors.push_back({first, desc->banks[t], desc->elem_size[t],
                          desc->shift[t], t < desc->num_inputs});
  }
  s->dense = dense;
  s->dense_failed = dense == nullptr;
  s->linear.assign(linear, linear + desc->num_linear);
  s->unwire.resize(desc->num_inputs, nullptr);
  for (int i = 0; unwire && i < desc->num_inputs; ++i) s->unwire[i] = unwire[i];
  s->wire.assign(wire, wire + desc->num_outputs);
  for (soda_hip_program* c : s->unwire) if (c) c->bank_tensors = true;
  for (soda_hip_program* c : s->wire) if (c) c->bank_tensors = true;
  s->dense_in.resize(desc->num_inputs);
  s->dense_out.resize(desc->num_outputs);
  *stream = s;
  return SODA_HIP_OK;
}

int soda_hip_stream_destroy(soda_hip_stream_t* s) {
  if (!s) return SODA_HIP_OK;
  for (auto* v : {&s->dense_in, &s->dense_out, &s->host_banks, &s->banked_tmp})
    for (auto& b : *v)
      if (b.ptr) (void)hipFree(b.ptr);
  delete s;
  return SODA_HIP_OK;
}

int soda_hip_stream_last_mode(soda_hip_stream_t* s) { return s ? s->last_mode : 0; }

int soda_hip_stream_set_device_dense_min_tile(soda_hip_stream_t* s,
                                              int32_t min_tile0) {
  if (!s || min_tile0 < 0)
    return fail(SODA_HIP_ERR_INVALID, "stream_set_device_dense_min_tile");
  s->device_dense_min_tile0 = min_tile0;
  s->warm.clear();
  return SODA_HIP_OK;
}

int soda_hip_stream_set_banked(soda_hip_stream_t* s, soda_hip_program_t* program,
                               const int32_t* in_kernel) {
  if (!s) return fail(SODA_HIP_ERR_INVALID, "stream_set_banked: NULL stream");
  s->warm.clear();
  if (!program) {
    s->banked = s->banked_first = s->banked_last = nullptr;
    s->in_kernel.clear();
    if (s->dense) s->dense->auto_calibrate = !getenv("SODA_HIP_NO_CALIBRATE");
    return SODA_HIP_OK;
  }
  if (!in_kernel)
    return fail(SODA_HIP_ERR_INVALID, "stream_set_banked: NULL mask");
  const soda_hip_stream_desc_t& d = s->desc;
  const soda_hip_plan_t& plan = program->plan;
  int ins = 0, outs = 0;
  bool any = false;
  for (size_t t = 0; t < s->tensors.size(); ++t) {
    const StreamTensor& st = s->tensors[t];
    const int nb = st.banks;
    if (in_kernel[t]) {
      // fragments start on bank-group boundaries only if NB divides the tile
      // row; a delay is undone by starting shift / NB elements into each bank
      if ((nb != 2 && nb != 4) || d.tile[0] % nb || st.shift % nb ||
          (!st.input && st.shift))
        return fail(SODA_HIP_ERR_INVALID,
                    "stream_set_banked: a tensor the program cannot address "
                    "bank by bank");
      any = true;
    } else if (!st.input && !s->wire[t - d.num_inputs] && nb != 1) {
      return fail(SODA_HIP_ERR_INVALID, "stream_set_banked: missing wire kernel");
    }
    (st.input ? ins : outs) += in_kernel[t] ? nb : 1;
  }
  if (!any || d.dim < 2 || !one_kernel(plan, d.dim) || plan.num_inputs != ins ||
      plan.num_outputs != outs || ins + outs >= SODA_HIP_MAX_TENSORS)
    return fail(SODA_HIP_ERR_INVALID,
                "stream_set_banked: not the one-launch banked form of this "
                "stream's program");
  s->banked = program;
  program->bank_tensors = true;
  s->banked_first = s->banked_last = nullptr;
  s->in_kernel.assign(in_kernel, in_kernel + s->tensors.size());
  // one source for both paths of this stream: which launches a run takes is
  // asked of the dense program's MODEL schedule (banked_launches), so the
  // copy path of the same stream must not re-schedule from the clock
  if (s->dense) s->dense->auto_calibrate = false;
  return SODA_HIP_OK;
}

int soda_hip_stream_set_banked_pair(soda_hip_stream_t* s,
                                    soda_hip_program_t* first,
                                    soda_hip_program_t* last) {
  if (!s || !s->banked)
    return fail(SODA_HIP_ERR_INVALID,
                "stream_set_banked_pair: no banked program is set");
  s->warm.clear();
  if (!first && !last) {
    s->banked_first = s->banked_last = nullptr;
    return SODA_HIP_OK;
  }
  const soda_hip_stream_desc_t& d = s->desc;
  const soda_hip_plan_t& whole = s->banked->plan;
  if (d.iterate != 2 || d.num_inputs != d.num_outputs || !first || !last ||
      !one_kernel(first->plan, d.dim) || !one_kernel(last->plan, d.dim) ||
      first->plan.num_inputs != whole.num_inputs ||
      first->plan.num_outputs != d.num_outputs ||
      last->plan.num_inputs != d.num_inputs ||
      last->plan.num_outputs != whole.num_outputs)
    return fail(SODA_HIP_ERR_INVALID,
                "stream_set_banked_pair: not the two one-iteration launches of "
                "this stream's two-iteration program");
  for (int o = 0; o < d.num_outputs; ++o)
    if (d.elem_size[o] != d.elem_size[d.num_inputs + o])
      return fail(SODA_HIP_ERR_INVALID,
                  "stream_set_banked_pair: input and output cell sizes differ");
  s->banked_first = first;
  s->banked_last = last;
  first->bank_tensors = last->bank_tensors = true;
  s->banked_tmp.resize(d.num_outputs);
  return SODA_HIP_OK;
}

// the route's buffers, new output staging zero-filled on the caller's stream
static int route_allocate(const StreamRoute& r, hipStream_t stream) {
  for (int b = 0; b < r.num_buffers; ++b) {
    DeviceBuffer& buf = *r.buffers[b].buf;
    const void* before = buf.ptr;
    if (int rc = ensure(buf, r.buffers[b].bytes)) return rc;
    if (r.buffers[b].zero_new && buf.ptr != before)
      HIP_TRY(hipMemsetAsync(buf.ptr, 0, buf.bytes, stream));
  }
  return SODA_HIP_OK;
}

// the route's launches in order; *mode: what soda_hip_stream_last_mode tells
static int route_launch(soda_hip_stream* s, const StreamRoute& r,
                        void* const* out_banks, const void* const* in_banks,
                        void* hip_stream, int* mode) {
  // what the program reads and writes: one entry per tensor, NB per kByBank
  // one; the temporaries between the two launches of kBankedTwo
  std::vector<const void*> din;
  std::vector<void*> dout, tmp;
  for (size_t t = 0; t < s->tensors.size(); ++t) {
    const StreamTensor& st = s->tensors[t];
    const void* const* banks = banks_of(st, out_banks, in_banks);
    for (int b = 0; b < (r.role[t] == kByBank ? st.banks : 1); ++b) {
      // (in place: the bank IS the dense stream / born at its wire position)
      const void* at = r.role[t] == kStaged ? r.buffers[r.staging[t]].buf->ptr
                                            : banks[b];
      if (st.input) din.push_back(at);
      else dout.push_back(const_cast<void*>(at));
    }
  }
  for (size_t o = 0; r.form == kBankedTwo && o < s->banked_tmp.size(); ++o)
    tmp.push_back(s->banked_tmp[o].ptr);
  *mode = r.banked() ? 3 : r.form == kDenseView ? 1 : 2;
  bool second = false;      // of the two launches of kBankedTwo
  for (int k = 0; k < r.num_launches; ++k) {
    const RouteLaunch& l = r.launches[k];
    void* const* outs = dout.data();
    const void* const* ins = din.data();
    void* stage[1];
    if (l.tensor >= 0) {       // a copy kernel: the banks <-> the staging array
      const StreamTensor& st = s->tensors[l.tensor];
      stage[0] = r.buffers[r.staging[l.tensor]].buf->ptr;
      if (st.input) outs = stage, ins = in_banks + st.first;
      else outs = out_banks + st.first, ins = stage;
    } else if (r.form == kBankedTwo) {
      if (second) ins = tmp.data();
      else outs = tmp.data();
      second = true;
    }
    l.program->stream_elems = l.stream_elems;
    int rc = soda_hip_run_device(l.program, outs, ins, l.extent, l.iterate,
                                 hip_stream);
    if (rc == SODA_HIP_ERR_INVALID && r.form == kDenseView && l.tensor < 0) {
      // the dense program refuses for a reason the route did not foresee (the
      // route asks its geometry only): the call goes linear, as it always has
      const int32_t ext1[1] = {r.n};
      rc = soda_hip_run_device(s->linear[r.linear_pick], outs, ins, ext1,
                               l.iterate, hip_stream);
      *mode = 2;
    }
    if (rc) return rc;
  }
  return SODA_HIP_OK;
}

int soda_hip_stream_run_device(soda_hip_stream_t* s, void* const* out_banks,
                               const void* const* in_banks,
                               uint64_t coalesced_data_num, void* hip_stream) {
  if (!s || !out_banks || !in_banks)
    return fail(SODA_HIP_ERR_INVALID, "stream_run: NULL argument");
  int32_t n;
  if (!stream_length(s->desc, coalesced_data_num, &n))
    return fail(SODA_HIP_ERR_INVALID, "stream_run: stream length out of range");
  HIP_TRY(hipSetDevice(s->linear.back()->device));
  StreamRoute r;
  if (int rc = stream_route(s, out_banks, in_banks, n, &r)) return rc;
  // A length that has not run this way before may allocate.  On a stream that
  // is being captured that is refused here, ahead of whatever else is wrong
  // with the call.
  const std::pair<int32_t, int> key(n, r.banked());
  const bool warm =
      std::find(s->warm.begin(), s->warm.end(), key) != s->warm.end();
  if (!warm) {
    bool grows = false;
    if (route_grows(r, &grows) == SODA_HIP_OK && grows)
      if (int rc = refuse_growth_while_capturing(hip_stream, "stream_run"))
        return rc;
  }
  if (int rc = route_refusal(s, r, out_banks, in_banks)) return rc;
  // nothing is launched before this line
  if (int rc = route_allocate(r, static_cast<hipStream_t>(hip_stream)))
    return rc;
  int mode = 0;
  if (int rc = route_launch(s, r, out_banks, in_banks, hip_stream, &mode))
    return rc;
  s->last_mode = mode;
  if (!warm) {
    if (s->warm.size() >= 64) s->warm.clear();
    s->warm.push_back(key);
  }
  return SODA_HIP_OK;
}

int soda_hip_stream_run_host(soda_hip_stream_t* s, void* const* out_banks,
                             const void* const* in_banks,
                             uint64_t coalesced_data_num) {
  if (!s || !out_banks || !in_banks)
    return fail(SODA_HIP_ERR_INVALID, "stream_run_host: NULL argument");
  const soda_hip_stream_desc_t& d = s->desc;
  int32_t n;
  const bool in_range = stream_length(d, coalesced_data_num, &n);
  // Every tensor on one bank that the program reads / writes in place, and the
  // stream a dense array of rows: the caller's banks ARE host arrays of the
  // n-D program, and the call is the host-array entry's (soda_host.cpp) --
  // copy-in, kernels and copy-out overlapped in bands along the rows.  The
  // elements of the partial last row stay as the caller left them (void tail).
  // Banked tensors ride along: their (de)interleave is done by the host
  // threads in the pack / unpack step instead of by copy kernels on the GPU.
  bool in_place = !getenv("SODA_HIP_STREAM_NO_BANDS");
  // (a delayed input on ONE bank is un-delayed in the pack step as well)
  for (const StreamTensor& st : s->tensors)
    in_place = in_place && (st.shift == 0 || (st.input && st.banks == 1));
  int32_t ext[SODA_HIP_MAX_DIM];
  if (in_place && in_range && dense_view(s, n, ext)) {
    int32_t stride[SODA_HIP_MAX_DIM];
    int64_t run = 1;
    for (int t = 0; t < SODA_HIP_MAX_DIM; ++t) {
      stride[t] = run > INT32_MAX ? INT32_MAX : (int32_t)run;   // (t >= dim: unread)
      run *= ext[t];
    }
    std::vector<soda_hip_host_tensor_t> tin, tout;
    for (const StreamTensor& st : s->tensors) {
      const void* const* banks = banks_of(st, out_banks, in_banks);
      if (any_null(st, banks))
        return fail(SODA_HIP_ERR_INVALID, "stream_run_host: NULL bank");
      // one bank: the array itself; several: the list of them
      (st.input ? tin : tout).push_back(
          {const_cast<void*>(st.banks == 1 ? banks[0]
                                           : static_cast<const void*>(banks)),
           ext, stride, nullptr});
    }
    int rc = run_host_call(s->dense, tin.data(), tout.data(), d.iterate,
                           nullptr, nullptr, d.banks, d.shift, n);
    if (rc == SODA_HIP_OK) s->last_mode = 1;
    if (rc != SODA_HIP_ERR_INVALID) return rc;
    // INVALID: this extent does not suit the dense kernels; the long way
  }
  // Otherwise the banks -- the generated host's pageable `aligned_alloc`
  // buffers (ref frt/host.py:165-178) -- travel whole through the pinned rings
  // and the worker threads of the host-array entry, on one stream with the
  // kernels.
  soda_hip_program* owner = s->linear.back();
  hipStream_t stream = nullptr;
  if (int rc = host_stream(owner, &stream)) return rc;
  size_t total = 0;
  for (const StreamTensor& st : s->tensors) {
    if (any_null(st, banks_of(st, out_banks, in_banks)))
      return fail(SODA_HIP_ERR_INVALID,
                  st.input ? "stream_run_host: NULL input bank"
                           : "stream_run_host: NULL output bank");
    total += st.banks;
  }
  s->host_banks.resize(total);
  std::vector<const void*> dev_in;
  std::vector<void*> dev_out;
  std::vector<size_t> out_bytes;
  size_t slot = 0;      // inputs first, then outputs, like the tensors
  for (const StreamTensor& st : s->tensors)
    for (int b = 0; b < st.banks; ++b, ++slot) {
      DeviceBuffer& buf = s->host_banks[slot];
      const size_t bytes = (size_t)coalesced_data_num * d.elems_per_cycle[0] /
                           st.banks * st.elem;
      const void* before = buf.ptr;
      if (int rc = ensure(buf, bytes)) return rc;
      if (st.input) {
        if (int rc = ring_send(owner, buf.ptr, in_banks[st.first + b], bytes,
                               stream))
          return rc;
        dev_in.push_back(buf.ptr);
        continue;
      }
      // void positions a program writing in place never touches: the same
      // bytes for the caller run after run
      if (buf.ptr != before) HIP_TRY(hipMemsetAsync(buf.ptr, 0, bytes, stream));
      dev_out.push_back(buf.ptr);
      out_bytes.push_back(bytes);
    }
  if (int rc = soda_hip_stream_run_device(s, dev_out.data(), dev_in.data(),
                                          coalesced_data_num, stream))
    return rc;
  for (size_t k = 0; k < dev_out.size(); ++k)
    if (int rc = ring_fetch(owner, out_banks[k], dev_out[k], out_bytes[k],
                            stream))
      return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  return SODA_HIP_OK;
}

}  // extern "C"

