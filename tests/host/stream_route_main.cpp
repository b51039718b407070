// stream_route_main.cpp -- the route of a call on a wire stream object
// (stream_route, soda_amd/csrc/soda_stream.h) on the CPU, under a host
// sanitizer: a program with its own main built against the library's sources,
// -fsanitize=address,undefined; no GPU, nothing loaded into an interpreter.
//
// Stream objects of one input and one output of 4-byte cells, 2-D, made from
// hand-made descriptions and hand-made programs (a plan each; measured times
// where a schedule is forced).  Banks are integers cast to pointers: the route
// looks at the addresses and never behind them.  Every route is compared whole
// with one written out by hand; then the look-ahead (route_grows) must have
// looked at exactly the route's buffers and launches, every staged tensor must
// have its buffer and every launch a program.  Exit status 0: all held.
#include "soda_stream.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace soda_detail;

static int failures = 0;
#define EXPECT(cond, ...)                          \
  do {                                             \
    if (!(cond)) {                                 \
      ++failures;                                  \
      std::fprintf(stderr, "FAILED %s: ", #cond);  \
      std::fprintf(stderr, __VA_ARGS__);           \
      std::fprintf(stderr, "\n");                  \
    }                                              \
  } while (0)

static const uintptr_t kBase = 0x40000000;   // 16-byte aligned, never read

static void* at(uintptr_t a) { return reinterpret_cast<void*>(a); }

static std::string last_error() {
  char buf[512];
  soda_hip_last_error(buf, sizeof buf);
  return buf;
}

// A program that is a plan and nothing else: `fused` lists the passes' depths
// (descending, the last 1), one kernel per pass; march: 1 + the dimension the
// kernels stream along (0: none).
static soda_hip_program* program(int dim, int ins, int outs,
                                 std::vector<int> fused, int march) {
  soda_hip_program* p = new soda_hip_program;
  soda_hip_plan_t& plan = p->plan;
  std::memset(&plan, 0, sizeof plan);
  plan.abi_version = SODA_HIP_ABI_VERSION;
  plan.dim = dim;
  plan.num_inputs = ins;
  plan.num_outputs = outs;
  for (int t = 0; t < ins + outs; ++t) plan.elem_size[t] = 4;
  plan.num_kernels = plan.num_passes = (int32_t)fused.size();
  for (size_t k = 0; k < fused.size(); ++k) {
    soda_hip_kernel_desc_t& kd = plan.kernels[k];
    std::snprintf(kd.name, sizeof kd.name, "k%d", (int)k);
    kd.block[0] = 64;
    kd.block[1] = kd.block[2] = 1;
    for (int d = 0; d < dim; ++d) kd.tile[d] = d == 0 ? 64 : 4;
    kd.march_dim = march;
    kd.window_extra = -1;
    plan.passes[k].fused_iters = fused[k];
    plan.passes[k].num_kernels = 1;
    plan.passes[k].kernel[0] = (int32_t)k;
  }
  p->temps.resize(outs);
  p->temps2.resize(outs);
  return p;
}

// the programs a stream may be given, and the stream
struct Rig {
  soda_hip_program* dense;
  soda_hip_program* linear[2];
  soda_hip_program* unwire;
  soda_hip_program* wire;
  soda_hip_program* banked;   // both tensors bank by bank, all iterations
  soda_hip_program* first;    // one iteration, the input bank by bank
  soda_hip_program* last;     // one iteration, the output bank by bank
  soda_hip_stream* s = nullptr;
  soda_hip_stream_desc_t desc;

  // tile[0] = tile, stencil distance = tile, `banks` per tensor, linear
  // programs of 4 cells and of 1 cell per thread (num_linear == 2) or the latter
  Rig(int tile, int banks, int iterate, int epc = 16, int num_linear = 1) {
    dense = iterate == 2 ? program(2, 1, 1, {2, 1}, 2) : program(2, 1, 1, {1}, 2);
    for (auto& l : linear) l = program(1, 1, 1, {1}, 0);
    unwire = program(1, banks, 1, {1}, 0);
    wire = program(1, 1, banks, {1}, 0);
    banked = program(2, banks, banks, {1}, 2);
    first = program(2, banks, 1, {1}, 2);
    last = program(2, 1, banks, {1}, 2);
    std::memset(&desc, 0, sizeof desc);
    desc.dim = 2;
    desc.num_inputs = desc.num_outputs = 1;
    desc.iterate = iterate;
    desc.tile[0] = tile;
    desc.stencil_distance = tile;
    for (int t = 0; t < 2; ++t) {
      desc.banks[t] = banks;
      desc.elem_size[t] = 4;
      desc.elems_per_cycle[t] = epc;
    }
    desc.num_linear = num_linear;
    desc.linear_vec[0] = num_linear == 2 ? 4 : 1;
    desc.linear_vec[1] = 1;
  }
  void create() {
    soda_hip_program* none[1] = {nullptr};
    const int rc = soda_hip_stream_create(
        &desc, dense, linear + (2 - desc.num_linear),
        desc.banks[0] > 1 ? &unwire : none, desc.banks[0] > 1 ? &wire : none, &s);
    EXPECT(rc == SODA_HIP_OK && s, "stream_create: %s", last_error().c_str());
  }
  // measured times of the dense program's two passes on `ext`
  void force(const int32_t* ext, double fused_ns, double single_ns) {
    dense->measured[ExtentKey{{ext[0], ext[1], 1, 1}}] = {fused_ns, single_ns};
  }
  ~Rig() {
    soda_hip_stream_destroy(s);
    for (soda_hip_program* p : {dense, linear[0], linear[1], unwire, wire,
                                banked, first, last})
      delete p;
  }
};

struct WantLaunch {
  const soda_hip_program* program;
  int32_t ext0, ext1, iterate, stream_elems;
  int tensor;
};
struct WantBuffer {
  const DeviceBuffer* buf;
  size_t bytes;
  bool zero_new;
};
struct Want {
  StreamForm form;
  int linear_pick;
  int32_t ext0, ext1;                  // the dense view (read unless kLinear)
  StreamRole in_role, out_role;
  std::vector<WantBuffer> buffers;
  std::vector<WantLaunch> launches;
};

// the route of (out, in, n) against `want`, then what holds for every route
static StreamRoute judge(const char* name, Rig& rig, const std::vector<void*>& out,
                         const std::vector<const void*>& in, int32_t n,
                         const Want& want) {
  StreamRoute r;
  std::memset(&r, 0xff, sizeof r);
  const int rc = stream_route(rig.s, out.data(), in.data(), n, &r);
  EXPECT(rc == SODA_HIP_OK, "%s: stream_route: %s", name, last_error().c_str());
  if (rc) return r;
  EXPECT(r.n == n && r.form == want.form, "%s: form %d", name, (int)r.form);
  EXPECT(r.linear_pick == want.linear_pick, "%s: pick %d", name, r.linear_pick);
  if (want.form != kLinear)
    EXPECT(r.extent[0] == want.ext0 && r.extent[1] == want.ext1 &&
               r.extent[2] == 1 && r.extent[3] == 1,
           "%s: dense view %d x %d", name, r.extent[0], r.extent[1]);
  EXPECT(r.role[0] == want.in_role && r.role[1] == want.out_role,
         "%s: roles %d, %d", name, (int)r.role[0], (int)r.role[1]);
  EXPECT(r.num_buffers == (int)want.buffers.size(), "%s: %d buffers", name,
         r.num_buffers);
  for (int b = 0; b < r.num_buffers && b < (int)want.buffers.size(); ++b) {
    const WantBuffer& w = want.buffers[b];
    EXPECT(r.buffers[b].buf == w.buf && r.buffers[b].bytes == w.bytes &&
               r.buffers[b].zero_new == w.zero_new,
           "%s: buffer %d: %zu bytes, zero_new %d", name, b, r.buffers[b].bytes,
           (int)r.buffers[b].zero_new);
  }
  EXPECT(r.num_launches == (int)want.launches.size(), "%s: %d launches", name,
         r.num_launches);
  for (int k = 0; k < r.num_launches && k < (int)want.launches.size(); ++k) {
    const WantLaunch& w = want.launches[k];
    const RouteLaunch& l = r.launches[k];
    EXPECT(l.program == w.program && l.extent[0] == w.ext0 &&
               l.extent[1] == w.ext1 && l.extent[2] == 1 && l.extent[3] == 1 &&
               l.iterate == w.iterate && l.stream_elems == w.stream_elems &&
               l.tensor == w.tensor,
           "%s: launch %d: extent %d x %d, iterate %d, stream_elems %d, "
           "tensor %d", name, k, l.extent[0], l.extent[1], l.iterate,
           l.stream_elems, l.tensor);
  }
  // ---- for every route ----------------------------------------------------
  std::vector<const void*> asked, mine;
  bool grows = false;
  EXPECT(route_grows(r, &grows, &asked) == SODA_HIP_OK, "%s: route_grows: %s",
         name, last_error().c_str());
  for (int b = 0; b < r.num_buffers; ++b) mine.push_back(r.buffers[b].buf);
  for (int k = 0; k < r.num_launches; ++k) {
    mine.push_back(r.launches[k].program);
    EXPECT(r.launches[k].program != nullptr, "%s: launch %d has no program",
           name, k);
  }
  EXPECT(asked == mine, "%s: the look-ahead asked %zu things, the route has %zu",
         name, asked.size(), mine.size());
  // (nothing here was ever allocated, so a route with a buffer grows; the one
  // program that needs scratch, the dense one run as 1 + 1, comes with two)
  EXPECT(grows == (r.num_buffers > 0), "%s: grows %d", name, (int)grows);
  for (int t = 0; t < 2; ++t)
    EXPECT((r.role[t] == kStaged) ==
               (r.staging[t] >= 0 && r.staging[t] < r.num_buffers),
           "%s: tensor %d: role %d, staging %d", name, t, (int)r.role[t],
           r.staging[t]);
  return r;
}

static void refused(const char* name, int rc, const char* text) {
  EXPECT(rc == SODA_HIP_ERR_INVALID && last_error() == text, "%s: %d `%s`", name,
         rc, last_error().c_str());
}

int main() {
  const uintptr_t B = kBase;
  const std::vector<void*> out1 = {at(B)}, out2 = {at(B), at(B + 0x10000)};
  const std::vector<const void*> in1 = {at(B + 0x20000)},
                                 in2 = {at(B + 0x20000), at(B + 0x30000)};
  const int32_t n = 256 * 5 + 16;      // five rows of 256 and a void tail
  const int32_t view[2] = {256, 5};
  {  // ---- one bank per tensor, no shift, no copy kernel: all in place -------
    Rig wide(256, 1, 1);
    wide.create();
    judge("wide tile", wide, out1, in1, n,
          {kDenseView, 0, 256, 5, kInPlace, kInPlace, {},
           {{wide.dense, 256, 5, 1, 0, -1}}});
    Rig narrow(32, 1, 1);
    narrow.create();
    const Want linear = {kLinear, 0, 0, 0, kInPlace, kInPlace, {},
                         {{narrow.linear[1], n, 1, 1, 0, -1}}};
    judge("narrow tile", narrow, out1, in1, n, linear);
    EXPECT(soda_hip_stream_set_device_dense_min_tile(narrow.s, 0) == SODA_HIP_OK,
           "set_device_dense_min_tile");
    judge("narrow tile, any tile dense", narrow, out1, in1, n,
          {kDenseView, 0, 32, n / 32, kInPlace, kInPlace, {},
           {{narrow.dense, 32, n / 32, 1, 0, -1}}});
    Rig ragged(256, 1, 1, 24);         // 256 % 24 != 0: tiles start mid-row
    ragged.create();
    judge("block % elems_per_cycle != 0", ragged, out1, in1, n,
          {kLinear, 0, 0, 0, kInPlace, kInPlace, {},
           {{ragged.linear[1], n, 1, 1, 0, -1}}});
    Rig short_tail(256, 1, 1);
    short_tail.desc.stencil_distance = 255;
    short_tail.create();
    judge("stencil_distance < block", short_tail, out1, in1, n,
          {kLinear, 0, 0, 0, kInPlace, kInPlace, {},
           {{short_tail.linear[1], n, 1, 1, 0, -1}}});
    // a misaligned bank is the refusal step's: the route is the same
    const std::vector<const void*> off = {at(B + 0x20008)};
    judge("in place, misaligned", narrow, out1, off, n,
          {kDenseView, 0, 32, n / 32, kInPlace, kInPlace, {},
           {{narrow.dense, 32, n / 32, 1, 0, -1}}});
    StreamRoute r;
    stream_route(narrow.s, out1.data(), off.data(), n, &r);
    refused("in place, misaligned",
            route_refusal(narrow.s, r, out1.data(), off.data()),
            "stream_run: a bank the program reads in place must be 16-byte "
            "aligned");
  }
  {  // ---- the linear pick -----------------------------------------------------
    Rig rig(32, 1, 1, 1, 2);
    rig.create();
    judge("n % 4 == 0", rig, out1, in1, 1300,
          {kLinear, 0, 0, 0, kInPlace, kInPlace, {},
           {{rig.linear[0], 1300, 1, 1, 0, -1}}});
    judge("n % 4 != 0", rig, out1, in1, 1301,
          {kLinear, 1, 0, 0, kInPlace, kInPlace, {},
           {{rig.linear[1], 1301, 1, 1, 0, -1}}});
  }
  {  // ---- two banks in and out: staged, then the banked program --------------
    Rig rig(256, 2, 1);
    rig.create();
    const Want copies = {
        kDenseView, 0, 256, 5, kStaged, kStaged,
        {{&rig.s->dense_in[0], (size_t)n * 4, false},
         {&rig.s->dense_out[0], (size_t)n * 4, true}},
        {{rig.unwire, n, 1, 1, 0, 0}, {rig.dense, 256, 5, 1, 0, -1},
         {rig.wire, n, 1, 1, 0, 1}}};
    judge("two banks, no banked program", rig, out2, in2, n, copies);
    const int32_t both[2] = {1, 1};
    EXPECT(soda_hip_stream_set_banked(rig.s, rig.banked, both) == SODA_HIP_OK,
           "set_banked: %s", last_error().c_str());
    judge("banked", rig, out2, in2, n,
          {kBankedOne, 0, 256, 5, kByBank, kByBank, {},
           {{rig.banked, 256, 5, 1, n, -1}}});
    const std::vector<const void*> off = {in2[0], at(B + 0x30008)};
    judge("banked, a bank 8 bytes off", rig, out2, off, n, copies);
    const std::vector<void*> hole = {out2[0], nullptr};
    const StreamRoute r =
        judge("banked, a NULL bank", rig, hole, in2, n, copies);
    refused("banked, a NULL bank",
            route_refusal(rig.s, r, hole.data(), in2.data()),
            "stream_run: NULL output bank");
    EXPECT(route_refusal(rig.s, r, out2.data(), off.data()) == SODA_HIP_OK,
           "banks of a staged tensor may start anywhere: %s",
           last_error().c_str());
  }
  {  // ---- two iterations: the dense program's schedule names the launches ----
    Rig rig(256, 2, 2);
    rig.create();
    const int32_t both[2] = {1, 1};
    EXPECT(soda_hip_stream_set_banked(rig.s, rig.banked, both) == SODA_HIP_OK,
           "set_banked: %s", last_error().c_str());
    const Want copies = {
        kDenseView, 0, 256, 5, kStaged, kStaged,
        {{&rig.s->dense_in[0], (size_t)n * 4, false},
         {&rig.s->dense_out[0], (size_t)n * 4, true}},
        {{rig.unwire, n, 1, 1, 0, 0}, {rig.dense, 256, 5, 2, 0, -1},
         {rig.wire, n, 1, 1, 0, 1}}};
    rig.force(view, 10.0, 1.0);        // 1 + 1
    judge("1 + 1, no pair", rig, out2, in2, n, copies);
    EXPECT(soda_hip_stream_set_banked_pair(rig.s, rig.first, rig.last) ==
               SODA_HIP_OK, "set_banked_pair: %s", last_error().c_str());
    judge("1 + 1, pair", rig, out2, in2, n,
          {kBankedTwo, 0, 256, 5, kByBank, kByBank,
           {{&rig.s->banked_tmp[0], (size_t)n * 4, false}},
           {{rig.first, 256, 5, 1, n, -1}, {rig.last, 256, 5, 1, n, -1}}});
    rig.force(view, 1.0, 10.0);        // one fused launch
    judge("fused, pair", rig, out2, in2, n,
          {kBankedOne, 0, 256, 5, kByBank, kByBank, {},
           {{rig.banked, 256, 5, 1, n, -1}}});
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("stream routes: clean");
  return 0;
}
