// run_checks_main.cpp -- what a run asks of the caller's addresses
// (check_run_tensors, soda_internal.h: the overlap and alignment rules of the
// device entries) on the CPU, under a host sanitizer: a program with its own
// main built against the library's sources, -fsanitize=address,undefined; no
// GPU, nothing loaded into an interpreter.
//
// A hand-made plan -- 2 inputs, 2 outputs, 1 param array of 9 cells, one
// kernel -- on an extent of 64 x 40.  The addresses are integers cast to
// pointers; the check looks at them and never behind them.  Every layout is
// judged twice: as dense tensors (status and text as stated) and as the banks
// of a wire stream (bank_tensors: nothing is asked).  Exit status 0: all held.
#include "soda_internal.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

using soda_detail::check_run_tensors;

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

static const int64_t kCells = 64 * 40;
static const uintptr_t kBase = 0x40000000;   // 16-byte aligned, never read

static soda_hip_plan_t* make_plan(int32_t elem, int32_t vec) {
  soda_hip_plan_t* p = new soda_hip_plan_t;
  std::memset(p, 0, sizeof *p);
  p->abi_version = SODA_HIP_ABI_VERSION;
  p->dim = 2;
  p->num_inputs = p->num_outputs = 2;
  p->num_params = 1;
  for (int t = 0; t < 5; ++t) p->elem_size[t] = elem;   // in, in, out, out, prm
  p->param_elems[0] = 9;
  p->num_kernels = 1;
  p->kernels[0].vec = vec;
  return p;
}

// where the five arrays start
struct Layout {
  uintptr_t in0, in1, out0, out1, prm;
};

struct Case {
  const char* name;
  Layout at;
  int32_t elem, vec, batch;
  const char* refused;   // null: passes; else a fragment of the refusal
};

static std::string last_error() {
  char buf[512];
  soda_hip_last_error(buf, sizeof buf);
  return buf;
}

static void judge(const Case& c) {
  soda_hip_plan_t* plan = make_plan(c.elem, c.vec);
  void* const outputs[2] = {reinterpret_cast<void*>(c.at.out0),
                            reinterpret_cast<void*>(c.at.out1)};
  const void* const inputs[3] = {reinterpret_cast<const void*>(c.at.in0),
                                 reinterpret_cast<const void*>(c.at.in1),
                                 reinterpret_cast<const void*>(c.at.prm)};
  const int rc = check_run_tensors(*plan, false, outputs, inputs, kCells,
                                   c.batch);
  if (!c.refused) {
    EXPECT(rc == SODA_HIP_OK, "%s: refused: %s", c.name, last_error().c_str());
  } else {
    const std::string text = last_error();
    const std::string tail = "nothing was launched";
    EXPECT(rc == SODA_HIP_ERR_INVALID, "%s: status %d", c.name, rc);
    EXPECT(text.find(c.refused) != std::string::npos, "%s: `%s` not in `%s`",
           c.name, c.refused, text.c_str());
    EXPECT(text.size() >= tail.size() &&
               text.compare(text.size() - tail.size(), tail.size(), tail) == 0,
           "%s: `%s` does not end in `%s`", c.name, text.c_str(),
           tail.c_str());
  }
  // banks of a wire stream: any address, any length -- the stream layer checks
  EXPECT(check_run_tensors(*plan, true, outputs, inputs, kCells, c.batch) ==
             SODA_HIP_OK,
         "%s: refused as bank tensors: %s", c.name, last_error().c_str());
  delete plan;
}

int main() {
  const uintptr_t B = kBase;
  const uintptr_t N = kCells * 4;    // bytes of a tensor of 4-byte cells
  const uintptr_t far = B + 100 * N;
  // apart: two tensors' worth of room each -- two items fit, three do not;
  // wide: four tensors' worth (8-byte cells fit, moved a little as well)
  const Layout apart = {B, B + 2 * N, B + 4 * N, B + 6 * N, far};
  const Layout wide = {B, B + 4 * N, B + 8 * N, B + 12 * N, far};
  Layout misaligned_in = wide, misaligned_in2 = wide, in_at_8 = wide,
         in_at_16 = wide, prm_at_4 = wide, prm_at_2 = wide;
  misaligned_in.in1 += 4;
  misaligned_in2.in1 += 2;
  in_at_8.in1 += 8;
  in_at_16.in1 += 16;
  prm_at_4.prm += 4;
  prm_at_2.prm += 2;
  const Case cases[] = {
      // ---- overlap --------------------------------------------------------
      {"back to back, no byte shared",
       {B, B + N, B + 2 * N, B + 3 * N, B + 4 * N}, 4, 4, 1, nullptr},
      {"output equals input", {B, B + N, B, B + 3 * N, far}, 4, 4, 1,
       "aliases an input"},
      {"output begins on the input's last byte",
       {B, B + 5 * N, B + N - 1, B + 3 * N, far}, 4, 4, 1,
       "overlaps an input"},
      {"output's last byte is the param array's first",
       {B, B + N, B + 2 * N, B + 3 * N, B + 4 * N - 1}, 4, 4, 1,
       "overlaps a param array"},
      {"two outputs one byte into each other",
       {B, B + N, B + 2 * N, B + 3 * N - 1, far}, 4, 4, 1,
       "two outputs overlap"},
      {"two tensors' room, one item", apart, 4, 4, 1, nullptr},
      {"two tensors' room, two items", apart, 4, 4, 2, nullptr},
      {"two tensors' room, three items", apart, 4, 4, 3, "overlaps an input"},
      // ---- alignment ------------------------------------------------------
      {"input at + 4, four cells per lane", misaligned_in, 4, 4, 1,
       "input 1 at 0x4000a004 is not aligned to 16 bytes"},
      {"input at + 4, one cell per lane", misaligned_in, 4, 1, 1, nullptr},
      {"input at + 2, one cell per lane", misaligned_in2, 4, 1, 1,
       "is not aligned to 4 bytes"},
      {"8-byte cells, input at + 16: the demand stops at 16", in_at_16, 8, 4, 1,
       nullptr},
      {"8-byte cells, input at + 8", in_at_8, 8, 4, 1,
       "is not aligned to 16 bytes"},
      {"param array at + 4: its own cell size", prm_at_4, 4, 4, 1, nullptr},
      {"param array at + 2", prm_at_2, 4, 4, 1,
       "param array 0 at 0x400fa002 is not aligned to 4 bytes"},
  };
  for (const Case& c : cases) judge(c);
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("run tensor checks: clean");
  return 0;
}
