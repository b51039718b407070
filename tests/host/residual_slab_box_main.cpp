// residual_slab_box_main.cpp -- the library's pure residual planning under a
// host sanitizer (tools/sanitize.sh builds this program with its own main
// against the library's sources, -fsanitize=address,undefined; no GPU, nothing
// loaded into an interpreter).
//
// A hand-made plan of a 5-point 2-D program with marching kernels and twins:
// for every number of slabs 1..7 (ragged row counts included), iterate 1..40
// and both border modes, the boxes soda_hip_plan_residual_slab_box gives the
// slabs are disjoint along the last dimension and their cells add up to the
// global box's; soda_hip_plan_launches_residual ends in the pass that takes
// the residual and keeps the multiset of depths.  Exit status 0: all held.
#include "soda_hip.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond, ...)                  \
  do {                                     \
    if (!(cond)) {                         \
      ++failures;                          \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);   \
      std::fprintf(stderr, "\n");          \
    }                                      \
  } while (0)

static void kernel(soda_hip_kernel_desc_t* k, const char* name, int twin,
                   int march) {
  std::memset(k, 0, sizeof *k);
  std::snprintf(k->name, sizeof k->name, "%s", name);
  k->block[0] = 64;
  k->block[1] = k->block[2] = 1;
  k->tile[0] = 248;
  k->tile[1] = 8;
  k->vec = 4;
  k->march_dim = march ? 2 : 0;
  k->waves_along = march ? 1 : 0;
  k->warm = march ? 2 : 0;
  k->window_extra = -1;
  k->chunk_fixed = 1;
  k->twin = twin;
}

static soda_hip_plan_t* make_plan(int whole) {
  soda_hip_plan_t* p = new soda_hip_plan_t;
  std::memset(p, 0, sizeof *p);
  p->abi_version = SODA_HIP_ABI_VERSION;
  p->dim = 2;
  p->num_inputs = p->num_outputs = 1;
  p->elem_size[0] = p->elem_size[1] = 4;
  p->num_kernels = 6;
  kernel(&p->kernels[0], "k4", 2, 1);
  kernel(&p->kernels[1], "k1", 3, 1);
  kernel(&p->kernels[2], "k4_rs", -1, 1);
  kernel(&p->kernels[3], "k1_rs", -1, 1);
  kernel(&p->kernels[4], "k_residual", -1, 0);
  kernel(&p->kernels[5], "k_residual_zero", -1, 0);
  p->num_passes = 2;
  p->passes[0].fused_iters = 4;
  p->passes[0].num_kernels = 1;
  p->passes[0].kernel[0] = 0;
  p->passes[1].fused_iters = 1;
  p->passes[1].num_kernels = 1;
  p->passes[1].kernel[0] = 1;
  p->has_reach = 1;
  p->reach_lo = p->reach_hi = 1;
  p->residual.present = 1;
  p->residual.kernel = 4;
  p->residual.zero_kernel = 5;
  p->residual.whole = whole;
  for (int o = 0; o < SODA_HIP_MAX_RES_PAIRS; ++o)
    for (int i = 0; i < SODA_HIP_MAX_RES_PAIRS; ++i)
      for (int d = 0; d < SODA_HIP_MAX_DIM; ++d)
        p->residual.dep_lo[o][i][d] = p->residual.dep_hi[o][i][d] =
            SODA_HIP_RES_NONE;
  for (int d = 0; d < 2; ++d) {
    p->residual.base_lo[0][d] = -1;
    p->residual.base_hi[0][d] = 1;
    p->residual.dep_lo[0][0][d] = -1;
    p->residual.dep_hi[0][0][d] = 1;
  }
  return p;
}

static void boxes(const soda_hip_plan_t* plan, int whole) {
  const int32_t gext[4] = {40, 121, 1, 1};
  for (int n = 1; n <= 7; ++n)
    for (int iterate = 1; iterate <= 40; iterate += iterate < 6 ? 1 : 7) {
      int32_t glo[2], ghi[2];
      EXPECT(soda_hip_plan_residual_box(plan, gext, iterate, glo, ghi) == 0,
             "global box");
      const long want = (long)(ghi[0] - glo[0]) * (ghi[1] - glo[1]);
      if (whole) EXPECT(want == 40L * 121, "whole: %ld", want);
      long sum = 0;
      int32_t prev_end = 0;
      const int base = gext[1] / n, extra = gext[1] % n;
      for (int s = 0; s < n; ++s) {
        const int own0 = s * base + std::min(s, extra);
        const int own1 = own0 + base + (s < extra ? 1 : 0);
        const int g0 = std::min(own0, 3), g1 = std::min(gext[1] - own1, 3);
        const int32_t origin[4] = {0, own0 - g0, 0, 0};
        const int32_t ext[4] = {40, own1 - own0 + g0 + g1, 1, 1};
        // exactly as many values as the function may write: the sanitizer
        // sees a store past num_outputs x dim
        std::vector<int32_t> lo(2), hi(2);
        EXPECT(soda_hip_plan_residual_slab_box(plan, gext, origin, ext, g0,
                                               g0 + own1 - own0, iterate,
                                               lo.data(), hi.data()) == 0,
               "slab box");
        EXPECT(0 <= lo[0] && lo[0] <= hi[0] && hi[0] <= ext[0], "dim 0");
        EXPECT(g0 <= lo[1] && lo[1] <= hi[1] && hi[1] <= g0 + own1 - own0,
               "kept rows: [%d, %d) of [%d, %d)", lo[1], hi[1], g0,
               g0 + own1 - own0);
        const long cells = (long)(hi[0] - lo[0]) * (hi[1] - lo[1]);
        if (cells) {
          EXPECT(lo[1] + origin[1] >= prev_end, "slabs overlap");
          prev_end = hi[1] + origin[1];
          EXPECT(lo[0] == glo[0] && hi[0] == ghi[0], "dim 0 of the box");
        }
        sum += cells;
      }
      EXPECT(sum == want, "n %d iterate %d: %ld cells, want %ld", n, iterate,
             sum, want);
    }
  // refusals
  int32_t lo[2], hi[2];
  const int32_t origin[4] = {0, 100, 0, 0}, ext[4] = {40, 30, 1, 1};
  EXPECT(soda_hip_plan_residual_slab_box(plan, gext, origin, ext, 0, 30, 1, lo,
                                         hi) == SODA_HIP_ERR_INVALID,
         "a slab outside the grid");
}

static void launches(const soda_hip_plan_t* plan) {
  const int32_t ext[4] = {520, 48, 1, 1};
  soda_hip_slab_run_t run;
  std::memset(&run, 0, sizeof run);
  run.keep_lo = 4;
  run.keep_hi = 44;
  run.reach_lo = run.reach_hi = 1;
  run.send_lo = run.send_hi = 4;
  run.sendable = &run;      // "given": never dereferenced by the planner
  for (int iterate = 1; iterate <= 13; ++iterate) {
    soda_hip_launch_info_t plain[16], res[16];
    int32_t np = 0, nr = 0, mode = 0;
    EXPECT(soda_hip_plan_launches(plan, ext, iterate, &run, 16, plain, &np) == 0,
           "plain launches");
    EXPECT(soda_hip_plan_launches_residual(plan, ext, iterate, &run, 16, res,
                                           &nr, &mode) == 0,
           "residual launches");
    EXPECT(np == nr && mode == 1, "iterate %d: %d / %d launches, mode %d",
           iterate, np, nr, mode);
    std::vector<int> a, b;
    for (int i = 0; i < np; ++i) a.push_back(plain[i].fused_iters);
    for (int i = 0; i < nr; ++i) b.push_back(res[i].fused_iters);
    std::sort(a.begin(), a.end());
    std::sort(b.begin(), b.end());
    EXPECT(a == b, "iterate %d: another multiset of depths", iterate);
    EXPECT(nr > 0 && res[nr - 1].fused_iters == b.back() &&
               res[nr - 1].record == 1,
           "iterate %d: the deepest pass goes last", iterate);
    // backwards: every pass covers what the passes behind it read
    int32_t need_lo = run.keep_lo, need_hi = run.keep_hi;
    for (int i = nr - 1; i >= 0; --i) {
      need_lo = std::max(0, need_lo - res[i].fused_iters * run.reach_lo);
      need_hi = std::min(ext[1], need_hi + res[i].fused_iters * run.reach_hi);
      EXPECT(res[i].lo == need_lo && res[i].hi == need_hi,
             "iterate %d launch %d: rows [%d, %d), want [%d, %d)", iterate, i,
             res[i].lo, res[i].hi, need_lo, need_hi);
    }
  }
}

int main() {
  for (int whole = 0; whole < 2; ++whole) {
    soda_hip_plan_t* plan = make_plan(whole);
    boxes(plan, whole);
    launches(plan);
    delete plan;
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("residual slab planning: clean");
  return 0;
}
