// domain_boxes_main.cpp -- the partition a fused bordered domain counts its
// residual by (soda_hip_border_fused_residual_boxes) under a
// host sanitizer: this program with its own main against the library's
// sources, -fsanitize=address,undefined (`make domain_boxes_asan`); no GPU,
// nothing loaded into an interpreter.
//
// Hand-made plans of 2-D and 3-D programs; for every combination of border
// modes (walls, wrap, mixed), of reaches per dimension (symmetric, one-sided,
// none), of depths 1, 2 and 4 and of extents around N = L + H: the boxes lie
// in the padded arrays they index, and painted back on the domain they cover
// every cell exactly once.  Exit status 0 and "OK": all held.
#include "soda_hip.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond, ...)                         \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);          \
      std::fprintf(stderr, "\n");                 \
    }                                             \
  } while (0)

static soda_hip_plan_t* make_plan(int dim, int fused) {
  soda_hip_plan_t* p = new soda_hip_plan_t;
  std::memset(p, 0, sizeof *p);
  p->abi_version = SODA_HIP_ABI_VERSION;
  p->dim = dim;
  p->num_inputs = p->num_outputs = 1;
  p->elem_size[0] = p->elem_size[1] = 4;
  p->num_kernels = 2;               // a fused kernel and the one-iteration one
  for (int i = 0; i < 2; ++i) {
    soda_hip_kernel_desc_t* k = &p->kernels[i];
    std::snprintf(k->name, sizeof k->name, "k%d", i ? 1 : fused);
    k->block[0] = 64;
    k->block[1] = k->block[2] = 1;
    for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) k->tile[d] = d ? 1 : 64;
    k->vec = 1;
    k->window_extra = -1;
    k->twin = -1;
    p->passes[i].fused_iters = i ? 1 : fused;
    p->passes[i].num_kernels = 1;
    p->passes[i].kernel[0] = i;
  }
  p->num_passes = 2;
  return p;
}

struct Paint {
  int dim;
  int32_t n[4];
  std::vector<int> count;
  explicit Paint(int dim_, const int32_t* n_) : dim(dim_) {
    long cells = 1;
    for (int d = 0; d < 4; ++d) {
      n[d] = d < dim ? n_[d] : 1;
      cells *= n[d];
    }
    count.assign(cells, 0);
  }
  // [lo, hi) in domain coordinates
  void add(const int32_t* lo, const int32_t* hi) {
    int32_t l[4] = {0, 0, 0, 0}, h[4] = {1, 1, 1, 1};
    for (int d = 0; d < dim; ++d) {
      l[d] = lo[d];
      h[d] = hi[d];
      EXPECT(l[d] >= 0 && h[d] <= n[d], "a box leaves the domain: [%d, %d) of "
             "%d along %d", l[d], h[d], n[d], d);
      if (l[d] < 0 || h[d] > n[d]) return;
    }
    for (int32_t w = l[3]; w < h[3]; ++w)
      for (int32_t z = l[2]; z < h[2]; ++z)
        for (int32_t y = l[1]; y < h[1]; ++y)
          for (int32_t x = l[0]; x < h[0]; ++x)
            ++count[((((long)w * n[2] + z) * n[1] + y) * n[0]) + x];
  }
};

static long cases = 0;

static void check(const soda_hip_plan_t* plan, const int32_t* mode,
                  const int32_t* rlo, const int32_t* rhi, int depth,
                  const int32_t* extent) {
  const int dim = plan->dim;
  soda_hip_border_fused_desc_t desc;
  std::memset(&desc, 0, sizeof desc);
  desc.depth = depth;
  for (int d = 0; d < dim; ++d) {
    desc.border.domain.extent[d] = extent[d];
    desc.border.mode[d] = mode[d];
    const int times = mode[d] == SODA_HIP_BORDER_WRAP ? depth : 1;
    desc.border.domain.ghost_lo[d] = times * rlo[d];
    desc.border.domain.ghost_hi[d] = times * rhi[d];
    desc.reach_lo[d] = rlo[d];
    desc.reach_hi[d] = rhi[d];
  }
  soda_hip_border_fused_info_t info;
  soda_hip_border_fused_boxes_t boxes;
  const int rc = soda_hip_border_fused_plan(plan, &desc, 0, &info, 0, nullptr,
                                            nullptr);
  if (rc) {
    char why[256] = "";
    soda_hip_last_error(why, sizeof why);
    EXPECT(rc == 0, "plan refused (%d): %s", rc, why);
    return;
  }
  EXPECT(soda_hip_border_fused_residual_boxes(plan, &desc, &boxes) == 0,
         "boxes refused what the plan served");
  ++cases;
  EXPECT(boxes.depth == info.depth && boxes.num_strips == info.num_strips,
         "depth %d / %d, strips %d / %d", boxes.depth, info.depth,
         boxes.num_strips, info.num_strips);
  Paint paint(dim, extent);
  int32_t lo[4], hi[4];
  for (int d = 0; d < dim; ++d) {
    EXPECT(boxes.trusted_lo[d] >= 0 &&
               boxes.trusted_hi[d] <= info.main.padded[d],
           "the trusted box leaves the padded array along %d", d);
    lo[d] = boxes.trusted_lo[d] - info.main.ghost_lo[d];
    hi[d] = boxes.trusted_hi[d] - info.main.ghost_lo[d];
    const bool wall = mode[d] != SODA_HIP_BORDER_WRAP && info.depth > 1;
    EXPECT(lo[d] == (wall ? (info.depth - 1) * rlo[d] : 0) &&
               hi[d] == extent[d] - (wall ? (info.depth - 1) * rhi[d] : 0),
           "trusted [%d, %d) along %d", lo[d], hi[d], d);
  }
  paint.add(lo, hi);
  for (int i = 0; i < boxes.num_strips; ++i) {
    const soda_hip_border_strip_t& s = info.strip[i];
    const soda_hip_border_rims_t& r = boxes.strip[i];
    EXPECT(r.dim == s.dim, "strip %d: dimension %d / %d", i, r.dim, s.dim);
    for (int side = 0; side < 2; ++side) {
      bool empty = false;
      for (int d = 0; d < dim; ++d) {
        EXPECT(r.lo[side][d] >= 0 && r.hi[side][d] <= s.info.padded[d] &&
                   r.lo[side][d] <= r.hi[side][d],
               "a rim leaves the strip's padded array along %d", d);
        lo[d] = r.lo[side][d] - s.info.ghost_lo[d];
        hi[d] = r.hi[side][d] - s.info.ghost_lo[d];
        if (lo[d] == hi[d]) empty = true;
      }
      EXPECT(hi[s.dim] - lo[s.dim] == (side ? s.take_hi : s.take_lo),
             "a rim is not what the scatter takes");
      // the strip's high part sits at the domain's far wall
      const int32_t shift = side ? extent[s.dim] - (s.lo + s.hi) : 0;
      lo[s.dim] += shift;
      hi[s.dim] += shift;
      if (!empty) paint.add(lo, hi);
    }
  }
  long bad = 0;
  for (int c : paint.count) bad += c != 1;
  EXPECT(bad == 0, "%ld cells not counted exactly once (dim %d depth %d)", bad,
         dim, depth);
}

int main() {
  const int32_t kModes[3] = {SODA_HIP_BORDER_WRAP, SODA_HIP_BORDER_CLAMP,
                             SODA_HIP_BORDER_CONSTANT};
  const int32_t kReach[4][2] = {{1, 1}, {0, 2}, {2, 1}, {0, 0}};
  for (int dim = 2; dim <= 3; ++dim) {
    soda_hip_plan_t* plan = make_plan(dim, 4);
    int combos = 1;
    for (int d = 0; d < dim; ++d) combos *= 3 * 4;
    for (int c = 0; c < combos; ++c) {
      int32_t mode[4] = {0, 0, 0, 0}, rlo[4] = {0, 0, 0, 0},
              rhi[4] = {0, 0, 0, 0};
      int rest = c;
      for (int d = 0; d < dim; ++d) {
        mode[d] = kModes[rest % 3];
        rest /= 3;
        rlo[d] = kReach[rest % 4][0];
        rhi[d] = kReach[rest % 4][1];
        rest /= 4;
      }
      for (int depth : {1, 2, 4})
        for (int delta : {0, 3, -1}) {
          int32_t extent[4] = {1, 1, 1, 1};
          for (int d = 0; d < dim; ++d) {
            extent[d] = 2 * depth * (rlo[d] + rhi[d]) + delta + (d == 1);
            if (extent[d] < 1) extent[d] = 5;
          }
          check(plan, mode, rlo, rhi, depth, extent);
        }
    }
    delete plan;
  }
  // refusals: what the plan refuses, the boxes refuse, and write nothing
  soda_hip_plan_t* plan = make_plan(2, 4);
  soda_hip_border_fused_desc_t desc;
  std::memset(&desc, 0, sizeof desc);
  desc.border.domain.extent[0] = desc.border.domain.extent[1] = 20;
  desc.border.mode[0] = desc.border.mode[1] = SODA_HIP_BORDER_CLAMP;
  desc.reach_lo[0] = desc.reach_hi[0] = 1;      // ... and no frame for it
  soda_hip_border_fused_boxes_t boxes;
  std::memset(&boxes, 0x5a, sizeof boxes);
  EXPECT(soda_hip_border_fused_residual_boxes(plan, &desc, &boxes) != 0,
         "a frame below the reach was served");
  EXPECT(boxes.depth == 0x5a5a5a5a, "a refusal wrote the boxes");
  desc.depth = -1;
  EXPECT(soda_hip_border_fused_residual_boxes(plan, &desc, &boxes) != 0,
         "depth < 0 was served");
  EXPECT(soda_hip_border_fused_residual_boxes(plan, &desc, nullptr) != 0,
         "NULL boxes were served");
  EXPECT(soda_hip_border_fused_residual_boxes(nullptr, &desc, &boxes) != 0,
         "a NULL plan was served");
  delete plan;
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("OK domain boxes: %ld plans partitioned exactly\n", cases);
  return 0;
}
