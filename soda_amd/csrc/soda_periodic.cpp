// soda_periodic.cpp -- periodic domains: a program on a torus (DESIGN.md 4.11,
// include/soda_hip.h soda_hip_periodic_*).  A handle over an existing program
// keeps the state in padded arrays, advances it k iterations at a time through
// the program's ordinary run path on the padded extent (run_core) and refills
// the ghost frame in between with the wrap kernel (soda_rt_wrap.h), which also
// pads the dense entry's inputs and crops its outputs.  The program, its
// module and its plan know nothing of this.
//
// Bordered domains (soda_hip_border_*) are the same handle
// with another rule for the ghost frame: a mode per dimension and a constant
// per tensor, the extend kernel (soda_rt_extend.h) in the wrap kernel's place,
// one iteration between refills unless every mode wraps.  Everything below is
// written once for both, told apart by a Kind.
//
// Fused bordered domains (soda_hip_border_fused_*) put such
// handles together: one on the domain, whose chunks run fused, and one per
// wall dimension on a narrow strip, which runs the loop above and mends the
// rim; the box kernel (soda_rt_box.h) carries cells between them.
//
// Residual, norms and run_until on all three: the last chunk
// of a run takes the residual through run_core with the interior as its box;
// a fused handle counts each cell where it is made right -- the interior run
// a trusted box, every strip its two rims.
//
// Batched domains (soda_hip_periodic_create_batch,
// soda_hip_border_create_batch): the same handle over a batched program, fixed
// to one (extent, batch).  Every array is `batch` items one behind the other;
// the batch is a field of the frame, one more launch dimension of the helper
// kernels (their `_bt` forms) and the `batch` of the chunks' RunRequest.
//
// Top to bottom: the helper kernels' launchers and loader, planning, the two
// handle structs, the chunk loop, the run cores, the exported entries.
#include "soda_internal.h"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

using namespace soda_detail;

namespace {

// -- the helper kernels: their arguments, their launches, their modules ------

const int kHelperBlock = 256;
const int kWrapMaxRegions = 5;
const int kBoxMax = 4;
const int64_t kHelperMaxBlocks = 1 << 15;   // the lanes stride over the items

// the wrap kernel's one argument, as soda_rt_wrap.h declares it
struct WrapArgs {
  void* dst[16];
  const void* src[16];
  int32_t dext[4];
  int32_t sext[4];
  int32_t n[4];
  int32_t sub[4];
  int32_t add[4];
  int32_t glo[4];
  int32_t nreg;
  int32_t level[kWrapMaxRegions];
  uint32_t per_row[kWrapMaxRegions];
  uint32_t ends[kWrapMaxRegions];
  uint32_t reserved;
  uint64_t start[kWrapMaxRegions];
  uint64_t total;
};

// the extend kernel's (soda_rt_extend.h): the same block, then the border
struct ExtendArgs {
  WrapArgs w;
  int32_t mode[4];
  uint64_t constant[16];
};

// the faces kernel's (soda_rt_faces.h): the same block, then
// a mode per face and, per tensor, a constant per face
struct FacesArgs {
  WrapArgs w;
  int32_t mode_lo[4];
  int32_t mode_hi[4];
  uint64_t constant[16][4][2];
};

// a batched wrap, extend or faces kernel's (soda_rt_domain_batch.h): its
// unbatched block, then the cells from an item to the next in the destination
// and in the source.  Room for the steps behind any of the blocks, which all
// begin with the wrap kernel's
struct DomainArgs {
  union {
    ExtendArgs e;
    FacesArgs f;
  };
  uint64_t steps[2];
};
// (the kernels' struct puts the steps at the block's size: no padding)
static_assert(sizeof(WrapArgs) % alignof(uint64_t) == 0 &&
                  sizeof(ExtendArgs) % alignof(uint64_t) == 0 &&
                  sizeof(FacesArgs) % alignof(uint64_t) == 0 &&
                  sizeof(ExtendArgs) <= sizeof(FacesArgs) &&
                  offsetof(DomainArgs, steps) == sizeof(FacesArgs),
              "the item steps lie right behind any block");

// the box kernel's one argument, as soda_rt_box.h declares it
struct BoxArgs {
  void* dst[16];
  const void* src[16];
  int32_t dext[4];
  int32_t sext[4];
  int32_t nbox;
  uint32_t reserved;
  int32_t dorg[kBoxMax][4];
  int32_t sorg[kBoxMax][4];
  int32_t size[kBoxMax][4];
  uint32_t per_row[kBoxMax];
  uint64_t start[kBoxMax];
  uint64_t total;
};

struct Box {
  int32_t to[4], from[4], size[4];
};

enum WrapJob { kFill, kPad, kCrop };

// what tells a torus from a bordered domain: the names in messages, the kernel
struct Kind {
  const char* who;
  const char* domain;
  const char* kernel;
  bool extend;
};
const Kind kTorus = {"periodic", "a torus", "soda_wrap", false};
const Kind kBorder = {"border", "a bordered domain", "soda_extend", true};

struct Torus {
  int dim;
  int32_t n[4], glo[4], ghi[4], p[4];
};

// the modules and kernels of one helper (wrap or extend, box), by log2(elem)
struct Helpers {
  hipModule_t module[4] = {nullptr, nullptr, nullptr, nullptr};
  hipFunction_t fn[4] = {nullptr, nullptr, nullptr, nullptr};
};

// what a wrap launch needs of a handle: the frame and the rule that fills it
struct Frame {
  const Kind* kind = &kTorus;
  int32_t mode[4] = {0, 0, 0, 0};      // kBorder: SODA_HIP_BORDER_* ...
  uint64_t constant[SODA_HIP_MAX_TENSORS] = {};   // ... and per input
  // kBorder, a request whose faces differ: `mode` the low
  // faces, these the high ones and the constants per input, dimension, side
  bool faces = false;
  int32_t mode_hi[4] = {0, 0, 0, 0};
  uint64_t face_constant[SODA_HIP_MAX_TENSORS][4][2] = {};
  Torus t;
  Helpers wrap;                        // the wrap, the extend or (`faces`)
                                       // the faces kernels
  int32_t batch = 0;                   // > 0: a batched handle, every array
                                       // that many items, `wrap` the _bt
                                       // kernels
  int32_t items() const { return batch ? batch : 1; }
};

int log2_elem(int elem) {
  return elem == 1 ? 0 : elem == 2 ? 1 : elem == 4 ? 2 : elem == 8 ? 3 : -1;
}

int64_t cells_of(const int32_t* e, int dim) {
  int64_t c = 1;
  for (int d = 0; d < dim; ++d) c *= e[d];
  return c;
}

int32_t plan_vec(const soda_hip_plan_t& plan) {
  int32_t vec = 1;
  for (int k = 0; k < plan.num_kernels; ++k)
    if (plan.kernels[k].vec > vec) vec = plan.kernels[k].vec;
  return vec;
}

// The regions of a job on cells of `elem` bytes (soda_rt_wrap.h); false if a
// region has 2^31 rows or more (the kernel counts rows in 32 bits).
bool wrap_regions(const Torus& t, WrapJob job, int elem, WrapArgs* a) {
  const int dim = t.dim, v = 16 / elem;
  for (int d = 0; d < 4; ++d) {
    const bool in = d < dim;
    a->n[d] = in ? t.n[d] : 1;
    a->glo[d] = in ? t.glo[d] : 0;
    a->dext[d] = in ? (job == kCrop ? t.n[d] : t.p[d]) : 1;
    a->sext[d] = in ? (job == kPad ? t.n[d] : t.p[d]) : 1;
    a->sub[d] = in && job != kCrop ? t.glo[d] : 0;
    a->add[d] = in && job != kPad ? t.glo[d] : 0;
  }
  a->nreg = 0;
  a->total = 0;
  auto add = [&](int level, int64_t rows, int64_t per_row, bool ends) {
    if (rows < 1 || per_row < 1) return true;     // an empty region
    if (rows > 0x7fffffffLL || per_row > 0x7fffffffLL) return false;
    const int k = a->nreg++;
    a->level[k] = level;
    a->per_row[k] = (uint32_t)per_row;
    a->ends[k] = ends ? 1u : 0u;
    a->start[k] = a->total;
    a->total += (uint64_t)rows * (uint64_t)per_row;
    return true;
  };
  // fragments a whole row may need: it starts up to v - 1 cells behind a
  // 16-byte boundary
  const int64_t frags = ((int64_t)a->dext[0] + 2 * v - 2) / v;
  if (job != kFill) {
    int64_t rows = 1;
    for (int d = 1; d < dim; ++d) rows *= a->dext[d];
    return add(dim, rows, frags, false);
  }
  // fill: the rows with dimension `level` in the ghost frame, the dimensions
  // above it inside the torus, those below it anywhere -- every ghost row
  // exactly once -- and the two ends of the rows inside the torus
  for (int level = dim - 1; level >= 1; --level) {
    int64_t rows = t.p[level] - t.n[level];
    for (int d = 1; d < dim; ++d)
      if (d != level) rows *= d < level ? t.p[d] : t.n[d];
    if (!add(level, rows, frags, false)) return false;
  }
  int64_t inner = 1;
  for (int d = 1; d < dim; ++d) inner *= t.n[d];
  return add(0, inner, (int64_t)t.glo[0] + t.ghi[0], true);
}

// One launch of a helper kernel per cell size among `count` tensors with cells
// of elem[i] bytes.  `prepare(size, tensor, m, &args, &total)` fills the
// kernel's argument for the `m` tensors tensor[0..m) of that size and says
// how many items the launch has (0: none, it is skipped), or refuses.  `bytes`
// of `args` reach the kernel; `batch` is the grid's z: the domains of a
// batched handle, 1 elsewhere.
template <class Args, class Prepare>
int launch_by_size(const Helpers& kernels, const char* who, const char* what,
                   const int32_t* elem, int count, size_t bytes, int32_t batch,
                   hipStream_t stream, Prepare prepare) {
  for (int size = 1; size <= 8; size *= 2) {
    int tensor[16], m = 0;
    for (int i = 0; i < count; ++i)
      if (elem[i] == size) tensor[m++] = i;
    if (!m) continue;
    Args args;
    memset(&args, 0, sizeof args);
    uint64_t total = 0;
    if (int rc = prepare(size, tensor, m, &args, &total)) return rc;
    if (!total) continue;
    hipFunction_t fn = kernels.fn[log2_elem(size)];
    if (!fn)
      return fail(SODA_HIP_ERR_INVALID,
                  std::string(who) + ": no " + what + " kernel");
    int64_t blocks = (int64_t)((total + kHelperBlock - 1) / kHelperBlock);
    if (blocks > kHelperMaxBlocks) blocks = kHelperMaxBlocks;
    void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &args,
                     HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes,
                     HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(fn, (unsigned)blocks, (unsigned)m,
                                  (unsigned)batch, kHelperBlock, 1, 1, 0,
                                  stream, nullptr, extra));
  }
  return SODA_HIP_OK;
}

// One job on `count` tensors: dst[i] / src[i] with cells of elem[i] bytes (a
// bordered domain: and the constant of input i); one launch per cell size
// among them (no ghost cells: nothing to fill, no launch).  A batched handle:
// the job on every item of the arrays, in the same launches.
int wrap_launch(const Frame& f, WrapJob job, void* const* dst,
                const void* const* src, const int32_t* elem, int count,
                hipStream_t stream) {
  // the wrap kernel takes the block without the border behind it, a batched
  // kernel the item steps behind its block
  const size_t block = f.faces          ? sizeof(FacesArgs)
                       : f.kind->extend ? sizeof(ExtendArgs)
                                        : sizeof(WrapArgs);
  const uint64_t padded = (uint64_t)cells_of(f.t.p, f.t.dim);
  const uint64_t dense = (uint64_t)cells_of(f.t.n, f.t.dim);
  const uint64_t steps[2] = {job == kCrop ? dense : padded,
                             job == kPad ? dense : padded};
  return launch_by_size<DomainArgs>(
      f.wrap, f.kind->who, "wrap", elem, count,
      block + (f.batch ? sizeof steps : 0), f.items(), stream,
      [&](int size, const int* tensor, int m, DomainArgs* all,
          uint64_t* total) -> int {
        ExtendArgs* args = &all->e;
        if (f.faces) {      // the same block, the faces kernel's border behind
          FacesArgs* fa = &all->f;
          for (int j = 0; j < m; ++j) {
            fa->w.dst[j] = dst[tensor[j]];
            fa->w.src[j] = src[tensor[j]];
            memcpy(fa->constant[j], f.face_constant[tensor[j]],
                   sizeof fa->constant[j]);
          }
          for (int d = 0; d < 4; ++d) {
            fa->mode_lo[d] = f.mode[d];
            fa->mode_hi[d] = f.mode_hi[d];
          }
        } else {
          for (int j = 0; j < m; ++j) {
            args->w.dst[j] = dst[tensor[j]];
            args->w.src[j] = src[tensor[j]];
            args->constant[j] = f.constant[tensor[j]];
          }
          for (int d = 0; d < 4; ++d) args->mode[d] = f.mode[d];
        }
        if (!wrap_regions(f.t, job, size, &args->w))
          return fail(SODA_HIP_ERR_INVALID,
                      std::string(f.kind->who) +
                          ": 2^31 rows or more; nothing was launched");
        if (f.batch)      // (behind the wrap kernel's block: over the border)
          memcpy(reinterpret_cast<char*>(all) + block, steps, sizeof steps);
        *total = args->w.total;
        return SODA_HIP_OK;
      });
}

// `nbox` boxes from the arrays src[i] of extent `sext` into dst[i] of `dext`,
// `count` tensors with cells of elem[i] bytes; one launch per cell size among
// them.  A box that leaves either extent is refused before anything runs.
int box_launch(const Helpers& kernels, void* const* dst, const int32_t* dext,
               const void* const* src, const int32_t* sext,
               const int32_t* elem, int count, const Box* boxes, int nbox,
               int dim, hipStream_t stream) {
  for (int b = 0; b < nbox; ++b)
    for (int d = 0; d < dim; ++d) {
      const Box& x = boxes[b];
      if (x.size[d] < 0 || x.to[d] < 0 || x.from[d] < 0 ||
          (int64_t)x.to[d] + x.size[d] > dext[d] ||
          (int64_t)x.from[d] + x.size[d] > sext[d])
        return fail(SODA_HIP_ERR_INVALID,
                    "border_fused: a box leaves its array; nothing was "
                    "launched");
    }
  return launch_by_size<BoxArgs>(
      kernels, "border_fused", "box", elem, count, sizeof(BoxArgs), 1, stream,
      [&](int size, const int* tensor, int m, BoxArgs* a,
          uint64_t* total) -> int {
        for (int j = 0; j < m; ++j) {
          a->dst[j] = dst[tensor[j]];
          a->src[j] = src[tensor[j]];
        }
        const int v = 16 / size;
        for (int d = 0; d < 4; ++d) {
          a->dext[d] = d < dim ? dext[d] : 1;
          a->sext[d] = d < dim ? sext[d] : 1;
        }
        for (int b = 0; b < nbox && a->nbox < kBoxMax; ++b) {
          int64_t rows = 1;
          bool empty = false;
          for (int d = 0; d < dim; ++d) {
            if (boxes[b].size[d] < 1) empty = true;
            if (d) rows *= boxes[b].size[d];
          }
          if (empty) continue;
          if (rows > 0x7fffffffLL)
            return fail(SODA_HIP_ERR_INVALID,
                        "border_fused: 2^31 rows or more; nothing was "
                        "launched");
          const int k = a->nbox++;
          for (int d = 0; d < 4; ++d) {
            a->dorg[k][d] = d < dim ? boxes[b].to[d] : 0;
            a->sorg[k][d] = d < dim ? boxes[b].from[d] : 0;
            a->size[k][d] = d < dim ? boxes[b].size[d] : 1;
          }
          // fragments a row may need: it starts up to v - 1 cells behind a
          // 16-byte boundary
          a->per_row[k] =
              (uint32_t)(((int64_t)boxes[b].size[0] + 2 * v - 2) / v);
          a->start[k] = a->total;
          a->total += (uint64_t)rows * a->per_row[k];
        }
        *total = a->total;
        return SODA_HIP_OK;
      });
}

// need[l]: cells of 1 << l bytes are among the program's inputs and outputs.
// Refuses any other cell size, and a needed size whose `what` module is not
// in `code`.
int helpers_needed(const soda_hip_plan_t& plan, const void* const* code,
                   const size_t* code_size, const std::string& who,
                   const char* what, bool need[4]) {
  for (int s = 0; s < plan.num_inputs + plan.num_outputs; ++s) {
    const int l = log2_elem(plan.elem_size[s]);
    if (l < 0)
      return fail(SODA_HIP_ERR_UNSUPPORTED,
                  who + ": cells of 1, 2, 4 or 8 bytes only");
    need[l] = true;
  }
  for (int l = 0; l < 4; ++l)
    if (need[l] && (!code[l] || !code_size[l]))
      return fail(SODA_HIP_ERR_INVALID,
                  who + "_create: the " + what + " module of a cell size of "
                        "the program is missing");
  return SODA_HIP_OK;
}

// The module of every needed cell size loaded from `code`, and its kernel
// `<kernel>_e<bytes>_d<dim>` looked up (`batch`: `..._bt`, the batched one).
int load_helpers(Helpers* out, const bool need[4], const void* const* code,
                 const char* kernel, int dim, const std::string& who,
                 const char* what, bool batch = false) {
  for (int l = 0; l < 4; ++l) {
    if (!need[l]) continue;
    hipError_t e = hipModuleLoadData(&out->module[l], code[l]);
    if (e != hipSuccess)
      return hip_fail(e, (who + "_create: hipModuleLoadData").c_str());
    char name[64];
    snprintf(name, sizeof name, "%s_e%d_d%d%s", kernel, 1 << l, dim,
             batch ? "_bt" : "");
    e = hipModuleGetFunction(&out->fn[l], out->module[l], name);
    if (e != hipSuccess)
      return hip_fail(e, (who + "_create: hipModuleGetFunction (is this the " +
                          (batch ? "batched " : "") + what +
                          " module of the cell size and dimension "
                          "count?)").c_str());
  }
  return SODA_HIP_OK;
}

void unload_helpers(Helpers* h) {
  for (auto& m : h->module)
    if (m) (void)hipModuleUnload(m);
}

// -- planning: no GPU ---------------------------------------------------------

bool can_iterate(const soda_hip_plan_t& plan, bool not_iterable) {
  if (not_iterable || plan.num_inputs != plan.num_outputs) return false;
  for (int i = 0; i < plan.num_inputs; ++i)
    if (plan.elem_size[i] != plan.elem_size[plan.num_inputs + i]) return false;
  return true;
}

int check_iterate(const soda_hip_plan_t& plan, bool not_iterable,
                  int32_t iterate, const char* who) {
  if (iterate < 1)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": cannot iterate < 1 times; nothing was "
                                   "launched");
  if (iterate > 1 && !can_iterate(plan, not_iterable))
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": the program cannot iterate (it needs as "
                                   "many outputs as inputs, of the same "
                                   "types) and iterate > 1; nothing was "
                                   "launched");
  return SODA_HIP_OK;
}

// the deepest fusion of the plan's passes: the default chunk of a handle
int32_t deepest_pass(const soda_hip_plan_t& plan) {
  int32_t deepest = 0;
  for (int i = 0; i < plan.num_passes; ++i)
    if (plan.passes[i].fused_iters > deepest)
      deepest = plan.passes[i].fused_iters;
  return deepest;
}

// the iterations of the next chunk of a run with `left` to go, `k` at most
int32_t chunk_len(int32_t left, int32_t k) { return left < k ? left : k; }

// a plan entry's answer: the chunks of a run of `iterate` in chunks of `k`
void list_chunks(int32_t iterate, int32_t k, int32_t capacity, int32_t* chunks,
                 int32_t* count) {
  int32_t n = 0;
  for (int32_t left = iterate; left > 0; left -= k, ++n)
    if (chunks && n < capacity) chunks[n] = chunk_len(left, k);
  if (count) *count = n;
}

// a handle's batch as the _batch entries take it: 1..SODA_HIP_MAX_BATCH, over
// a batched plan only -- never a loop of launches in its place
int check_domain_batch(const soda_hip_plan_t& plan, int32_t batch,
                       const std::string& who) {
  if (batch < 1 || batch > SODA_HIP_MAX_BATCH) {
    char buf[160];
    snprintf(buf, sizeof buf, ": batch = %d, must be 1 to %d (the grid's z "
             "dimension); nothing was launched", batch, SODA_HIP_MAX_BATCH);
    return fail(SODA_HIP_ERR_INVALID, who + buf);
  }
  if (!plan.batched)
    return fail(SODA_HIP_ERR_INVALID,
                who + ": the program's kernels are not batched (build it with "
                      "LowerOptions.batch / sodac --hip-batch); nothing was "
                      "launched");
  return SODA_HIP_OK;
}

// soda_hip_periodic_plan, and soda_hip_border_plan behind its modes; `batch`
// > 0: their _batch forms, the batch checked by check_domain_batch (0: the
// unbatched entries, which refuse a batched plan)
int plan_core(const Kind& kind, const soda_hip_plan_t* plan,
              const soda_hip_periodic_desc_t* desc, int32_t iterate,
              soda_hip_periodic_info_t* info, int32_t capacity,
              int32_t* chunks, int32_t* count, int32_t batch = 0) {
  const std::string who(kind.who);
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, who + "_plan: NULL argument");
  if (plan->abi_version != SODA_HIP_ABI_VERSION || plan->dim < 1 ||
      plan->dim > SODA_HIP_MAX_DIM || plan->num_passes < 1 ||
      plan->num_passes > SODA_HIP_MAX_PASSES)
    return fail(SODA_HIP_ERR_INVALID, who + "_plan: bad plan");
  if (desc->preserve || (plan->residual.present && plan->residual.whole))
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                who + ": a program with `border: preserve` pins its border, "
                      "and " + kind.domain + " has none; nothing was launched");
  if (plan->batched && !batch)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                who + ": batched plans are not served on " + kind.domain +
                    "; nothing was launched");
  const int dim = plan->dim;
  int32_t k = desc->refill_every;
  if (k < 0)
    return fail(SODA_HIP_ERR_INVALID, who + ": refill_every < 0");
  if (k == 0) k = deepest_pass(*plan);
  if (k < 1) return fail(SODA_HIP_ERR_INVALID, who + ": bad plan");
  soda_hip_periodic_info_t out;
  memset(&out, 0, sizeof out);
  out.refill_every = k;
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) out.padded[d] = 1;
  for (int d = 0; d < dim; ++d) {
    if (desc->extent[d] < 1 || desc->ghost_lo[d] < 0 || desc->ghost_hi[d] < 0)
      return fail(SODA_HIP_ERR_INVALID,
                  who + ": extent < 1 or a negative ghost width; nothing was "
                        "launched");
    out.ghost_lo[d] = desc->ghost_lo[d];
    out.ghost_hi[d] = desc->ghost_hi[d];
  }
  if (plan->has_reach) {
    const int ax = dim - 1;
    if ((int64_t)out.ghost_lo[ax] < (int64_t)k * plan->reach_lo ||
        (int64_t)out.ghost_hi[ax] < (int64_t)k * plan->reach_hi) {
      char buf[256];
      snprintf(buf, sizeof buf,
               "%s: ghosts of %d / %d cells along the last dimension, "
               "%d iterations between refills reach %d / %d; nothing was "
               "launched", kind.who, out.ghost_lo[ax], out.ghost_hi[ax], k,
               k * plan->reach_lo, k * plan->reach_hi);
      return fail(SODA_HIP_ERR_INVALID, buf);
    }
  }
  const int32_t vec = plan_vec(*plan);
  int64_t cells = 1;
  for (int d = 0; d < dim; ++d) {
    int64_t p = (int64_t)out.ghost_lo[d] + desc->extent[d] + out.ghost_hi[d];
    if (d == 0 && p % vec) {
      out.ghost_hi[0] += (int32_t)(vec - p % vec);
      p += vec - p % vec;
    }
    if (p > 0x7fffffffLL)
      return fail(SODA_HIP_ERR_INVALID, who + ": padded extent overflows");
    out.padded[d] = (int32_t)p;
    cells *= p;
  }
  if (iterate < 0) return fail(SODA_HIP_ERR_INVALID, who + ": iterate < 0");
  if (iterate > 1)
    if (int rc = check_iterate(*plan, desc->not_iterable != 0, iterate,
                               kind.who))
      return rc;
  // what the kernels ask of the padded extent: row length, max_extent0, the
  // 1 GiB window of a plane (of an item's)
  if (int rc = batch ? soda_hip_plan_geometry_batch(plan, out.padded, batch,
                                                    nullptr, nullptr)
                     : soda_hip_plan_geometry(plan, out.padded, nullptr,
                                              nullptr))
    return rc;
  const int nin = plan->num_inputs, nout = plan->num_outputs;
  for (int i = 0; i < nin; ++i)
    out.scratch_bytes += cells * plan->elem_size[i];
  for (int o = 0; o < nout; ++o)
    out.scratch_bytes +=
        cells * plan->elem_size[nin + o] *
        (can_iterate(*plan, desc->not_iterable != 0) ? 2 : 1);
  if (batch) out.scratch_bytes *= batch;
  if (info) *info = out;
  list_chunks(iterate, k, capacity, chunks, count);
  return SODA_HIP_OK;
}

// Whether every mode of a bordered request wraps; its modes checked.
int border_modes(const soda_hip_plan_t* plan,
                 const soda_hip_border_desc_t* desc, bool* all_wrap) {
  *all_wrap = true;
  const int dim = plan->dim < 0                  ? 0
                  : plan->dim > SODA_HIP_MAX_DIM ? SODA_HIP_MAX_DIM
                                                 : plan->dim;
  for (int d = 0; d < dim; ++d) {
    if (desc->mode[d] < SODA_HIP_BORDER_WRAP ||
        desc->mode[d] > SODA_HIP_BORDER_CONSTANT)
      return fail(SODA_HIP_ERR_INVALID,
                  "border: a mode that is none of SODA_HIP_BORDER_*; nothing "
                  "was launched");
    if (desc->mode[d] != SODA_HIP_BORDER_WRAP) *all_wrap = false;
  }
  if (!*all_wrap && desc->domain.refill_every > 1)
    return fail(SODA_HIP_ERR_INVALID,
                "border: only a wrapped ghost evolves with its interior: with "
                "any other mode the frame is refilled after every iteration "
                "(refill_every 0 or 1); nothing was launched");
  return SODA_HIP_OK;
}

// A bordered request with its faces resolved.
struct FaceRule {
  bool asymmetric;          // a pair of faces or a tensor's constants differ
  int32_t mode_hi[4];
  uint64_t constant[SODA_HIP_MAX_TENSORS][4][2];
  // the request of soda_hip_border_*: the low faces as its modes, per input
  // the constant of dimension 0's low face.  A symmetric request IS this one;
  // an asymmetric one has its geometry (the same wall dimensions)
  soda_hip_border_desc_t low;
};

// The faces of a request checked and resolved; `faces` NULL: the desc's own.
int border_faces(const soda_hip_plan_t* plan,
                 const soda_hip_border_desc_t* desc,
                 const soda_hip_border_faces_t* faces, FaceRule* out) {
  memset(out, 0, sizeof *out);
  out->low = *desc;
  const int dim = plan->dim < 0                  ? 0
                  : plan->dim > SODA_HIP_MAX_DIM ? SODA_HIP_MAX_DIM
                                                 : plan->dim;
  const int nin = plan->num_inputs < 0 ? 0
                  : plan->num_inputs > SODA_HIP_MAX_TENSORS
                      ? SODA_HIP_MAX_TENSORS
                      : plan->num_inputs;
  bool all_wrap = true;
  for (int d = 0; d < dim; ++d) {
    const int32_t lo = desc->mode[d], hi = faces ? faces->mode_hi[d] : lo;
    if (lo < SODA_HIP_BORDER_WRAP || lo > SODA_HIP_BORDER_CONSTANT ||
        hi < SODA_HIP_BORDER_WRAP || hi > SODA_HIP_BORDER_CONSTANT)
      return fail(SODA_HIP_ERR_INVALID,
                  "border: a face mode that is none of SODA_HIP_BORDER_*; "
                  "nothing was launched");
    if ((lo == SODA_HIP_BORDER_WRAP) != (hi == SODA_HIP_BORDER_WRAP))
      return fail(SODA_HIP_ERR_INVALID,
                  "border: a dimension wraps on both faces or on none (wrap "
                  "on one face only is not served); nothing was launched");
    if (lo != SODA_HIP_BORDER_WRAP) all_wrap = false;
    if (lo != hi) out->asymmetric = true;
    out->mode_hi[d] = hi;
  }
  if (!all_wrap && desc->domain.refill_every > 1)
    return fail(SODA_HIP_ERR_INVALID,
                "border: only a wrapped ghost evolves with its interior: with "
                "any other mode the frame is refilled after every iteration "
                "(refill_every 0 or 1); nothing was launched");
  const bool per_face = faces && faces->per_face_constants;
  for (int i = 0; i < nin; ++i) {
    const uint64_t first = per_face ? faces->constant[i][0][0]
                                    : desc->constant[i];
    out->low.constant[i] = first;
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        const uint64_t c = per_face ? faces->constant[i][d][side] : first;
        out->constant[i][d][side] = c;
      }
  }
  // Only a CONSTANT face ever shows its constant: a tensor's constants are
  // one where those of its CONSTANT faces are, and that one is the request's
  for (int i = 0; i < nin && per_face; ++i) {
    bool seen = false;
    uint64_t shown = out->low.constant[i];
    for (int d = 0; d < dim; ++d)
      for (int side = 0; side < 2; ++side) {
        const int32_t m = side ? out->mode_hi[d] : desc->mode[d];
        if (m != SODA_HIP_BORDER_CONSTANT) continue;
        if (seen && out->constant[i][d][side] != shown) out->asymmetric = true;
        if (!seen) shown = out->constant[i][d][side];
        seen = true;
      }
    out->low.constant[i] = shown;
  }
  return SODA_HIP_OK;
}

// SODA_HIP_FACES_FORCE=1 (A/B runs, tools/faces_ab.py; read once per handle,
// when it is made): a create twin that is given the faces module serves a
// symmetric request with it too
bool faces_forced() {
  const char* g = getenv("SODA_HIP_FACES_FORCE");
  return g && !strcmp(g, "1");
}

// soda_hip_border_fused_plan: a handle on the domain whose
// chunks run fused on P, and per wall dimension a handle of the same kind on
// a narrow strip that advances the cells near the two walls one iteration at
// a time.  *all_wrap: the request is a torus.
int fused_plan_core(const soda_hip_plan_t* plan,
                    const soda_hip_border_fused_desc_t* desc, int32_t iterate,
                    soda_hip_border_fused_info_t* info, int32_t capacity,
                    int32_t* chunks, int32_t* count, bool* all_wrap) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, "border_fused_plan: NULL argument");
  if (int rc = border_modes(plan, &desc->border, all_wrap)) return rc;
  if (desc->border.domain.refill_every > 1)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused: refill_every is 0 or 1 here, the depth takes "
                "its place; nothing was launched");
  if (desc->depth < 0)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused: depth < 0; nothing was launched");
  soda_hip_border_fused_info_t out;
  memset(&out, 0, sizeof out);
  // everything soda_hip_border_plan asks of the plan, of N and of the frame
  soda_hip_periodic_desc_t domain = desc->border.domain;
  domain.refill_every = 1;
  const Kind& kind = *all_wrap ? kTorus : kBorder;
  if (int rc = plan_core(kind, plan, &domain, iterate, &out.main, capacity,
                         chunks, count))
    return rc;
  const int dim = plan->dim;
  int32_t depth = desc->depth;
  if (depth == 0) depth = deepest_pass(*plan);
  if (depth < 1) return fail(SODA_HIP_ERR_INVALID, "border_fused: bad plan");
  const int32_t* rlo = desc->reach_lo;
  const int32_t* rhi = desc->reach_hi;
  for (int d = 0; d < dim; ++d)
    if (rlo[d] < 0 || rhi[d] < 0)
      return fail(SODA_HIP_ERR_INVALID,
                  "border_fused: a negative reach; nothing was launched");
  if (plan->has_reach &&
      (rlo[dim - 1] < plan->reach_lo || rhi[dim - 1] < plan->reach_hi))
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused: a reach along the last dimension below the "
                "plan's; nothing was launched");
  // the fallbacks: a program that cannot iterate, a wall dimension too narrow
  // for the two parts of its strip
  const int32_t* n = domain.extent;
  if (!*all_wrap) {
    if (!can_iterate(*plan, domain.not_iterable != 0)) depth = 1;
    for (int d = 0; d < dim; ++d)
      if (desc->border.mode[d] != SODA_HIP_BORDER_WRAP &&
          (int64_t)n[d] < 2 * (int64_t)depth * ((int64_t)rlo[d] + rhi[d]))
        depth = 1;
  }
  for (int d = 0; d < dim; ++d) {
    const int64_t times =
        desc->border.mode[d] == SODA_HIP_BORDER_WRAP ? depth : 1;
    if (domain.ghost_lo[d] < times * rlo[d] ||
        domain.ghost_hi[d] < times * rhi[d]) {
      char buf[256];
      snprintf(buf, sizeof buf,
               "border_fused: a frame of %d / %d cells along dimension %d, "
               "where %d iteration(s) reach %d / %d; nothing was launched",
               domain.ghost_lo[d], domain.ghost_hi[d], d, (int)times,
               (int)(times * rlo[d]), (int)(times * rhi[d]));
      return fail(SODA_HIP_ERR_INVALID, buf);
    }
  }
  out.depth = depth;
  if (*all_wrap) {
    domain.refill_every = depth;
    if (int rc = plan_core(kTorus, plan, &domain, iterate, &out.main, capacity,
                           chunks, count))
      return rc;
  } else if (depth > 1) {
    list_chunks(iterate, depth, capacity, chunks, count);
    for (int d = 0; d < dim; ++d) {
      if (desc->border.mode[d] == SODA_HIP_BORDER_WRAP || rlo[d] + rhi[d] == 0)
        continue;
      soda_hip_border_strip_t& s = out.strip[out.num_strips++];
      s.dim = d;
      s.lo = s.hi = depth * (rlo[d] + rhi[d]);
      s.take_lo = (depth - 1) * rlo[d];
      s.take_hi = (depth - 1) * rhi[d];
      soda_hip_periodic_desc_t sdom = domain;
      sdom.extent[d] = s.lo + s.hi;
      for (int e = 0; e < SODA_HIP_MAX_DIM; ++e)
        s.extent[e] = e < dim ? sdom.extent[e] : 1;
      if (int rc = plan_core(kBorder, plan, &sdom, 0, &s.info, 0, nullptr,
                             nullptr))
        return rc;
    }
  }
  out.scratch_bytes = out.main.scratch_bytes;
  for (int i = 0; i < out.num_strips; ++i)
    out.scratch_bytes += out.strip[i].info.scratch_bytes;
  if (info) *info = out;
  return SODA_HIP_OK;
}

// The partition of the domain a residual counts by, from the
// numbers of a resolved plan alone: the trusted box in the padded coordinates
// of the domain, per strip the two rims it scatters in the strip's own, cut to
// the trusted interval in every wall dimension below the strip's.  A wall
// dimension's trusted interval is what its strip does not take (all of it
// where the reach is zero and there is no strip), a WRAP dimension's is all.
void residual_boxes(const soda_hip_border_fused_info_t& info,
                    const int32_t* n, int dim,
                    soda_hip_border_fused_boxes_t* out) {
  memset(out, 0, sizeof *out);
  out->depth = info.depth;
  out->num_strips = info.num_strips;
  int32_t tlo[4] = {0, 0, 0, 0}, thi[4] = {1, 1, 1, 1};   // domain coordinates
  for (int d = 0; d < dim; ++d) thi[d] = n[d];
  for (int i = 0; i < info.num_strips; ++i) {
    const soda_hip_border_strip_t& s = info.strip[i];
    tlo[s.dim] = s.take_lo;
    thi[s.dim] = n[s.dim] - s.take_hi;
  }
  for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
    const int32_t g = d < dim ? info.main.ghost_lo[d] : 0;
    out->trusted_lo[d] = g + tlo[d];
    out->trusted_hi[d] = g + thi[d];
  }
  for (int i = 0; i < info.num_strips; ++i) {
    const soda_hip_border_strip_t& s = info.strip[i];
    soda_hip_border_rims_t& r = out->strip[i];
    r.dim = s.dim;
    for (int side = 0; side < 2; ++side)
      for (int e = 0; e < SODA_HIP_MAX_DIM; ++e) {
        const int32_t g = e < dim ? s.info.ghost_lo[e] : 0;
        int32_t lo = 0, hi = e < dim ? n[e] : 1;
        if (e == s.dim) {
          lo = side ? s.lo + s.hi - s.take_hi : 0;
          hi = side ? s.lo + s.hi : s.take_lo;
        } else if (e < s.dim) {      // (trusted == whole where e has no walls)
          lo = tlo[e];
          hi = thi[e];
        }
        r.lo[side][e] = g + lo;
        r.hi[side][e] = g + hi;
      }
  }
}

}  // namespace

// -- the handles --------------------------------------------------------------

struct soda_hip_periodic : Frame {
  soda_hip_program* prog = nullptr;
  int32_t k = 1;
  bool not_iterable = false;
  std::vector<DeviceBuffer> pad_in;    // dense entry: the padded inputs
  std::vector<DeviceBuffer> pad_out;   // ... and outputs
  std::vector<DeviceBuffer> pong;      // the chunks' partner of the outputs
};

struct soda_hip_border_fused {
  soda_hip_periodic* main = nullptr;
  int32_t depth = 1;
  int nstrips = 0;
  struct Strip {
    soda_hip_periodic* h = nullptr;
    int32_t d = 0, lo = 0, hi = 0, take_lo = 0, take_hi = 0;
  } strip[SODA_HIP_MAX_DIM];
  Helpers box;                           // the box kernels
  soda_hip_border_fused_boxes_t boxes;   // where a residual counts each cell
};

namespace {

int create_core(const Kind& kind, soda_hip_program_t* p,
                const soda_hip_periodic_desc_t* desc, const int32_t* mode,
                const uint64_t* constant, const void* const* code,
                const size_t* code_size, soda_hip_periodic** handle,
                int32_t batch = 0, const FaceRule* rule = nullptr) {
  // (`rule`: a handle that fills by the faces kernels, `code` their modules)
  const std::string who(kind.who);
  const char* what = rule ? "faces" : "wrap";
  const soda_hip_plan_t& plan = p->plan;
  if (p->bank_tensors)
    return fail(SODA_HIP_ERR_UNSUPPORTED,
                who + ": programs on wire-format banks are not served on " +
                    kind.domain + "; nothing was launched");
  soda_hip_periodic_info_t info;
  if (int rc = plan_core(kind, &plan, desc, 0, &info, 0, nullptr, nullptr,
                         batch))
    return rc;
  const int nin = plan.num_inputs, nout = plan.num_outputs;
  bool need[4] = {false, false, false, false};
  if (int rc = helpers_needed(plan, code, code_size, who, what, need))
    return rc;
  HIP_TRY(hipSetDevice(p->device));
  soda_hip_periodic* h = new (std::nothrow) soda_hip_periodic;
  if (!h) return fail(SODA_HIP_ERR_NOMEM, "new " + who + " handle");
  h->prog = p;
  h->kind = &kind;
  h->batch = batch;
  h->k = info.refill_every;
  h->not_iterable = desc->not_iterable != 0;
  const bool iterates = can_iterate(plan, h->not_iterable);
  h->t.dim = plan.dim;
  for (int d = 0; d < 4; ++d) {
    h->t.n[d] = d < plan.dim ? desc->extent[d] : 1;
    h->t.glo[d] = info.ghost_lo[d];
    h->t.ghi[d] = info.ghost_hi[d];
    h->t.p[d] = info.padded[d];
    if (mode) h->mode[d] = d < plan.dim ? mode[d] : 0;
  }
  if (constant)
    for (int i = 0; i < nin; ++i) h->constant[i] = constant[i];
  if (rule) {
    h->faces = true;
    memcpy(h->mode_hi, rule->mode_hi, sizeof h->mode_hi);
    memcpy(h->face_constant, rule->constant, sizeof h->face_constant);
  }
  int rc = load_helpers(&h->wrap, need, code, rule ? "soda_faces" : kind.kernel,
                        plan.dim, who, what, batch > 0);
  // (a batched handle: every array [batch, P...])
  const int64_t cells = cells_of(h->t.p, plan.dim) * h->items();
  h->pad_in.resize(nin);
  h->pad_out.resize(nout);
  h->pong.resize(iterates ? nout : 0);
  for (int i = 0; i < nin && !rc; ++i)
    rc = ensure(h->pad_in[i], (size_t)cells * plan.elem_size[i]);
  for (int o = 0; o < nout && !rc; ++o) {
    rc = ensure(h->pad_out[o], (size_t)cells * plan.elem_size[nin + o]);
    if (!rc && iterates)
      rc = ensure(h->pong[o], (size_t)cells * plan.elem_size[nin + o]);
  }
  if (rc) {
    const std::string why = last_error_text();
    soda_hip_periodic_destroy(h);
    return fail(rc, why);
  }
  *handle = h;
  return SODA_HIP_OK;
}

// The two boxes of a strip in padded coordinates: the gather takes the
// domain's cells [0, L) and [N - H, N) along d into the strip's [0, L + H),
// the scatter the strip's [0, take_lo) and [L + H - take_hi, L + H) back to
// the domain's two rims; every other dimension over the whole domain.
void strip_boxes(const soda_hip_border_fused* f,
                 const soda_hip_border_fused::Strip& s, bool gather,
                 Box* low, Box* high) {
  const Torus& m = f->main->t;
  const int d = s.d;
  for (int e = 0; e < 4; ++e) {
    low->to[e] = low->from[e] = high->to[e] = high->from[e] = m.glo[e];
    low->size[e] = high->size[e] = m.n[e];
  }
  const int32_t g = m.glo[d], n = m.n[d], w = s.lo + s.hi;
  if (gather) {                 // main -> strip
    low->size[d] = s.lo;
    high->size[d] = s.hi;
    high->to[d] = g + s.lo;
    high->from[d] = g + n - s.hi;
  } else {                      // strip -> main
    low->size[d] = s.take_lo;
    high->size[d] = s.take_hi;
    high->to[d] = g + n - s.take_hi;
    high->from[d] = g + w - s.take_hi;
  }
}

// -- the chunk loop -----------------------------------------------------------

// The same box for every pair: [lo, hi) per dimension of the handle's padded
// arrays.
soda_hip_resbox_t resbox_of(const soda_hip_periodic* h, const int32_t* lo,
                            const int32_t* hi) {
  soda_hip_resbox_t box;
  memset(&box, 0, sizeof box);
  for (int o = 0; o < h->prog->plan.num_outputs; ++o)
    for (int d = 0; d < SODA_HIP_MAX_DIM; ++d) {
      box.lo[o][d] = d < h->t.dim ? lo[d] : 0;
      box.hi[o][d] = d < h->t.dim ? hi[d] : 1;
    }
  return box;
}

// the counted cells of a torus or a depth-1 bordered domain: the interior
soda_hip_resbox_t interior_box(const soda_hip_periodic* h) {
  int32_t hi[4];
  for (int d = 0; d < 4; ++d) hi[d] = h->t.glo[d] + h->t.n[d];
  return resbox_of(h, h->t.glo, hi);
}

// The chunks of a run on padded arrays of handle `h`, `k` iterations each and
// the last one what is left: `inputs` filled in, `outputs` filled out, the
// chunks alternating between `outputs` and the handle's `pong` so that the
// last one lands in `outputs`.  `step(dst, src, n, last)` advances one chunk
// of n iterations from `src` (inputs, then the param arrays) to `dst`; the
// frame of `dst` is filled behind it.
template <class Step>
int chunk_loop(soda_hip_periodic* h, int32_t k, void* const* outputs,
               const void* const* inputs, int32_t iterate, void* stream,
               Step step) {
  const soda_hip_plan_t& plan = h->prog->plan;
  const int nin = plan.num_inputs, nout = plan.num_outputs;
  const int chunks = (iterate + k - 1) / k;
  std::vector<const void*> src(inputs, inputs + nin + plan.num_params);
  std::vector<void*> dst(nout);
  std::vector<int32_t> elem(nout);
  for (int o = 0; o < nout; ++o) elem[o] = plan.elem_size[nin + o];
  int32_t left = iterate;
  for (int c = 0; c < chunks; ++c) {
    const int32_t n = chunk_len(left, k);
    const bool to_out = ((chunks - 1 - c) % 2) == 0;
    for (int o = 0; o < nout; ++o)
      dst[o] = to_out ? outputs[o] : h->pong[o].ptr;
    if (int rc = step(dst.data(), src.data(), n, c + 1 == chunks)) return rc;
    if (int rc = wrap_launch(*h, kFill, dst.data(), dst.data(), elem.data(),
                             nout, static_cast<hipStream_t>(stream)))
      return rc;
    left -= n;
    if (c + 1 < chunks)
      for (int i = 0; i < nin; ++i) src[i] = dst[i];
  }
  return SODA_HIP_OK;
}

// What the last chunk of run_chunks takes of a residual.
// `behind` false: box[0] rides in the chunk's run (run_core: a twin, or the
// generic kernels behind the one-iteration pass).  `behind` true, a strip:
// every box is counted behind the chunk by the generic kernels, cur the
// chunk's result, prev what it read.
struct ChunkResidual {
  ResidualRun run;
  soda_hip_resbox_t box[2];
  int nbox;
  bool behind;
};

// The chunks of a torus, a depth-1 bordered domain or a strip: a chunk is one
// run of the program on the padded extent.
int run_chunks(soda_hip_periodic* h, void* const* outputs,
               const void* const* inputs, int32_t iterate, void* stream,
               const ChunkResidual* res = nullptr) {
  soda_hip_program* p = h->prog;
  return chunk_loop(
      h, h->k, outputs, inputs, iterate, stream,
      [&](void* const* dst, const void* const* src, int32_t n,
          bool last) -> int {
        RunRequest rq = {dst, src, h->t.p, n, stream};
        rq.batch = h->items();
        ResidualRun riding;
        if (res && last && !res->behind) {
          riding = res->run;
          riding.box = &res->box[0];
          rq.residual = &riding;
        }
        if (int rc = run_core(p, rq)) return rc;
        if (res && last && res->behind)
          for (int b = 0; b < res->nbox; ++b)
            if (int rc = residual_add(p, dst, src, h->t.p, res->run,
                                      res->box[b], stream))
              return rc;
        return SODA_HIP_OK;
      });
}

// The chunks of a fused run with strips: per chunk of n <= depth iterations
// the strips gathered from the chunk's inputs and advanced n times, the
// interior launched on P, the strips' rims scattered over its result (and the
// frame filled, by the loop).  One stream, in that order.
// `res`: the last chunk also takes the residual, each cell where it is made
// right: the struct zeroed once ahead of the gather, the rims
// behind every strip's last iteration, the trusted box in the interior's run.
int fused_chunks(soda_hip_border_fused* f, void* const* outputs,
                 const void* const* inputs, int32_t iterate, void* stream_,
                 const ResidualRun* res) {
  soda_hip_periodic* h = f->main;
  soda_hip_program* p = h->prog;
  const soda_hip_plan_t& plan = p->plan;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int nin = plan.num_inputs, nout = plan.num_outputs, dim = plan.dim;
  std::vector<const void*> ssrc(inputs, inputs + nin + plan.num_params);
  std::vector<void*> sin(nin), sout(nout);
  std::vector<int32_t> ein(nin), eout(nout);
  for (int i = 0; i < nin; ++i) ein[i] = plan.elem_size[i];
  for (int o = 0; o < nout; ++o) eout[o] = plan.elem_size[nin + o];
  return chunk_loop(
      h, f->depth, outputs, inputs, iterate, stream_,
      [&](void* const* dst, const void* const* src, int32_t n,
          bool last) -> int {
        const bool take = res && last;
        ChunkResidual part;
        if (take) {
          if (int rc = residual_zero(p, *res, stream_)) return rc;
          part.run = *res;
          part.run.accumulate = true;
        }
        for (int k = 0; k < f->nstrips; ++k) {
          const soda_hip_border_fused::Strip& s = f->strip[k];
          Box box[2];
          strip_boxes(f, s, true, &box[0], &box[1]);
          for (int i = 0; i < nin; ++i) {
            sin[i] = s.h->pad_in[i].ptr;
            ssrc[i] = sin[i];
          }
          for (int o = 0; o < nout; ++o) sout[o] = s.h->pad_out[o].ptr;
          if (int rc = box_launch(f->box, sin.data(), s.h->t.p, src, h->t.p,
                                  ein.data(), nin, box, 2, dim, stream))
            return rc;
          if (int rc = wrap_launch(*s.h, kFill, sin.data(), ssrc.data(),
                                   ein.data(), nin, stream))
            return rc;
          if (take) {
            const soda_hip_border_rims_t& r = f->boxes.strip[k];
            part.box[0] = resbox_of(s.h, r.lo[0], r.hi[0]);
            part.box[1] = resbox_of(s.h, r.lo[1], r.hi[1]);
            part.nbox = 2;
            part.behind = true;
          }
          if (int rc = run_chunks(s.h, sout.data(), ssrc.data(), n, stream_,
                                  take ? &part : nullptr))
            return rc;
        }
        RunRequest rq = {dst, src, h->t.p, n, stream_};
        if (take) {
          part.box[0] = resbox_of(h, f->boxes.trusted_lo, f->boxes.trusted_hi);
          part.run.box = &part.box[0];
          rq.residual = &part.run;
        }
        if (int rc = run_core(p, rq)) return rc;
        for (int k = 0; k < f->nstrips; ++k) {
          const soda_hip_border_fused::Strip& s = f->strip[k];
          Box box[2];
          strip_boxes(f, s, false, &box[0], &box[1]);
          for (int o = 0; o < nout; ++o) sout[o] = s.h->pad_out[o].ptr;
          if (int rc = box_launch(f->box, dst, h->t.p,
                                  const_cast<const void* const*>(sout.data()),
                                  s.h->t.p, eout.data(), nout, box, 2, dim,
                                  stream))
            return rc;
        }
        return SODA_HIP_OK;
      });
}

// What a run entry runs on: the handle on the domain -- its frame, its scratch
// and its name in messages -- and, where its chunks run fused, the handle that
// has it as `main`.
struct Domain {
  soda_hip_periodic* h;
  soda_hip_border_fused* fused;

  // The chunks of a run on padded arrays; `res`: with the residual of the
  // last iteration over the whole domain.  A fused handle without strips (a
  // torus, depth 1) runs the plain chunks of its main handle.
  int chunks(void* const* outputs, const void* const* inputs, int32_t iterate,
             void* stream, const ResidualRun* res = nullptr) const {
    if (fused && fused->nstrips)
      return fused_chunks(fused, outputs, inputs, iterate, stream, res);
    if (!res) return run_chunks(h, outputs, inputs, iterate, stream);
    const ChunkResidual whole = {*res, {interior_box(h), {}}, 1, false};
    return run_chunks(h, outputs, inputs, iterate, stream, &whole);
  }
};

Domain domain_of(soda_hip_periodic* h) { return {h, nullptr}; }
Domain domain_of(soda_hip_border_fused* f) { return {f->main, f}; }

// -- the run cores ------------------------------------------------------------

// The device entry contract (include/soda_hip.h, soda_hip_run_device) on the
// caller's arrays, each the dense array of `batch` items of `extent`: no output
// shares a byte with an input, a param array or another output; inputs and
// outputs are aligned to min(16, vec x cell size) bytes.
int check_contract(const soda_hip_plan_t& plan, void* const* outputs,
                   const void* const* inputs, const int32_t* extent,
                   int32_t batch, const char* who_) {
  const std::string who(who_);
  const int nin = plan.num_inputs, nout = plan.num_outputs;
  const int prm0 = nin + nout + plan.num_locals;
  for (int i = 0; i < nin + plan.num_params; ++i)
    if (!inputs[i]) return fail(SODA_HIP_ERR_INVALID, who + ": NULL input");
  for (int o = 0; o < nout; ++o)
    if (!outputs[o]) return fail(SODA_HIP_ERR_INVALID, who + ": NULL output");
  const uint64_t cells = (uint64_t)cells_of(extent, plan.dim) * batch;
  auto overlap = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
  };
  for (int o = 0; o < nout; ++o) {
    const uint64_t no = cells * plan.elem_size[nin + o];
    for (int i = 0; i < nin; ++i)
      if (overlap(outputs[o], no, inputs[i], cells * plan.elem_size[i]))
        return fail(SODA_HIP_ERR_INVALID,
                    who + ": an output overlaps an input; nothing was "
                          "launched");
    for (int k = 0; k < plan.num_params; ++k)
      if (overlap(outputs[o], no, inputs[nin + k],
                  (uint64_t)plan.param_elems[k] * plan.elem_size[prm0 + k]))
        return fail(SODA_HIP_ERR_INVALID,
                    who + ": an output overlaps a param array; nothing was "
                          "launched");
    for (int q = 0; q < o; ++q)
      if (overlap(outputs[o], no, outputs[q],
                  cells * plan.elem_size[nin + q]))
        return fail(SODA_HIP_ERR_INVALID,
                    who + ": two outputs overlap; nothing was launched");
  }
  const int32_t vec = plan_vec(plan);
  for (int t = 0; t < nin + nout; ++t) {
    const void* ptr = t < nin ? inputs[t] : outputs[t - nin];
    int64_t align = (int64_t)vec * plan.elem_size[t];
    if (align > 16) align = 16;
    if (reinterpret_cast<uintptr_t>(ptr) % (uintptr_t)align) {
      char buf[200];
      snprintf(buf, sizeof buf,
               ": %s %d at %p is not aligned to %d bytes; nothing was "
               "launched", t < nin ? "input" : "output",
               t < nin ? t : t - nin, ptr, (int)align);
      return fail(SODA_HIP_ERR_INVALID, who + buf);
    }
  }
  return SODA_HIP_OK;
}

int fill_core(soda_hip_periodic* h, void* const* arrays, int32_t count,
              void* stream) {
  const std::string who(h->kind->who);
  const soda_hip_plan_t& plan = h->prog->plan;
  if (count < 0 || count > plan.num_outputs)
    return fail(SODA_HIP_ERR_INVALID,
                who + "_fill: one array per output at most; nothing was "
                      "launched");
  int32_t elem[SODA_HIP_MAX_TENSORS];
  for (int i = 0; i < count; ++i) {
    elem[i] = plan.elem_size[plan.num_inputs + i];
    if (!arrays[i] || reinterpret_cast<uintptr_t>(arrays[i]) % elem[i])
      return fail(SODA_HIP_ERR_INVALID,
                  who + "_fill: an array is NULL or not aligned to its cell "
                        "size; nothing was launched");
  }
  HIP_TRY(hipSetDevice(h->prog->device));
  return wrap_launch(*h, kFill, arrays,
                     const_cast<const void* const*>(arrays), elem, count,
                     static_cast<hipStream_t>(stream));
}

int run_padded_core(const Domain& dom, void* const* outputs,
                    const void* const* inputs, int32_t iterate,
                    void* stream) {
  soda_hip_periodic* h = dom.h;
  const std::string who = std::string(h->kind->who) + "_run_padded";
  if (int rc = check_iterate(h->prog->plan, h->not_iterable, iterate,
                             who.c_str()))
    return rc;
  if (int rc = check_contract(h->prog->plan, outputs, inputs, h->t.p,
                              h->items(), who.c_str()))
    return rc;
  return dom.chunks(outputs, inputs, iterate, stream);
}

// The dense entries' staging in the handle's padded scratch: `in` / `out` its
// padded inputs / outputs, `src` what a run from `in` reads (then the
// caller's param arrays).
struct Staging {
  soda_hip_periodic* h;
  const void* const* inputs;
  std::vector<void*> in, out;
  std::vector<const void*> src;
  std::vector<int32_t> ein, eout;

  Staging(soda_hip_periodic* h_, const void* const* inputs_)
      : h(h_), inputs(inputs_) {
    const soda_hip_plan_t& plan = h->prog->plan;
    const int nin = plan.num_inputs, nout = plan.num_outputs;
    in.resize(nin);
    ein.resize(nin);
    out.resize(nout);
    eout.resize(nout);
    src.assign(inputs, inputs + nin + plan.num_params);
    for (int i = 0; i < nin; ++i) {
      in[i] = h->pad_in[i].ptr;
      src[i] = in[i];
      ein[i] = plan.elem_size[i];
    }
    for (int o = 0; o < nout; ++o) {
      out[o] = h->pad_out[o].ptr;
      eout[o] = plan.elem_size[nin + o];
    }
  }

  // pad: every cell of the padded inputs, ghosts included
  int pad(hipStream_t stream) {
    return wrap_launch(*h, kPad, in.data(), inputs, ein.data(),
                       (int)in.size(), stream);
  }

  // crop: the caller's dense outputs from the padded arrays `from`
  int crop(void* const* outputs, void* const* from, hipStream_t stream) {
    return wrap_launch(*h, kCrop, outputs,
                       const_cast<const void* const*>(from), eout.data(),
                       (int)out.size(), stream);
  }
};

int run_device_core(const Domain& dom, void* const* outputs,
                    const void* const* inputs, int32_t iterate,
                    void* stream_) {
  soda_hip_periodic* h = dom.h;
  const std::string who = std::string(h->kind->who) + "_run_device";
  const soda_hip_plan_t& plan = h->prog->plan;
  if (int rc = check_iterate(plan, h->not_iterable, iterate, who.c_str()))
    return rc;
  // the device entry contract on the caller's dense arrays of N
  if (int rc = check_contract(plan, outputs, inputs, h->t.n, h->items(),
                              who.c_str()))
    return rc;
  HIP_TRY(hipSetDevice(h->prog->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  Staging st(h, inputs);
  if (int rc = st.pad(stream)) return rc;
  if (int rc = dom.chunks(st.out.data(), st.src.data(), iterate, stream_))
    return rc;
  return st.crop(outputs, st.out.data(), stream);
}

// The residual of a batch is not served: the entries that
// take one refuse a batched handle before anything else.
int refuse_batched(const soda_hip_periodic* h, const std::string& who) {
  if (!h->batch) return SODA_HIP_OK;
  return fail(SODA_HIP_ERR_UNSUPPORTED,
              who + ": residuals, norms and runs until converged are not "
                    "served on a batched handle; nothing was launched");
}

// <handle>_run_padded_residual / _run_padded_norms (`norms` != nullptr):
// run_padded_core with the struct at `dev` filled.  Every
// refusal comes before the first launch.
int run_padded_residual_core(const Domain& dom, soda_hip_norms_handle* norms,
                             void* const* outputs, const void* const* inputs,
                             int32_t iterate, void* dev, void* stream) {
  soda_hip_periodic* h = dom.h;
  const std::string who = std::string(h->kind->who) +
                          (norms ? "_run_padded_norms" : "_run_padded_residual");
  soda_hip_program* p = h->prog;
  if (int rc = refuse_batched(h, who)) return rc;
  for (int o = 0; o < p->plan.num_outputs; ++o)
    if (!outputs[o]) return fail(SODA_HIP_ERR_INVALID, who + ": NULL output");
  if (int rc = norms ? check_norms_request(p, norms, outputs, h->t.p, dev,
                                           who.c_str())
                     : check_residual_request(p, outputs, h->t.p, dev,
                                              who.c_str()))
    return rc;
  if (int rc = check_iterate(p->plan, h->not_iterable, iterate, who.c_str()))
    return rc;
  if (int rc = check_contract(p->plan, outputs, inputs, h->t.p, 1,
                              who.c_str()))
    return rc;
  const ResidualRun run = {dev, 0, norms};
  return dom.chunks(outputs, inputs, iterate, stream, &run);
}

// <handle>_run_until / _run_until_norm on DENSE arrays of N: pads once, runs
// `check_every` iterations at a time on the handle's padded scratch until
// `converged(&stop)` says so by the struct of the last chunk -- `host_bytes`
// fetched into `host` -- or `max_iterate` iterations are done, crops.  The
// first chunk goes from pad_in to pad_out, every later one back into the set
// the one before it read (an iterable program's pad_in[i] is as large as its
// pad_out[i]).  Synchronous.
template <class Converged>
int run_until_core(const Domain& dom, soda_hip_norms_handle* norms,
                   void* const* outputs, const void* const* inputs,
                   int32_t max_iterate, int32_t check_every, void* host,
                   size_t host_bytes, Converged converged,
                   int32_t* iterations_done, void* stream_) {
  soda_hip_periodic* h = dom.h;
  const std::string who = std::string(h->kind->who) +
                          (norms ? "_run_until_norm" : "_run_until");
  soda_hip_program* p = h->prog;
  const soda_hip_plan_t& plan = p->plan;
  const int nin = plan.num_inputs, nout = plan.num_outputs;
  if (int rc = refuse_batched(h, who)) return rc;
  if (max_iterate < 1 || check_every < 1)
    return fail(SODA_HIP_ERR_INVALID,
                who + ": max_iterate and check_every must be >= 1");
  for (int o = 0; o < nout; ++o)
    if (!outputs[o]) return fail(SODA_HIP_ERR_INVALID, who + ": NULL output");
  if (int rc = norms ? check_norms_request(p, norms, outputs, h->t.n, nullptr,
                                           who.c_str())
                     : check_residual_request(p, outputs, h->t.n, nullptr,
                                              who.c_str()))
    return rc;
  if (int rc = check_iterate(plan, h->not_iterable, max_iterate, who.c_str()))
    return rc;
  if (int rc = check_contract(plan, outputs, inputs, h->t.n, 1, who.c_str()))
    return rc;
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &capture) != hipSuccess) {
    (void)hipGetLastError();
    capture = hipStreamCaptureStatusNone;
  }
  if (capture != hipStreamCaptureStatusNone)
    return fail(SODA_HIP_ERR_INVALID,
                who + ": synchronous, not for a stream that is being captured; "
                      "nothing was launched");
  if (int rc = ensure(p->until_struct, host_bytes)) return rc;
  Staging st(h, inputs);
  if (int rc = st.pad(stream)) return rc;
  memset(host, 0, host_bytes);
  const ResidualRun run = {p->until_struct.ptr, 0, norms};
  void* const* dst = st.out.data();
  int32_t done = 0;
  for (int32_t chunk = 0; done < max_iterate; ++chunk) {
    const int32_t n = chunk_len(max_iterate - done, check_every);
    dst = chunk % 2 ? st.in.data() : st.out.data();
    if (int rc = dom.chunks(dst, st.src.data(), n, stream_, &run)) return rc;
    HIP_TRY(hipMemcpyAsync(host, p->until_struct.ptr, host_bytes,
                           hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    done += n;
    bool stop = false;
    if (int rc = converged(&stop)) return rc;
    if (stop) break;
    // (another chunk follows: the program iterates, nin == nout)
    for (int i = 0; i < nin; ++i) st.src[i] = dst[i];
  }
  if (int rc = st.crop(outputs, dst, stream)) return rc;
  HIP_TRY(hipStreamSynchronize(stream));
  if (iterations_done) *iterations_done = done;
  return SODA_HIP_OK;
}

int until_residual(const Domain& dom, void* const* outputs,
                   const void* const* inputs, int32_t max_iterate,
                   int32_t check_every, double tol, uint64_t int_tol,
                   soda_hip_residual_t* result_host, int32_t* iterations_done,
                   void* stream) {
  soda_hip_residual_t host;
  auto converged = [&](bool* stop) {
    *stop = residual_converged(host, tol, int_tol);
    return (int)SODA_HIP_OK;
  };
  if (int rc = run_until_core(dom, nullptr, outputs, inputs, max_iterate,
                              check_every, &host, sizeof host, converged,
                              iterations_done, stream))
    return rc;
  if (result_host) *result_host = host;
  return SODA_HIP_OK;
}

int until_norm(const Domain& dom, soda_hip_norms_handle* norms,
               void* const* outputs, const void* const* inputs,
               int32_t max_iterate, int32_t check_every, int32_t which,
               double tol, soda_hip_norms_t* result_host,
               int32_t* iterations_done, void* stream) {
  const std::string who = std::string(dom.h->kind->who) + "_run_until_norm";
  if (which != SODA_HIP_NORMS_WHICH_L1 && which != SODA_HIP_NORMS_WHICH_L2)
    return fail(SODA_HIP_ERR_INVALID, who + ": bad `which`");
  soda_hip_norms_t host;
  auto converged = [&](bool* stop) {
    if (!norms_converged(host, which, tol, stop))
      return fail(SODA_HIP_ERR_RUNTIME,
                  who + ": the struct fetched is of no kind");
    return (int)SODA_HIP_OK;
  };
  if (int rc = run_until_core(dom, norms, outputs, inputs, max_iterate,
                              check_every, &host, sizeof host, converged,
                              iterations_done, stream))
    return rc;
  if (result_host) *result_host = host;
  return SODA_HIP_OK;
}

}  // namespace

// -- the exported entries -----------------------------------------------------

extern "C" {

int soda_hip_periodic_plan(const soda_hip_plan_t* plan,
                           const soda_hip_periodic_desc_t* desc,
                           int32_t iterate, soda_hip_periodic_info_t* info,
                           int32_t capacity, int32_t* chunks, int32_t* count) {
  return plan_core(kTorus, plan, desc, iterate, info, capacity, chunks, count);
}

int soda_hip_periodic_create(soda_hip_program_t* p,
                             const soda_hip_periodic_desc_t* desc,
                             const void* const* wrap_code,
                             const size_t* wrap_code_size,
                             soda_hip_periodic_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !wrap_code || !wrap_code_size || !handle)
    return fail(SODA_HIP_ERR_INVALID, "periodic_create: NULL argument");
  return create_core(kTorus, p, desc, nullptr, nullptr, wrap_code,
                     wrap_code_size, handle);
}

// -- batched domains: the entries above over a batch --------

int soda_hip_periodic_plan_batch(const soda_hip_plan_t* plan,
                                 const soda_hip_periodic_desc_t* desc,
                                 int32_t batch, int32_t iterate,
                                 soda_hip_periodic_info_t* info,
                                 int32_t capacity, int32_t* chunks,
                                 int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, "periodic_plan_batch: NULL argument");
  if (int rc = check_domain_batch(*plan, batch, "periodic_plan_batch"))
    return rc;
  return plan_core(kTorus, plan, desc, iterate, info, capacity, chunks, count,
                   batch);
}

int soda_hip_periodic_create_batch(soda_hip_program_t* p,
                                   const soda_hip_periodic_desc_t* desc,
                                   int32_t batch,
                                   const void* const* wrap_code,
                                   const size_t* wrap_code_size,
                                   soda_hip_periodic_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !wrap_code || !wrap_code_size || !handle)
    return fail(SODA_HIP_ERR_INVALID, "periodic_create_batch: NULL argument");
  if (int rc = check_domain_batch(p->plan, batch, "periodic_create_batch"))
    return rc;
  return create_core(kTorus, p, desc, nullptr, nullptr, wrap_code,
                     wrap_code_size, handle, batch);
}

int soda_hip_border_plan_batch(const soda_hip_plan_t* plan,
                               const soda_hip_border_desc_t* desc,
                               int32_t batch, int32_t iterate,
                               soda_hip_periodic_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, "border_plan_batch: NULL argument");
  if (int rc = check_domain_batch(*plan, batch, "border_plan_batch"))
    return rc;
  bool all_wrap;
  if (int rc = border_modes(plan, desc, &all_wrap)) return rc;
  soda_hip_periodic_desc_t domain = desc->domain;
  if (!all_wrap && domain.refill_every == 0) domain.refill_every = 1;
  return plan_core(all_wrap ? kTorus : kBorder, plan, &domain, iterate, info,
                   capacity, chunks, count, batch);
}

int soda_hip_border_create_batch(soda_hip_program_t* p,
                                 const soda_hip_border_desc_t* desc,
                                 int32_t batch, const void* const* code,
                                 const size_t* code_size,
                                 soda_hip_border_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !code || !code_size || !handle)
    return fail(SODA_HIP_ERR_INVALID, "border_create_batch: NULL argument");
  if (int rc = check_domain_batch(p->plan, batch, "border_create_batch"))
    return rc;
  bool all_wrap;
  if (int rc = border_modes(&p->plan, desc, &all_wrap)) return rc;
  soda_hip_periodic_desc_t domain = desc->domain;
  if (!all_wrap && domain.refill_every == 0) domain.refill_every = 1;
  return create_core(kBorder, p, &domain, desc->mode, desc->constant, code,
                     code_size, handle, batch);
}

int soda_hip_periodic_destroy(soda_hip_periodic_t* h) {
  if (!h) return SODA_HIP_OK;
  (void)hipSetDevice(h->prog->device);
  for (auto* v : {&h->pad_in, &h->pad_out, &h->pong})
    for (auto& b : *v)
      if (b.ptr) (void)hipFree(b.ptr);
  unload_helpers(&h->wrap);
  delete h;
  return SODA_HIP_OK;
}

int soda_hip_periodic_info(soda_hip_periodic_t* h,
                           soda_hip_periodic_info_t* info) {
  if (!h || !info)
    return fail(SODA_HIP_ERR_INVALID,
                std::string(h ? h->kind->who : "periodic") +
                    "_info: NULL argument");
  memset(info, 0, sizeof *info);
  info->refill_every = h->k;
  for (int d = 0; d < 4; ++d) {
    info->ghost_lo[d] = h->t.glo[d];
    info->ghost_hi[d] = h->t.ghi[d];
    info->padded[d] = h->t.p[d];
  }
  for (const auto* v : {&h->pad_in, &h->pad_out, &h->pong})
    for (const auto& b : *v) info->scratch_bytes += (int64_t)b.bytes;
  return SODA_HIP_OK;
}

// -- bordered domains: the same handle behind its modes ----

int soda_hip_border_plan(const soda_hip_plan_t* plan,
                         const soda_hip_border_desc_t* desc, int32_t iterate,
                         soda_hip_periodic_info_t* info, int32_t capacity,
                         int32_t* chunks, int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, "border_plan: NULL argument");
  bool all_wrap;
  if (int rc = border_modes(plan, desc, &all_wrap)) return rc;
  if (all_wrap)
    return soda_hip_periodic_plan(plan, &desc->domain, iterate, info, capacity,
                                  chunks, count);
  soda_hip_periodic_desc_t domain = desc->domain;
  if (domain.refill_every == 0) domain.refill_every = 1;
  return plan_core(kBorder, plan, &domain, iterate, info, capacity, chunks,
                   count);
}

int soda_hip_border_create(soda_hip_program_t* p,
                           const soda_hip_border_desc_t* desc,
                           const void* const* code, const size_t* code_size,
                           soda_hip_border_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !code || !code_size || !handle)
    return fail(SODA_HIP_ERR_INVALID, "border_create: NULL argument");
  bool all_wrap;
  if (int rc = border_modes(&p->plan, desc, &all_wrap)) return rc;
  soda_hip_periodic_desc_t domain = desc->domain;
  if (!all_wrap && domain.refill_every == 0) domain.refill_every = 1;
  return create_core(kBorder, p, &domain, desc->mode, desc->constant, code,
                     code_size, handle);
}

int soda_hip_border_destroy(soda_hip_border_t* h) {
  return soda_hip_periodic_destroy(h);
}

int soda_hip_border_info(soda_hip_border_t* h,
                         soda_hip_periodic_info_t* info) {
  if (!h) return fail(SODA_HIP_ERR_INVALID, "border_info: NULL argument");
  return soda_hip_periodic_info(h, info);
}

// -- bordered domains, fused away from the walls -----------

int soda_hip_border_fused_plan(const soda_hip_plan_t* plan,
                               const soda_hip_border_fused_desc_t* desc,
                               int32_t iterate,
                               soda_hip_border_fused_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count) {
  bool all_wrap;
  return fused_plan_core(plan, desc, iterate, info, capacity, chunks, count,
                         &all_wrap);
}

// soda_hip_border_fused_create; `rule`: of its _faces twin on a request served
// by the faces kernels, `code` their modules -- the main
// handle and every strip take the request's faces and constants
static int fused_create(soda_hip_program_t* p,
                        const soda_hip_border_fused_desc_t* desc,
                        const void* const* code, const size_t* code_size,
                        const void* const* box_code,
                        const size_t* box_code_size,
                        soda_hip_border_fused_t** handle,
                        const FaceRule* rule) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !code || !code_size || !box_code || !box_code_size ||
      !handle)
    return fail(SODA_HIP_ERR_INVALID, "border_fused_create: NULL argument");
  const soda_hip_plan_t& plan = p->plan;
  soda_hip_border_fused_info_t info;
  bool all_wrap;
  if (int rc = fused_plan_core(&plan, desc, 0, &info, 0, nullptr, nullptr,
                               &all_wrap))
    return rc;
  bool need[4] = {false, false, false, false};   // box kernels: with strips
  if (info.num_strips)
    if (int rc = helpers_needed(plan, box_code, box_code_size, "border_fused",
                                "box", need))
      return rc;
  soda_hip_border_fused* f = new (std::nothrow) soda_hip_border_fused;
  if (!f) return fail(SODA_HIP_ERR_NOMEM, "new border_fused handle");
  f->depth = info.depth;
  soda_hip_periodic_desc_t domain = desc->border.domain;
  domain.refill_every = all_wrap ? info.depth : 1;
  int rc = create_core(kBorder, p, &domain, desc->border.mode,
                       desc->border.constant, code, code_size, &f->main, 0,
                       rule);
  for (int i = 0; i < info.num_strips && !rc; ++i) {
    const soda_hip_border_strip_t& s = info.strip[i];
    soda_hip_border_fused::Strip& mine = f->strip[i];
    soda_hip_periodic_desc_t sdom = domain;
    sdom.extent[s.dim] = s.lo + s.hi;
    rc = create_core(kBorder, p, &sdom, desc->border.mode,
                     desc->border.constant, code, code_size, &mine.h, 0, rule);
    if (rc) break;
    mine.d = s.dim;
    mine.lo = s.lo;
    mine.hi = s.hi;
    mine.take_lo = s.take_lo;
    mine.take_hi = s.take_hi;
    f->nstrips = i + 1;
  }
  if (!rc)
    rc = load_helpers(&f->box, need, box_code, "soda_box", plan.dim,
                      "border_fused", "box");
  if (rc) {
    const std::string why = last_error_text();
    soda_hip_border_fused_destroy(f);
    return fail(rc, why);
  }
  residual_boxes(info, domain.extent, plan.dim, &f->boxes);
  *handle = f;
  return SODA_HIP_OK;
}

int soda_hip_border_fused_create(soda_hip_program_t* p,
                                 const soda_hip_border_fused_desc_t* desc,
                                 const void* const* code,
                                 const size_t* code_size,
                                 const void* const* box_code,
                                 const size_t* box_code_size,
                                 soda_hip_border_fused_t** handle) {
  return fused_create(p, desc, code, code_size, box_code, box_code_size,
                      handle, nullptr);
}

int soda_hip_border_fused_destroy(soda_hip_border_fused_t* f) {
  if (!f) return SODA_HIP_OK;
  for (auto& s : f->strip) soda_hip_periodic_destroy(s.h);
  if (f->main) (void)hipSetDevice(f->main->prog->device);
  unload_helpers(&f->box);
  soda_hip_periodic_destroy(f->main);
  delete f;
  return SODA_HIP_OK;
}

int soda_hip_border_fused_info(soda_hip_border_fused_t* f,
                               soda_hip_border_fused_info_t* info) {
  if (!f || !info)
    return fail(SODA_HIP_ERR_INVALID, "border_fused_info: NULL argument");
  memset(info, 0, sizeof *info);
  if (int rc = soda_hip_periodic_info(f->main, &info->main)) return rc;
  info->depth = f->depth;
  info->num_strips = f->nstrips;
  info->scratch_bytes = info->main.scratch_bytes;
  for (int i = 0; i < f->nstrips; ++i) {
    const soda_hip_border_fused::Strip& s = f->strip[i];
    soda_hip_border_strip_t& out = info->strip[i];
    out.dim = s.d;
    out.lo = s.lo;
    out.hi = s.hi;
    out.take_lo = s.take_lo;
    out.take_hi = s.take_hi;
    for (int e = 0; e < SODA_HIP_MAX_DIM; ++e) out.extent[e] = s.h->t.n[e];
    if (int rc = soda_hip_periodic_info(s.h, &out.info)) return rc;
    info->scratch_bytes += out.info.scratch_bytes;
  }
  return SODA_HIP_OK;
}

int soda_hip_border_fused_move(soda_hip_border_fused_t* f, int32_t strip,
                               int32_t gather, void* const* main_arrays,
                               void* const* strip_arrays, int32_t count,
                               void* stream) {
  if (!f || !main_arrays || !strip_arrays)
    return fail(SODA_HIP_ERR_INVALID, "border_fused_move: NULL argument");
  const soda_hip_plan_t& plan = f->main->prog->plan;
  if (strip < 0 || strip >= f->nstrips || count < 0 ||
      count > plan.num_outputs)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused_move: no such strip, or more arrays than "
                "outputs; nothing was launched");
  int32_t elem[SODA_HIP_MAX_TENSORS];
  for (int i = 0; i < count; ++i) {
    elem[i] = plan.elem_size[plan.num_inputs + i];
    if (!main_arrays[i] || !strip_arrays[i] ||
        reinterpret_cast<uintptr_t>(main_arrays[i]) % elem[i] ||
        reinterpret_cast<uintptr_t>(strip_arrays[i]) % elem[i])
      return fail(SODA_HIP_ERR_INVALID,
                  "border_fused_move: an array is NULL or not aligned to its "
                  "cell size; nothing was launched");
  }
  HIP_TRY(hipSetDevice(f->main->prog->device));
  const soda_hip_border_fused::Strip& s = f->strip[strip];
  Box box[2];
  strip_boxes(f, s, gather != 0, &box[0], &box[1]);
  void* const* dst = gather ? strip_arrays : main_arrays;
  void* const* src = gather ? main_arrays : strip_arrays;
  return box_launch(f->box, dst, gather ? s.h->t.p : f->main->t.p,
                    const_cast<const void* const*>(src),
                    gather ? f->main->t.p : s.h->t.p, elem, count, box, 2,
                    plan.dim, static_cast<hipStream_t>(stream));
}

int soda_hip_border_fused_residual_boxes(
    const soda_hip_plan_t* plan, const soda_hip_border_fused_desc_t* desc,
    soda_hip_border_fused_boxes_t* boxes) {
  if (!boxes)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused_residual_boxes: NULL argument");
  soda_hip_border_fused_info_t info;
  bool all_wrap;
  if (int rc = fused_plan_core(plan, desc, 0, &info, 0, nullptr, nullptr,
                               &all_wrap))
    return rc;
  residual_boxes(info, desc->border.domain.extent, plan->dim, boxes);
  return SODA_HIP_OK;
}

// -- a mode and a constant per face: the _faces twins -------
// Each resolves the faces, then IS the entry it is named after on the request
// of the low faces -- all there is to a plan, whose geometry knows the wall
// dimensions only, and to a symmetric create -- or, for an asymmetric create,
// that entry's core with the faces kernels in the extend kernels' place.

// whether a create twin fills by the faces kernels; their modules, then
static int faces_serve(const FaceRule& rule, const void* const* faces_code,
                       const size_t* faces_code_size, const char* who,
                       bool* serve) {
  *serve = rule.asymmetric || (faces_forced() && faces_code && faces_code_size);
  if (*serve && (!faces_code || !faces_code_size))
    return fail(SODA_HIP_ERR_INVALID,
                std::string(who) + ": the faces differ and the faces modules "
                                   "are NULL; nothing was launched");
  return SODA_HIP_OK;
}

int soda_hip_border_plan_faces(const soda_hip_plan_t* plan,
                               const soda_hip_border_desc_t* desc,
                               const soda_hip_border_faces_t* faces,
                               int32_t iterate, soda_hip_periodic_info_t* info,
                               int32_t capacity, int32_t* chunks,
                               int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID, "border_plan_faces: NULL argument");
  FaceRule rule;
  if (int rc = border_faces(plan, desc, faces, &rule)) return rc;
  return soda_hip_border_plan(plan, &rule.low, iterate, info, capacity, chunks,
                              count);
}

int soda_hip_border_plan_batch_faces(const soda_hip_plan_t* plan,
                                     const soda_hip_border_desc_t* desc,
                                     const soda_hip_border_faces_t* faces,
                                     int32_t batch, int32_t iterate,
                                     soda_hip_periodic_info_t* info,
                                     int32_t capacity, int32_t* chunks,
                                     int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID,
                "border_plan_batch_faces: NULL argument");
  if (int rc = check_domain_batch(*plan, batch, "border_plan_batch_faces"))
    return rc;
  FaceRule rule;
  if (int rc = border_faces(plan, desc, faces, &rule)) return rc;
  return soda_hip_border_plan_batch(plan, &rule.low, batch, iterate, info,
                                    capacity, chunks, count);
}

int soda_hip_border_create_faces(soda_hip_program_t* p,
                                 const soda_hip_border_desc_t* desc,
                                 const soda_hip_border_faces_t* faces,
                                 const void* const* code,
                                 const size_t* code_size,
                                 const void* const* faces_code,
                                 const size_t* faces_code_size,
                                 soda_hip_border_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !handle)
    return fail(SODA_HIP_ERR_INVALID, "border_create_faces: NULL argument");
  FaceRule rule;
  if (int rc = border_faces(&p->plan, desc, faces, &rule)) return rc;
  bool serve;
  if (int rc = faces_serve(rule, faces_code, faces_code_size,
                           "border_create_faces", &serve))
    return rc;
  if (!serve)
    return soda_hip_border_create(p, &rule.low, code, code_size, handle);
  bool all_wrap;
  if (int rc = border_modes(&p->plan, &rule.low, &all_wrap)) return rc;
  soda_hip_periodic_desc_t domain = rule.low.domain;
  if (!all_wrap && domain.refill_every == 0) domain.refill_every = 1;
  return create_core(kBorder, p, &domain, rule.low.mode, rule.low.constant,
                     faces_code, faces_code_size, handle, 0, &rule);
}

int soda_hip_border_create_batch_faces(soda_hip_program_t* p,
                                       const soda_hip_border_desc_t* desc,
                                       const soda_hip_border_faces_t* faces,
                                       int32_t batch, const void* const* code,
                                       const size_t* code_size,
                                       const void* const* faces_code,
                                       const size_t* faces_code_size,
                                       soda_hip_border_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !handle)
    return fail(SODA_HIP_ERR_INVALID,
                "border_create_batch_faces: NULL argument");
  if (int rc = check_domain_batch(p->plan, batch, "border_create_batch_faces"))
    return rc;
  FaceRule rule;
  if (int rc = border_faces(&p->plan, desc, faces, &rule)) return rc;
  bool serve;
  if (int rc = faces_serve(rule, faces_code, faces_code_size,
                           "border_create_batch_faces", &serve))
    return rc;
  if (!serve)
    return soda_hip_border_create_batch(p, &rule.low, batch, code, code_size,
                                        handle);
  bool all_wrap;
  if (int rc = border_modes(&p->plan, &rule.low, &all_wrap)) return rc;
  soda_hip_periodic_desc_t domain = rule.low.domain;
  if (!all_wrap && domain.refill_every == 0) domain.refill_every = 1;
  return create_core(kBorder, p, &domain, rule.low.mode, rule.low.constant,
                     faces_code, faces_code_size, handle, batch, &rule);
}

int soda_hip_border_fused_plan_faces(const soda_hip_plan_t* plan,
                                     const soda_hip_border_fused_desc_t* desc,
                                     const soda_hip_border_faces_t* faces,
                                     int32_t iterate,
                                     soda_hip_border_fused_info_t* info,
                                     int32_t capacity, int32_t* chunks,
                                     int32_t* count) {
  if (!plan || !desc)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused_plan_faces: NULL argument");
  FaceRule rule;
  if (int rc = border_faces(plan, &desc->border, faces, &rule)) return rc;
  soda_hip_border_fused_desc_t low = *desc;
  low.border = rule.low;
  return soda_hip_border_fused_plan(plan, &low, iterate, info, capacity,
                                    chunks, count);
}

int soda_hip_border_fused_create_faces(
    soda_hip_program_t* p, const soda_hip_border_fused_desc_t* desc,
    const soda_hip_border_faces_t* faces, const void* const* code,
    const size_t* code_size, const void* const* box_code,
    const size_t* box_code_size, const void* const* faces_code,
    const size_t* faces_code_size, soda_hip_border_fused_t** handle) {
  if (handle) *handle = nullptr;
  if (!p || !desc || !handle)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused_create_faces: NULL argument");
  FaceRule rule;
  if (int rc = border_faces(&p->plan, &desc->border, faces, &rule)) return rc;
  bool serve;
  if (int rc = faces_serve(rule, faces_code, faces_code_size,
                           "border_fused_create_faces", &serve))
    return rc;
  soda_hip_border_fused_desc_t low = *desc;
  low.border = rule.low;
  if (!serve)
    return soda_hip_border_fused_create(p, &low, code, code_size, box_code,
                                        box_code_size, handle);
  return fused_create(p, &low, faces_code, faces_code_size, box_code,
                      box_code_size, handle, &rule);
}

int soda_hip_border_fused_residual_boxes_faces(
    const soda_hip_plan_t* plan, const soda_hip_border_fused_desc_t* desc,
    const soda_hip_border_faces_t* faces,
    soda_hip_border_fused_boxes_t* boxes) {
  if (!plan || !desc || !boxes)
    return fail(SODA_HIP_ERR_INVALID,
                "border_fused_residual_boxes_faces: NULL argument");
  FaceRule rule;
  if (int rc = border_faces(plan, &desc->border, faces, &rule)) return rc;
  soda_hip_border_fused_desc_t low = *desc;
  low.border = rule.low;
  return soda_hip_border_fused_residual_boxes(plan, &low, boxes);
}

// -- the entries every kind of handle has -----------
// soda_hip_<KIND>_fill, and the six run entries of soda_hip_<KIND>_t: each its
// NULL arguments refused under its own name, then the core on the handle's
// Domain.

#define SODA_DOMAIN_FILL_ENTRY(KIND)                                          \
  int soda_hip_##KIND##_fill(soda_hip_##KIND##_t* h, void* const* arrays,     \
                             int32_t count, void* stream) {                   \
    if (!h || !arrays)                                                        \
      return fail(SODA_HIP_ERR_INVALID, #KIND "_fill: NULL argument");        \
    return fill_core(h, arrays, count, stream);                               \
  }

#define SODA_DOMAIN_RUN_ENTRIES(KIND)                                         \
  int soda_hip_##KIND##_run_padded(soda_hip_##KIND##_t* h,                    \
                                   void* const* outputs,                      \
                                   const void* const* inputs,                 \
                                   int32_t iterate, void* stream) {           \
    if (!h || !outputs || !inputs)                                            \
      return fail(SODA_HIP_ERR_INVALID, #KIND "_run_padded: NULL argument");  \
    return run_padded_core(domain_of(h), outputs, inputs, iterate, stream);   \
  }                                                                           \
  int soda_hip_##KIND##_run_device(soda_hip_##KIND##_t* h,                    \
                                   void* const* outputs,                      \
                                   const void* const* inputs,                 \
                                   int32_t iterate, void* stream) {           \
    if (!h || !outputs || !inputs)                                            \
      return fail(SODA_HIP_ERR_INVALID, #KIND "_run_device: NULL argument");  \
    return run_device_core(domain_of(h), outputs, inputs, iterate, stream);   \
  }                                                                           \
  int soda_hip_##KIND##_run_padded_residual(                                  \
      soda_hip_##KIND##_t* h, void* const* outputs,                           \
      const void* const* inputs, int32_t iterate, void* residual_dev,         \
      void* stream) {                                                         \
    if (!h || !outputs || !inputs || !residual_dev)                           \
      return fail(SODA_HIP_ERR_INVALID,                                       \
                  #KIND "_run_padded_residual: NULL argument");               \
    return run_padded_residual_core(domain_of(h), nullptr, outputs, inputs,   \
                                    iterate, residual_dev, stream);           \
  }                                                                           \
  int soda_hip_##KIND##_run_padded_norms(                                     \
      soda_hip_##KIND##_t* h, soda_hip_norms_handle_t* norms,                 \
      void* const* outputs, const void* const* inputs, int32_t iterate,       \
      void* acc_dev, void* stream) {                                          \
    if (!h || !norms || !outputs || !inputs || !acc_dev)                      \
      return fail(SODA_HIP_ERR_INVALID,                                       \
                  #KIND "_run_padded_norms: NULL argument");                  \
    return run_padded_residual_core(domain_of(h), norms, outputs, inputs,     \
                                    iterate, acc_dev, stream);                \
  }                                                                           \
  int soda_hip_##KIND##_run_until(                                            \
      soda_hip_##KIND##_t* h, void* const* outputs,                           \
      const void* const* inputs, int32_t max_iterate, int32_t check_every,    \
      double tol, uint64_t int_tol, soda_hip_residual_t* result_host,         \
      int32_t* iterations_done, void* stream) {                               \
    if (!h || !outputs || !inputs)                                            \
      return fail(SODA_HIP_ERR_INVALID, #KIND "_run_until: NULL argument");   \
    return until_residual(domain_of(h), outputs, inputs, max_iterate,         \
                          check_every, tol, int_tol, result_host,             \
                          iterations_done, stream);                           \
  }                                                                           \
  int soda_hip_##KIND##_run_until_norm(                                       \
      soda_hip_##KIND##_t* h, soda_hip_norms_handle_t* norms,                 \
      void* const* outputs, const void* const* inputs, int32_t max_iterate,   \
      int32_t check_every, int32_t which, double tol,                         \
      soda_hip_norms_t* result_host, int32_t* iterations_done,                \
      void* stream) {                                                         \
    if (!h || !norms || !outputs || !inputs)                                  \
      return fail(SODA_HIP_ERR_INVALID,                                       \
                  #KIND "_run_until_norm: NULL argument");                    \
    return until_norm(domain_of(h), norms, outputs, inputs, max_iterate,      \
                      check_every, which, tol, result_host, iterations_done,  \
                      stream);                                                \
  }

SODA_DOMAIN_FILL_ENTRY(periodic)
SODA_DOMAIN_FILL_ENTRY(border)
SODA_DOMAIN_RUN_ENTRIES(periodic)
SODA_DOMAIN_RUN_ENTRIES(border)
SODA_DOMAIN_RUN_ENTRIES(border_fused)

#undef SODA_DOMAIN_FILL_ENTRY
#undef SODA_DOMAIN_RUN_ENTRIES

}  // extern "C"
