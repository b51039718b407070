"""Lowering of a Stencil to gfx950 HIP kernels + a launch plan.

What the reference's HLS emitter does for an FPGA (reference
src/soda/codegen/xilinx/hls_kernel.py:338-410 `print_code`, :665-886
`print_module_definition`; src/soda/dataflow.py:336-625) is done here for a
GPU.  Four families of kernels are generated:

`direct`   one kernel per stage, 16 bytes' worth of cells per thread, parents
           read straight from global memory into per-thread row buffers
           (L1/L2 give the reuse between threads).  Handles every program
           the front-end accepts (1-4 dimensions, any DAG); locals live in
           HBM scratch.  It is the correctness baseline and the fallback.

`march2d`  2-D programs.  One wavefront owns a strip of 64*V columns and
           marches along dimension 1 (the dimension SODA streams).  Every
           tensor of the -- possibly T-times unrolled -- stage chain keeps a
           sliding window of rows in REGISTERS; neighbours along dimension 0
           come from adjacent lanes by lane shifts (DPP, or DPP down and
           ds_swizzle up: default_lane_shift); inputs arrive by one
           coalesced 16-byte load per lane per row, PF rows ahead of use;
           only the last iteration's outputs are stored.  That is SODA's own
           micro-architecture (line buffers chained through all iterations so
           DRAM is touched once; reference core.py:338-369, README.md:155-156)
           mapped onto a wavefront: the FIFOs become registers, the `unroll
           factor` PEs become 64*V lanes, and `iterate` stages fused in one
           pipeline become T fused iterations per launch (temporal blocking).
           Unless a block shares x-halos (xshare) or fused iterations (pipe)
           through LDS, waves never talk to each other: the halo a strip
           needs is recomputed by overlapping strips/chunks.
           (`march3d` does the same for 3-D programs with a tile of rows
           per wave.)

`ldswin`   one-stage 2-D programs with windows many cells wide (contrast):
           the window rows live in an LDS ring that a block's waves fill
           together, every lane computes 8 cells, no lane shifts.

`tile3d`   3-D programs, on request only: a block marches a tile along
           dimension 2 with the planes of every fused level in LDS rings, so
           the fusion depth is bounded by LDS, not by registers (tile3d.py).

Floating-point results are bit-identical to the CPU oracle because the kernels
compile the same C expression text with -ffp-contract=off.

Layout of the package: module.py (Module, descriptors, the device runtime
text), march_schedule.py and march.py (`march2d` / `march3d`: what a kernel is,
built in named steps, and its text), ldswin.py, tile3d.py, direct.py; this
file holds the options and `lower()`, which picks the family and the shape
 in named steps: check_options, _lower_ldswin, _derive,
_add_march_passes (the shape from _one_iteration_shape, every kernel a
march_config added by _add_march) or `direct`, _add_tile3d_passes.
"""
import dataclasses
import itertools
import os
from typing import Dict, Optional, Sequence, Union

from soda_amd import core, util

from soda_amd.codegen.hip.module import (KernelDesc, Module, PassDesc,  # noqa: F401
                                         _check_native, runtime_text)
from soda_amd.codegen.hip import residual
from soda_amd.codegen.hip.direct import DIRECT_BLOCK, add_direct_pass  # noqa: F401
from soda_amd.codegen.hip.ldswin import (add_ldswin_pass,  # noqa: F401
                                         ldswin_candidate, ldswin_pays,
                                         ldswin_supported)
from soda_amd.codegen.hip.march import (LANE_SHIFTS, MAX_FUSE_3D,  # noqa: F401
                                        MAX_FUSE_PRESERVE, MAX_SHIFT_TEMPS,
                                        MAX_UNROLL, REG_BUDGET, MarchConfig,
                                        add_march_pass, add_march_twin,
                                        default_vec,
                                        march_supported)
from soda_amd.codegen.hip.tile3d import (add_tile3d_pass,  # noqa: F401
                                         tile3d_supported)

# ---------------------------------------------------------------------------
# whole module
# ---------------------------------------------------------------------------

MAX_TENSORS = 16       # SODA_HIP_MAX_TENSORS (include/soda_hip.h)
# The fusion depths iterated programs are offered by default -- ONE definition
# for `sodac --hip-fuse`, bench.py, __graft_entry__.prebuild_list and the parity
# tests of the benched schedule (tests/test_hip_parity.py): the library mixes
# them per extent (jacobi2d 8192^2 x 100 = 4 x T13 + 4 x T12).
DEFAULT_FUSE = (13, 12, 8, 4)
# integer sums along the streamed dimension as sliding sums in the marching
# kernels (march.py `slide`) instead of power-of-two chains (SODA_HIP_SLIDE=0/1)
SLIDING_SUMS = os.environ.get('SODA_HIP_SLIDE', '1') != '0'


# kernel families lower() can be asked for (LowerOptions.strategy)
STRATEGIES = ('auto', 'direct', 'march', 'ldswin', 'tile3d')


@dataclasses.dataclass(kw_only=True, eq=False)
class LowerOptions:
  """Knobs of the HIP backend (command-line spelling: --hip-*).  `None` means
  "the measured default for this program's dimensionality" (profiles/
  r01_sweeps.md): 2-D strips prefetch 2 rows with non-temporal loads (every
  input row is used by one wave only); 3-D tiles re-read their halo rows, so
  they use plain loads (the overlap then hits in L2), prefetch 1 plane and hold
  4 output rows per wave to stay under 128 VGPRs."""

  strategy: str = 'auto'        # one of STRATEGIES
  fuse: Sequence[int] = (4,)    # temporal-blocking depths to generate
  vec: Optional[int] = None
  chunk_rows: Optional[int] = None
  prefetch: Optional[int] = None
  waves_x: int = 1
  waves_y: int = 1
  # Cache hints, measured on MI355X with buffers ping-ponging as in a real
  # iterated run (tools/sweep.py --launches N): inputs are read once per
  # launch, so their loads are non-temporal; the outputs are the next
  # launch's inputs, so their stores are plain.
  nt_store: Optional[bool] = None
  nt_load: Optional[bool] = None
  xcd_swizzle: bool = True
  edge_loads: bool = True
  tile_rows: Optional[int] = None
  # 'dpp' or 'mixh' (march.LANE_SHIFTS); None: default_lane_shift
  lane_shift: Optional[str] = None
  min_waves: int = 0
  occupancy: int = 0
  # waves of a block sharing the fused iterations of a 2-D kernel; None =
  # default_pipe(fusion depth)
  pipe: Optional[int] = None
  pipe_rows: int = 2
  # estimated VGPRs a marching shape may need before _one_iteration_shape
  # moves on to a leaner one (None: REG_BUDGET)
  reg_budget: Optional[int] = None
  stamps: bool = False
  # trips of the unrolled loop whose warm-up is peeled into straight-line
  # code without the stages that do not matter yet: an int for every fusion
  # depth, a dict {depth: trips}, -1 = all of the warm-up, None = let
  # runtime.select_peel choose per kernel from the compiled register counts
  # (lower() itself treats None as -1)
  peel: Union[None, int, Dict[int, int]] = None
  # valid lanes of a strip as a multiple of this; None: as many as make a
  # strip's output rows start on 64-byte boundaries where they are written
  # with non-temporal stores, else 1.  SODA_HIP_ALIGN_LANES overrides None
  # for A/B runs
  align_lanes: Optional[int] = None
  # fused 3-D kernels whose block covers the whole row, x-halos handed over
  # through LDS (MarchConfig.xshare).  Needs the row length the program will
  # run on (`row_cells` = extent[0]; runtime.Program fills it in from its
  # extent): the kernels then REFUSE any other row length at launch.
  # None: where it applies (3-D, fused, <= 4 waves per row); True also in
  # 2-D; SODA_HIP_XSHARE=0/1 overrides for A/B runs
  xshare: Optional[bool] = None
  row_cells: Optional[int] = None
  # segmented x-halo sharing (MarchConfig.xshare_block): the fused kernels'
  # blocks are this many waves (2..16) side by side on a SEGMENT of the row,
  # x-halos shared through LDS inside it, overlap only between blocks.  Needs
  # no row length and runs any; wins over xshare / row_cells.  The
  # one-iteration kernel takes the form only if `xshare` is True as well (as
  # it shares whole rows only on request).  None: not used (`auto` never
  # picks it); SODA_HIP_XSHARE_BLOCK=B overrides for A/B runs
  xshare_block: Optional[int] = None
  # long integer window reductions (erosion's 19-tap min, xcorr's 19-tap
  # sums) as chains of power-of-two windows: 6 instead of 18 operations per
  # cell, bit-exact (optimization/windows.py).  SODA_HIP_WINDOWS=0/1
  # overrides for A/B runs
  windows: Optional[bool] = None
  # locals read only at the cell being computed are folded into their
  # consumers (optimization/pointwise.py): denoise3d is 4 tensors instead
  # of 10.  SODA_HIP_INLINE=0/1 overrides for A/B runs
  inline: Optional[bool] = None
  # `tile3d`: cells along x (a multiple of 64) and rows along y of a block's
  # LDS tile, ghost cells included, and the waves of the block (they divide
  # the rows); None: tile3d.py picks (64 cells, the height its LDS rule
  # allows, 8 / 4 / 2 / 1 waves)
  tile3d_w: Optional[int] = None
  tile3d_h: Optional[int] = None
  tile3d_waves: Optional[int] = None
  # the banked form of a wire stream's dense program (stream.py
  # `dense_banked`): {input or output: 2 or 4}, the tensor is that many banks
  # the marching kernels address themselves (MarchConfig.banks), and
  # {input: elements} the kernels start into the banks of a delayed input.
  # `march2d` / `march3d` only: a program that lowers to another family, or to
  # stage-pipelined blocks, is refused with a SemanticError
  banks: Optional[Dict[str, int]] = None
  bank_lead: Optional[Dict[str, int]] = None
  # batched kernels in every family (Module._batched, soda_rt_batch.h): a
  # launch of (blocks, batch, 1) runs `batch` independent grids of one extent,
  # item after item in every tensor (soda_hip_run_device_batch; the one-grid
  # entries refuse such a program's kernels nothing, they run them as batch
  # 1).  For callers and A/B runs: `auto` never sets it, no environment
  # override.  Not with `banks`
  batch: bool = False
  # residual of a run's last iteration (residual.py): every
  # default kernel is emitted unchanged; beside the marching kernels come
  # twins (`_rs`) that take |cur - prev| of the last fused iteration where they
  # store, and every module gets `<app>_residual` for the families and depths
  # without one (soda_hip_run_device_residual / _until).  For callers: `auto`
  # never sets it, no environment override.  Iterable programs only; not with
  # `batch`, not with `banks`
  residual: bool = False

  def __post_init__(self):
    self.fuse = tuple(self.fuse)
    if self.inline is None:
      self.inline = os.environ.get('SODA_HIP_INLINE', '1') != '0'
    if self.windows is None:
      self.windows = os.environ.get('SODA_HIP_WINDOWS', '1') != '0'
    if self.xshare is None and os.environ.get('SODA_HIP_XSHARE'):
      self.xshare = os.environ['SODA_HIP_XSHARE'] == '1'
    if self.xshare_block is None and os.environ.get('SODA_HIP_XSHARE_BLOCK'):
      self.xshare_block = int(os.environ['SODA_HIP_XSHARE_BLOCK'])
    if self.align_lanes is None and os.environ.get('SODA_HIP_ALIGN_LANES'):
      self.align_lanes = int(os.environ['SODA_HIP_ALIGN_LANES'])

  def resolved(self, dim: int, iterated: bool = True) -> 'LowerOptions':
    out = dataclasses.replace(self)
    if out.prefetch is None and dim == 3:
      out.prefetch = 1
    # 2-D: resolved per fusion depth in lower() (default_prefetch)
    # Cache hints.  Iterated programs (buffers ping-pong): inputs are read once
    # per launch -> non-temporal loads; outputs are the next launch's inputs ->
    # plain stores.  One-shot programs (iterate 1, e.g. blur): the output is
    # not re-read -> non-temporal stores, plain loads (blur 16384^2: 232 us vs
    # 294 us with the iterated defaults).  3-D tiles re-read halo rows -> plain
    # loads either way.
    if out.nt_load is None:
      out.nt_load = dim != 3 and iterated
    if out.nt_store is None:
      out.nt_store = not iterated
    if out.tile_rows is None:
      out.tile_rows = 4
    return out


# operations per cell (as written) between which a one-iteration 2-D program
# of fp32 cells runs on narrow strips (prefers_narrow_strips)
NARROW_STRIP_OPS = (48, 128)


def ops_per_cell(stencil: core.Stencil) -> int:
  """Arithmetic per cell of one iteration AS WRITTEN (the rewrites of _derive
  fold and split statements; what the shape choice wants to know is how much
  the program computes)."""
  from soda_amd import ir as _ir
  return sum(_ir.op_count(s.stmt.expr) +
             sum(_ir.op_count(l.expr) for l in s.stmt.let)
             for s in stencil.ordered_stages)


def prefers_narrow_strips(stencil: core.Stencil) -> bool:
  """One iteration per launch of a 2-D program that computes for 50-130
  operations per fp32 cell (denoise2d: 55): the kernel is bound by neither
  HBM nor the load queue but by how many waves can take turns, so 8 bytes per
  lane with 4 rows in flight (80 registers, six waves per SIMD) beat the usual
  16 bytes with 8 rows (127 registers, four waves): denoise2d 8192^2 171.6 /
  170.6 us -> 164.2 / 164.2 at 8 bytes per lane -> 157.9 with 4 rows in flight
  as well (4 bytes per lane 197.5; 16 bytes with 4 rows 168.0; 12 rows 176.6;
  profiles/r05_denoise_shapes.jsonl, one process; sustained over 900 launches
  each, alternating: 163.6 against 151.8 us, r05_denoise_sustained.json).
  Above the band a program goes through `ldswin` or takes 2 rows in flight
  (_one_iteration_shape); below it the loads are what a wave waits for.  fp32
  cells only: that is what was measured.  runtime.resolve_options applies it
  where the caller fixed neither the cells per lane nor the prefetch depth."""
  if os.environ.get('SODA_HIP_NARROW', '1') == '0':
    return False
  if stencil.dim != 2 or stencil.iterate != 1:
    return False
  if any(str(t) != 'float' for t in stencil.symbol_table.values()):
    return False
  return NARROW_STRIP_OPS[0] <= ops_per_cell(stencil) < NARROW_STRIP_OPS[1]


def default_pipe(fused_iters: int) -> int:
  """Waves of a block that share the fused iterations of a 2-D kernel
  (MarchConfig.pipe).  One: in kernel sweeps four waves with three iterations
  each beat one wave with twelve by 5-10 % (jacobi2d T=12 on 8192 x {8192, 4296,
  2248, 1224}: 148 vs 156, 91 vs 102, 65 vs 70, 44 vs 47 us), but in the
  sustained 9-launch steps of bench.py on one box they do not (1.383 vs 1.357
  ms on 8192^2; 0.552 vs 0.603 ms on a 4-GPU slab, 0.419 vs 0.399 ms on an
  8-GPU slab).  `--hip-pipe 4` selects them."""
  return 1


def default_lane_shift(fused_iters: int, dim: int) -> str:
  """How a lane gets its neighbours' cells.  One iteration to a few per launch:
  DPP whole-wave shifts, folded into the consuming add.  Deep 2-D fusion
  (T >= 8): 'mixh' -- the two directions on two different pipes, down through
  DPP (vector ALU), up through ds_swizzle (the LDS crossbar), on 32-lane half
  strips.  A DPP-carrying instruction costs the issuing SIMD ~4-8 cycles, a
  swizzle occupies the CU's shared LDS pipe; all of either kind is the same
  speed (T=12: 148.3 / 148.5 us), half of each is faster although a half strip
  has fewer valid lanes, and needs 11 registers less, which buys two more rows
  in flight (profiles/r03_sweep_mixh_*.json, jacobi2d, us per launch, dpp ->
  mixh: T=12 on 8192^2 146.3 -> 136.2, on the 4296- / 1224-row slabs of a 2- /
  8-GPU run 89.4 -> 79.7 / 39.1 -> 34.8; T=8 114.3 -> 114.0, 31.9 -> 29.7;
  T=4 100.4 -> 101.1, 19.5 -> 20.0: DPP stays)."""
  return 'mixh' if dim == 2 and fused_iters >= 8 else 'dpp'


def default_prefetch(fused_iters: int, lane_shift: str = 'dpp') -> int:
  """Rows a 2-D marching wave keeps in flight ahead of the one it computes.
  With the loop body branch-free (buffer addressing) the depth is real:
  jacobi2d 8192^2, one iteration per launch, 99.9 / 94.0 / 92.6 / 90.9 us at
  depth 1 / 2 / 4 / 8; the fused kernels have less to hide and fewer registers
  to spare (T=8: 116 us at 4 vs 119 at 2; T=12 with DPP shifts: 149 at 2 vs
  153 at 4; with 'mixh' shifts, 11 registers leaner: 149.6 at 2, 136.2 at 4)."""
  if fused_iters <= 2:
    return 8
  if fused_iters <= 8 or lane_shift == 'mixh':
    return 4
  return 2


# ---------------------------------------------------------------------------
# the steps of lower(), in the order it takes them
# ---------------------------------------------------------------------------

def check_options(stencil: core.Stencil, opts: LowerOptions) -> None:
  """Refuses what no family can build, before anything is built; `opts` are
  resolved.  A call that breaks two rules hears the first one here."""
  if opts.strategy not in STRATEGIES:
    raise util.SemanticError('strategy %r: one of %s' %
                             (opts.strategy, ', '.join(STRATEGIES)))
  if opts.lane_shift is not None and opts.lane_shift not in LANE_SHIFTS:
    raise util.SemanticError('lane_shift %r: None or one of %s' %
                             (opts.lane_shift, ', '.join(LANE_SHIFTS)))
  if opts.xshare_block is not None and not 2 <= opts.xshare_block <= 16:
    raise util.SemanticError('xshare_block %r: None or 2 to 16 waves per block'
                             % (opts.xshare_block,))
  if (opts.pipe or 1) > 1 and (
      not isinstance(opts.pipe_rows, int) or opts.pipe_rows < 1 or
      opts.pipe_rows & (opts.pipe_rows - 1)):
    # (refused here, whatever the strategy: the marching generator's own
    # refusal is caught by _add_march, and _add_march_passes would drop the
    # fused depth and hand back the one-iteration kernel without a word)
    raise util.SemanticError(
        'pipe_rows %r: the row steps per barrier of a stage-pipelined block '
        '(pipe %d) are a power of two' % (opts.pipe_rows, opts.pipe))
  if opts.batch and opts.banks:
    raise util.SemanticError(
        'batch: the wire format has no batch, `banks` cannot be combined with '
        'it')
  if opts.residual:
    residual.check_options(stencil, opts.batch, opts.banks)
  _check_native(stencil)
  stencil.check_preserve()
  if opts.banks and opts.strategy not in ('auto', 'march'):
    raise util.SemanticError('banks: `%s` kernels read and write dense arrays'
                             % opts.strategy)
  if opts.strategy == 'tile3d' and tile3d_supported(stencil):
    raise util.SemanticError('tile3d: %s' % tile3d_supported(stencil))


def same_boxes(a: core.Stencil, b: core.Stencil) -> bool:
  """A rewrite must leave the outputs' windows alone: they decide the valid
  box and, under `border: preserve`, which cells an iteration computes.  A
  tensor's window includes the tensor's own cell (core.iteration_boxes), so
  folding a local that is STORED off-centre can widen what its consumer may
  compute (`loc(0, -1) = in(1, 0); out(0, 0) = loc(0, -1)`: row 0 of `out`
  needs row -1 of `loc`; folded, it needs nothing outside the grid -- found
  by tools/fuzz_scan.py options, a preserved row computed instead)."""
  mine, theirs = a.iteration_boxes(), b.iteration_boxes()
  return all(mine[o] == theirs[o] for o in a.output_names)


def _lower_ldswin(stencil: core.Stencil,
                  opts: LowerOptions) -> Optional[Module]:
  """Wide 2-D windows through an LDS row ring (ldswin.py): a whole stage per
  thread, so every pointwise local -- the groups of a rebalanced sum included
  -- is a sub-expression there.  On request, and by itself where it pays
  (contrast: one input, 17 x 17 taps, 393 operations per cell).  None where
  `auto` does not take the family; an explicit `ldswin` hears why not."""
  if opts.strategy in ('auto', 'ldswin') and stencil.dim == 2 and \
      os.environ.get('SODA_HIP_LDSWIN', '1') != '0' and \
      (opts.strategy == 'ldswin' or ldswin_candidate(stencil)):
    from soda_amd.optimization import pointwise
    # (`auto`: a finite cap on the folded expression -- a local read k times
    # at one index is duplicated k times per level; contrast folds to ~400)
    whole = pointwise.inline_pointwise(
        stencil, fold_groups=True,
        max_ops=1 << 20 if opts.strategy == 'ldswin' else 1 << 13)
    if same_boxes(stencil, whole) and (
        (opts.strategy == 'ldswin' and ldswin_supported(whole) is None) or
        (opts.strategy == 'auto' and ldswin_pays(whole) and
         (opts.vec is None or opts.vec % 4 == 0))):
      if opts.banks:
        raise util.SemanticError(
            'banks: `ldswin` kernels read and write dense arrays')
      mod = Module(whole, batch=opts.batch, residual=opts.residual)
      try:
        add_ldswin_pass(mod, chunk=opts.chunk_rows or 64,
                        step=opts.waves_y if opts.waves_y > 1 else None)
        if opts.residual:
          residual.add_residual_kernel(mod)
        return mod
      except util.SemanticError:
        # the ring does not fit LDS (window too tall / too wide): only an
        # explicit `ldswin` request hears about it, `auto` moves on to the
        # marching / direct kernels with the program as written
        if opts.strategy == 'ldswin':
          raise
  if opts.strategy == 'ldswin':
    raise util.SemanticError('ldswin: %s' % (
        ldswin_supported(stencil) or 'the program does not fold to one stage'))
  return None


def _derive(stencil: core.Stencil, opts: LowerOptions) -> core.Stencil:
  """The program the marching / direct / tile3d kernels are built from, a
  DERIVED one: same tensors the caller sees (inputs, outputs, their windows
  and boxes), other locals."""
  if opts.inline:
    from soda_amd.optimization import pointwise
    folded = pointwise.inline_pointwise(stencil)
    if same_boxes(stencil, folded):
      stencil = folded
  if opts.windows:
    from soda_amd.optimization import windows
    # (the marching kernels reduce dimension-0 windows themselves, all cells
    # of a lane jointly; `direct` kernels get chains in every dimension)
    marching = opts.strategy in ('auto', 'march', 'tile3d') and \
        march_supported(stencil) is None
    skip = ()
    if marching:
      skip = ((0, None),) + (((stencil.dim - 1, '+'),) if SLIDING_SUMS else ())
    derived = windows.decompose(stencil, skip=skip)
    # (the auxiliaries are tensors of the launch plan: a program that would
    # exceed the argument block's slots keeps its windows as written)
    if len(derived.symbol_table) + len(derived.param_stmts) <= MAX_TENSORS \
        and same_boxes(stencil, derived):
      stencil = derived
  # operations whose operand ranges the text proves: cheaper sequences with
  # the same bits (exact.py; the program as written unless one is enabled)
  from soda_amd.codegen.hip import exact
  return exact.specialize(stencil)


def peel_for(opts: LowerOptions, t: int) -> int:
  """Trips of the warm-up the kernel of fusion depth `t` peels."""
  if opts.peel is None:
    return -1
  if isinstance(opts.peel, dict):
    return int(opts.peel.get(t, -1))
  return int(opts.peel)


def pipe_for(opts: LowerOptions, t: int) -> int:
  """Waves that share the `t` fused iterations: what was asked for (else
  default_pipe) where it divides them and the block is one wave otherwise,
  else quietly 1."""
  want = default_pipe(t) if opts.pipe is None else opts.pipe
  ok = (want > 1 and t > 1 and t % want == 0 and
        opts.waves_x * opts.waves_y == 1)
  return want if ok else 1


def shift_for(opts: LowerOptions, dim: int, t: int, xshare: int = 0) -> str:
  """The lane shifts of the kernel of depth `t`: as asked, else DPP for blocks
  of several waves (x-halo sharing, stage pipelines, waves_x / waves_y), else
  default_lane_shift."""
  if opts.lane_shift is not None:
    return opts.lane_shift
  if xshare or pipe_for(opts, t) > 1 or opts.waves_x * opts.waves_y != 1:
    return 'dpp'
  return default_lane_shift(t, dim)


def march_config(opts: LowerOptions, stencil: core.Stencil, t: int, vec: int,
                 pf: Optional[int], rows: Optional[int] = None,
                 xshare: int = 0, xshare_block: int = 0) -> MarchConfig:
  """The marching kernel of `t` fused iterations at `vec` cells per lane, `pf`
  rows in flight (None: default_prefetch) and `rows` rows per 3-D tile."""
  shift = shift_for(opts, stencil.dim, t, xshare or xshare_block)
  if pf is None:
    pf = default_prefetch(t, shift)
  align = opts.align_lanes
  if align is None:
    out_bytes = min(o.size_in_bytes for o in stencil.output_types)
    align = max(1, 64 // (vec * out_bytes)) if opts.nt_store else 1
  cfg = MarchConfig(
      fused_iters=t, vec=vec, chunk_rows=opts.chunk_rows or 64,
      prefetch=pf, waves_x=opts.waves_x, waves_y=opts.waves_y,
      nt_store=opts.nt_store, nt_load=opts.nt_load,
      xcd_swizzle=opts.xcd_swizzle, edge_loads=opts.edge_loads,
      tile_rows=rows or opts.tile_rows, lane_shift=shift,
      min_waves=opts.min_waves, occupancy=opts.occupancy,
      pipe=pipe_for(opts, t), pipe_rows=opts.pipe_rows, stamps=opts.stamps,
      peel=peel_for(opts, t), align_lanes=align, xshare=xshare,
      xshare_block=xshare_block,
      xwindow=bool(opts.windows),
      slide=bool(opts.windows) and SLIDING_SUMS,
      banks=opts.banks, bank_lead=opts.bank_lead)
  cfg.chunk_fixed = opts.chunk_rows is not None
  return cfg


def _fuse_depths(stencil: core.Stencil, opts: LowerOptions):
  """Fusion depths of the marching kernels, deepest first: each requested
  depth, clipped to the iteration count the program asks for (a 2-iteration
  program gets a T=2 kernel, not T=4) and, in 3-D, to MAX_FUSE_3D: a tile of
  rows x planes per tensor per fused iteration; two iterations still fit
  (heat3d 512^3: 118-125 us per iteration at T=2, 260 VGPRs, against 194 us at
  T=1; T=3 with 2 cells per lane: 129 us)."""
  if opts.strategy == 'tile3d':
    # the fused passes are tile3d's (_add_tile3d_passes); the marching family
    # supplies the one-iteration pass, as under `auto`
    return []
  iterable = (len(stencil.input_names) == len(stencil.output_names) and
              stencil.input_types == stencil.output_types)
  cap = stencil.iterate
  if stencil.dim == 3 and opts.strategy != 'march':
    cap = min(cap, MAX_FUSE_3D)
  if stencil.preserve_border and opts.strategy != 'march':
    # every fused iteration also keeps the window of the tensor it preserves
    # the border from: jacobi2d T=12 needs 186 VGPRs (2 waves per SIMD) and
    # runs 96 iterations in 2.51 ms, T=8 in 2.04 ms (1.54 / 1.61 ms without
    # preserve)
    cap = min(cap, MAX_FUSE_PRESERVE)
  return sorted({min(t, cap) for t in opts.fuse if iterable} - {0, 1},
                reverse=True)


def _one_iteration_shape(stencil: core.Stencil, opts: LowerOptions, work: int,
                         budget: int):
  """((cells per lane, prefetch depth, rows per tile) or None, the last
  refusal or None) of the one-iteration kernel, which is mandatory.  Tall
  windows (erosion and xcorr read 19 rows) or many live tensors may not fit
  the register budget at the preferred shape: try shallower prefetch, then
  fewer cells per lane, and take the first shape whose estimate stays within
  `budget` (else the leanest, the earlier of two alike); None if the
  generator refuses them all -- lower() then falls back to `direct` kernels,
  or raises the refusal where `march` was asked for."""
  # arithmetic per cell of one iteration (`work`): a program that computes
  # for hundreds of instructions per cell has nothing to hide behind a deep
  # prefetch queue and pays for its registers in resident waves (contrast,
  # 393 operations per cell: 703 us at 8 rows in flight, 660 at 2)
  first = default_prefetch(1) if stencil.dim == 2 and work < 128 else \
      (2 if stencil.dim == 2 else 1)
  pfs = [opts.prefetch] if opts.prefetch else [first, 2, 1]
  pfs = sorted(set(pfs), reverse=True)
  # (3-D: fewer rows per tile never paid -- denoise3d 512^3: 651 / 691 / 910
  # us at 4 / 2 / 1 rows, 1 cell per lane -- so the tile height stays)
  rows = opts.tile_rows
  vecs = []
  v = opts.vec or default_vec(stencil)
  while v >= 1:
    vecs.append(v)
    v //= 2
  leanest = None
  last_error = None
  for v, pf in itertools.product(vecs, pfs):
    trial = Module(stencil, opts.banks, opts.batch)
    try:
      est = add_march_pass(
          trial, march_config(opts, stencil, 1, v, pf, rows)).traffic_model[
              'est_window_regs']
    except util.SemanticError as e:
      last_error = e
      continue
    if est <= budget:
      return (v, pf, rows), last_error
    if leanest is None or est < leanest[0]:
      leanest = (est, v, pf, rows)
  return (leanest[1:] if leanest else None), last_error


def _append_march(mod: Module, cfg: MarchConfig, residual: bool) -> None:
  add_march_pass(mod, cfg)
  if residual:
    # (a form or depth whose twin does not fit has none: the library then
    # ends such a run in `<app>_residual`)
    add_march_twin(mod, cfg)


def _add_march(mod: Module, cfg: MarchConfig, residual: bool) -> bool:
  """The marching pass of `cfg`, and its residual twin if asked for, or
  nothing at all: False, with `mod` as it was, if the generator refuses."""
  keep = (len(mod.kernels), len(mod.passes), len(mod.chunks))
  try:
    _append_march(mod, cfg, residual)
  except util.SemanticError:
    del mod.kernels[keep[0]:], mod.passes[keep[1]:], mod.chunks[keep[2]:]
    return False
  return True


def _add_march_passes(mod: Module, stencil: core.Stencil, opts: LowerOptions,
                      work: int) -> bool:
  """The marching passes of every fusion depth that fits and of the one
  iteration; False, and nothing added, if no one-iteration shape exists."""
  shape, refusal = _one_iteration_shape(stencil, opts, work,
                                        opts.reg_budget or REG_BUDGET)
  if shape is None:
    if opts.strategy == 'march':
      raise refusal
    return False
  vec, pf1, rows1 = shape
  # waves that cover a whole row side by side, sharing x-halos through LDS
  share = 0
  if opts.row_cells and opts.xshare is not False and \
      (stencil.dim == 3 or opts.xshare) and opts.pipe in (None, 1):
    share = -(-opts.row_cells // (64 * vec))
    if share > (4 if opts.xshare is None else 16):
      share = 0
  # ... or a segment of it, on request (then instead of the whole row)
  seg = opts.xshare_block or 0
  if seg:
    share = 0
  for t in _fuse_depths(stencil, opts):
    # (xshare, xshare_block) to try in turn; overlapping strips last
    shared = [(0, seg)] if seg else ([(share, 0)] if share and t > 1 else [])
    for xs, xb in shared + [(0, 0)]:
      # a shape that does not fit: try without sharing; if the depth does not
      # fit at all the scheduler uses the others
      if _add_march(mod, march_config(opts, stencil, t, vec,
                                      opts.prefetch or None, xshare=xs,
                                      xshare_block=xb), opts.residual):
        break
  # (the one-iteration kernel shares x-halos only on request: measured)
  done1 = bool((share or seg) and opts.xshare) and _add_march(
      mod, march_config(opts, stencil, 1, vec, pf1, rows1, xshare=share,
                        xshare_block=seg), opts.residual)
  if not done1:
    _append_march(mod, march_config(opts, stencil, 1, vec, pf1, rows1),
                  opts.residual)
  return True


def _add_tile3d_passes(mod: Module, stencil: core.Stencil,
                       opts: LowerOptions) -> None:
  """One tile3d pass per requested depth, clipped to the iteration count only:
  the planes live in LDS, MAX_FUSE_3D (registers) does not bind.  A depth whose
  rings do not fit is dropped; an explicit request that ends with no fused
  pass at all hears why."""
  depths = sorted({min(t, stencil.iterate) for t in opts.fuse} - {0, 1},
                  reverse=True)
  refusal = None
  built = 0
  for t in depths:
    try:
      add_tile3d_pass(mod, t, tile_w=opts.tile3d_w, tile_h=opts.tile3d_h,
                      waves=opts.tile3d_waves, chunk=opts.chunk_rows,
                      nt_load=bool(opts.nt_load),
                      nt_store=bool(opts.nt_store),
                      xcd_swizzle=opts.xcd_swizzle)
      built += 1
    except util.SemanticError as e:
      refusal = refusal or e
  if not built:
    raise refusal or util.SemanticError(
        'tile3d: no fusion depth of 2 or more to build (iterate %d, fuse %s)'
        % (stencil.iterate, list(opts.fuse)))


def lower(stencil: core.Stencil, opts: Optional[LowerOptions] = None) -> Module:
  """Builds the module: passes for every requested fusion depth plus a
  1-iteration pass (always present: the scheduler needs it for remainders)."""
  opts = (opts or LowerOptions()).resolved(
      stencil.dim, iterated=stencil.iterate > 1)
  check_options(stencil, opts)
  mod = _lower_ldswin(stencil, opts)
  if mod is not None:
    return mod
  work = ops_per_cell(stencil)       # of the program as written
  stencil = _derive(stencil, opts)
  mod = Module(stencil, opts.banks, opts.batch, opts.residual)
  use_march = opts.strategy in ('auto', 'march', 'tile3d') and \
      march_supported(stencil) is None
  if opts.strategy == 'march' and not use_march:
    raise util.SemanticError('march: %s' % march_supported(stencil))
  if not (use_march and _add_march_passes(mod, stencil, opts, work)):
    if opts.banks:
      raise util.SemanticError(
          'banks: `direct` kernels read and write dense arrays')
    add_direct_pass(mod, opts.vec or 1)
  if opts.strategy == 'tile3d':
    _add_tile3d_passes(mod, stencil, opts)
  if opts.residual:
    residual.add_residual_kernel(mod)
  return mod
