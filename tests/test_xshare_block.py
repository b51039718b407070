"""Segmented x-halo sharing (`LowerOptions.xshare_block`, MarchConfig.
xshare_block): fused marching kernels whose block of B waves covers a SEGMENT
of the row, x-halos handed over through LDS between the block's waves, halo
lanes only at the segment's two outer sides.

CPU: the structure of what is built (name, block, tile, descriptor), its
resources, the launch geometry on any row length, the refusals and fallbacks,
the command line.  GPU: bit for bit against the C oracle on the valid box, on
row lengths taken from the built kernel's own segment width S = tile[0], so
that the seams between waves, between blocks and at a ragged row end are where
the test puts them whatever the generator makes S."""
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import fuzz

SUFFIX = '_xb%d'


def _stencil(name, iterate, **kw):
  from soda_amd import core
  if name.endswith('.soda'):
    return core.from_file(soda_path(name), iterate=iterate, **kw)
  return core.from_text(name, iterate=iterate, **kw)


def _opts(fuse, block, **kw):
  from soda_amd.codegen.hip import lower
  return lower.LowerOptions(fuse=tuple(fuse), xshare_block=block, **kw)


def _fused(mod):
  return [k for k in mod.kernels if k.tune and k.tune.get('fused', 1) > 1]


def _segment_kernels(mod, block):
  """The fused kernels of a module, all of which must be segmented ones of
  `block` waves."""
  fused = _fused(mod)
  assert fused, [k.name for k in mod.kernels]
  for k in fused:
    assert k.name.endswith(SUFFIX % block), k.name
    assert '_xs' not in k.name
    assert k.block == (64 * block, 1, 1)
    assert k.tune['max_extent0'] == 0
  return fused


def _halo_lanes(k, block):
  """(lanes_lo + lanes_hi) of a segmented kernel, from its tile."""
  v = k.tune['vec']
  assert k.tile[0] % v == 0
  return 64 * block - k.tile[0] // v


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def _heat3d_plan(built):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 4)
  opts = runtime.resolve_options(stencil, _opts((2,), 2), None)
  assert opts.row_cells is None            # no extent, no row length
  mod = lower.lower(stencil, opts)
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, 'heat3d.hip'))
  return stencil, mod, res


def test_heat3d_builds_without_a_row_length(built):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil, mod, res = _heat3d_plan(built)
  k, = _segment_kernels(mod, 2)
  assert k.block == (128, 1, 1)
  assert k.tune['max_extent0'] == 0
  # heat3d taps one cell to either side: two fused iterations lose two cells,
  # one lane of 4 cells, at each outer side
  lanes_lo = lanes_hi = 1
  v = k.tune['vec']
  assert v == 4
  assert k.tile[0] == (128 - lanes_lo - lanes_hi) * v
  assert k.tune['lane_redundancy'] == pytest.approx(128.0 / 126.0)
  assert k.tune['waves_per_block'] == 2
  r = res[k.name]
  assert r['scratch'] == 0, r
  # the whole-row form of the same program (rows of 512 cells: `_xs2`)
  whole = runtime.resolve_options(stencil, lower.LowerOptions(fuse=(2,)),
                                  (512, 512, 512))
  wmod = lower.lower(stencil, whole)
  wk, = _fused(wmod)
  assert wk.name.endswith('_xs2'), wk.name
  wres = runtime.kernel_resources(
      runtime.compile_source(wmod.source, 'heat3d.hip'))[wk.name]
  assert wres['scratch'] == 0
  assert runtime.waves_per_simd(r['vgpr']) >= \
      runtime.waves_per_simd(wres['vgpr']), (r, wres)


def test_one_plan_takes_rows_of_any_length(built):
  from soda_amd import runtime
  stencil, mod, res = _heat3d_plan(built)
  k, = _segment_kernels(mod, 2)
  plan = runtime.make_plan(mod, res)
  at = mod.kernels.index(k)
  for n0 in (64, 300, 512, 5000):
    tiles, ns = runtime.plan_geometry(plan, (n0, 9, 12))
    assert tiles[at][0] == k.tile[0]
    assert all(v > 0 for v in ns), (n0, ns)      # every pass stays modelled


def test_options_refusals_and_fallback(built):
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', 30)
  mod = lower.lower(stencil, runtime.resolve_options(
      stencil, _opts((13,), 8), None))
  k, = _segment_kernels(mod, 8)
  assert k.block == (512, 1, 1)
  # 13 cells at each side: 4 lanes of 4 cells
  assert _halo_lanes(k, 8) == 8 and k.tile[0] == (512 - 8) * 4
  r = runtime.kernel_resources(
      runtime.compile_source(mod.source, 'jacobi2d.hip'))[k.name]
  assert r['scratch'] == 0 and 0 < r['vgpr'] <= 512, \
      'jacobi2d T=13 xshare_block=8: %d VGPRs, %d bytes of scratch' % (
          r['vgpr'], r['scratch'])
  for bad in (1, 17):
    with pytest.raises(util.SemanticError, match='xshare_block'):
      lower.lower(stencil, _opts((13,), bad))
  # taps that reach two cells in x: overlapping strips, as without the option
  blur = _stencil('blur.soda', 4)
  got = lower.lower(blur, _opts((2,), 2, peel=0))
  fused = _fused(got)
  assert fused
  assert not any('_xb' in k.name or k.tune['max_extent0'] for k in got.kernels)
  plain = lower.lower(blur, lower.LowerOptions(fuse=(2,), peel=0))
  assert got.source == plain.source


def test_default_options_never_pick_it(monkeypatch):
  from soda_amd.codegen.hip import lower
  monkeypatch.delenv('SODA_HIP_XSHARE_BLOCK', raising=False)
  for name, iterate in (('jacobi2d.soda', 30), ('heat3d.soda', 4),
                        ('blur.soda', 4)):
    stencil = _stencil(name, iterate)
    for kw in (dict(peel=0), dict(peel=0, row_cells=512)):
      mod = lower.lower(stencil, lower.LowerOptions(**kw))
      assert not any('_xb' in k.name for k in mod.kernels)
      assert '_xb' not in mod.source
      # ... and saying "not used" changes nothing
      none = lower.lower(stencil, lower.LowerOptions(xshare_block=None, **kw))
      assert none.source == mod.source


def test_the_environment_override(monkeypatch):
  """SODA_HIP_XSHARE_BLOCK=B stands in where the option is not given, builds
  what the option builds, and yields to an explicit option."""
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 4)
  monkeypatch.delenv('SODA_HIP_XSHARE_BLOCK', raising=False)
  plain = lower.lower(stencil, lower.LowerOptions(fuse=(2,), peel=0))
  assert '_xb' not in plain.source
  asked = lower.lower(stencil, _opts((2,), 2, peel=0))
  monkeypatch.setenv('SODA_HIP_XSHARE_BLOCK', '2')
  opts = lower.LowerOptions(fuse=(2,), peel=0)
  assert opts.xshare_block == 2
  mod = lower.lower(stencil, opts)
  _segment_kernels(mod, 2)
  assert mod.source == asked.source
  assert _opts((2,), 4, peel=0).xshare_block == 4
  _segment_kernels(lower.lower(stencil, _opts((2,), 4, peel=0)), 4)
  monkeypatch.delenv('SODA_HIP_XSHARE_BLOCK')
  again = lower.lower(stencil, lower.LowerOptions(fuse=(2,), peel=0))
  assert again.source == plain.source


def test_it_wins_over_the_whole_row_form():
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 4)
  mod = lower.lower(stencil, _opts((2,), 4, peel=0, xshare=True,
                                   row_cells=512))
  _segment_kernels(mod, 4)


def _one_iteration_kernel(mod):
  k, = [k for k in mod.kernels if k.tune and k.tune.get('fused') == 1]
  return k


def test_the_one_iteration_kernel_takes_the_form_on_request_only():
  """As with whole rows: a one-iteration kernel has edge loads and no halo
  lanes to lose, so it shares x-halos only where `xshare=True` asks for it --
  denoise3d, whose local `g` is tapped one cell to either side."""
  from soda_amd.codegen.hip import lower
  stencil = _stencil('denoise3d.soda', 1)
  k = _one_iteration_kernel(lower.lower(stencil, _opts((), 2, peel=0)))
  assert '_xb' not in k.name and k.block == (64, 1, 1)
  k = _one_iteration_kernel(
      lower.lower(stencil, _opts((), 2, peel=0, xshare=True)))
  assert k.name.endswith('_xb2') and k.block == (128, 1, 1)
  assert k.tune['max_extent0'] == 0 and k.tile[0] < 128 * k.tune['vec']
  jacobi = _stencil('jacobi2d.soda', 9)
  mod = lower.lower(jacobi, _opts((4,), 2, peel=0))
  assert '_xb' not in _one_iteration_kernel(mod).name


def test_sodac_prints_a_segmented_kernel(built):
  r = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', soda_path('heat3d.soda'),
       '--iterate', '4', '--hip-fuse', '2', '--hip-xshare-block', '4',
       '--hip-kernel', '-'],
      capture_output=True, text=True, cwd=ROOT)
  assert r.returncode == 0, r.stderr
  assert 'void __launch_bounds__(256) heat3d_march3d_T2_' in r.stdout
  head = r.stdout[r.stdout.index('__launch_bounds__(256)'):]
  assert head[:head.index('(soda_hip_kargs_t')].endswith('_xb4')
  assert 'heat3d_march3d_T1_' in r.stdout        # the remainder pass


FUZZ_SEEDS = (25, 144, 304, 594, 663, 1129, 1376, 434, 626, 1049)


def _fuzz_case(seed):
  from soda_amd import core, util
  text, dim, iterate = fuzz.program(seed)
  try:
    return text, core.from_text(text)
  except util.SodaError as e:
    pytest.skip('seed %d: the generator produced an invalid program (%s)' %
                (seed, e))


def _fuzz_extent(seed, stencil, s, v):
  """A segment and nine lanes per row -- two blocks, the second nearly empty
  -- on the rows (x planes) fuzz gives the seed."""
  return (s + 9 * v,) + tuple(fuzz.extent_for(seed, stencil.dim)[1:])


def test_the_fuzz_seeds_build_the_new_kernel(built):
  """The ten seeds of the GPU test below: programs of fuzz's plain generator
  that are iterated and fusable and tap at most one cell to either side along
  x -- 2-D and 3-D, 1- to 8-byte cells.  The first seven have halo lanes at
  the segment's outer sides.  On the grid the GPU test uses, none has an empty
  valid box and the model, which schedules that never-calibrated run, launches
  the segmented kernel: no seed can skip or pass there without running it."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  halo = 0
  for seed in FUZZ_SEEDS:
    text, stencil = _fuzz_case(seed)
    assert stencil.iterate >= 2, seed
    mod = lower.lower(stencil,
                      runtime.resolve_options(stencil, _opts((2,), 2), None))
    fused = _segment_kernels(mod, 2)
    for k in fused:
      halo += _halo_lanes(k, 2) > 0
    extent = _fuzz_extent(seed, stencil, fused[0].tile[0],
                          fused[0].tune['vec'])
    lo, hi = stencil.valid_box(extent)
    assert all(h > l for l, h in zip(lo, hi)), (seed, extent, lo, hi)
    plan = runtime.make_plan(mod, runtime.kernel_resources(
        runtime.compile_source(mod.source, '%s.hip' % stencil.app_name)))
    count = dict(zip((p.fused_iters for p in mod.sorted_passes()),
                     runtime.plan_schedule(plan, extent, stencil.iterate)))
    assert count.get(2), (seed, extent, count)
  assert halo >= 7


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _inputs(stencil, extent, seed=0):
  shape = tuple(extent[::-1])
  rng = np.random.default_rng(seed)
  out = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if t.is_float:
      out[name] = rng.random(shape, dtype=np.float64).astype(dt)
    else:
      out[name] = rng.integers(0, 201, size=shape).astype(dt)
  return out


def _same_bits(g, w):
  if g.dtype.kind == 'f':
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    nan = np.isnan(w)
    return (np.ascontiguousarray(g).view(bits) ==
            np.ascontiguousarray(w).view(bits)) | (nan & np.isnan(g))
  return g == w


def _check(stencil, prog, extent, seed=0, whole=False, inputs=None):
  """One run of `prog` on `extent` against the C oracle: bit for bit on the
  valid box (`whole`: on the whole grid -- border: preserve)."""
  from oracle import c_oracle
  ins = inputs if inputs is not None else _inputs(stencil, extent, seed)
  want = c_oracle.COracle(stencil, openmp=False).run(ins)
  got = prog.run(ins)
  names = [k.name for k in prog.module.kernels]
  for o in stencil.output_names:
    if whole:
      g, w = got[o], want[o]
    else:
      lo, hi = stencil.valid_box(extent, o)
      assert all(h > l for l, h in zip(lo, hi)), \
          'empty valid box: bad test %s' % (extent,)
      idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
      g, w = got[o][idx], want[o][idx]
    same = _same_bits(g, w)
    assert same.all(), '%s on %s: %d cells of %s differ, columns %s (%s)' % (
        stencil.app_name, tuple(extent), int((~same).sum()), o,
        sorted(set(np.nonzero(~same)[-1].tolist()))[:12], names)


def _program(stencil, opts, block):
  """A program built WITHOUT an extent, never calibrated, and its segmented
  kernels' (S, V)."""
  from soda_amd import runtime
  prog = runtime.Program(stencil, opts, calibrate=False)
  assert prog.opts.row_cells is None
  fused = _segment_kernels(prog.module, block)
  s, v = fused[0].tile[0], fused[0].tune['vec']
  assert all(k.tile[0] == s and k.tune['vec'] == v for k in fused)
  return prog, s, v


def _runs_fused(prog, extent, depths):
  """The model's schedule for the run uses the segmented kernels."""
  sched = prog.schedule(extent, prog.stencil.iterate)
  for t in depths:
    assert sched.get(t), (extent, sched)


@pytest.mark.gpu
def test_seams_along_the_row(built):
  """heat3d T = 2 on blocks of two waves, ONE program handle on six row
  lengths: a wave that only keeps the barriers, a full segment, a second block
  with one valid lane, a row that ends in the second block's first wave (its
  second wave wholly beyond the row), a row that ends inside the outer halo
  lanes, three blocks and a bit."""
  stencil = _stencil('heat3d.soda', 4)
  prog, s, v = _program(stencil, _opts((2,), 2), 2)
  with prog:
    for n0 in (64, s, s + v, s + 64 * v + v, 2 * s - v, 3 * s + 40):
      extent = (n0, 9, 12)
      _runs_fused(prog, extent, (2,))
      _check(stencil, prog, extent, seed=n0)


@pytest.mark.gpu
@pytest.mark.parametrize('fuse,block,iterate', [(4, 2, 9), (8, 4, 9),
                                                (13, 2, 14)])
def test_depth_and_width_in_2d(built, fuse, block, iterate):
  """jacobi2d, 4 / 8 / 13 fused iterations on 2 / 4 / 2 waves per block; the
  iteration count leaves a remainder for the one-iteration pass; chunks of 16
  rows on 50: three chunks and a ragged fourth; two blocks and a bit per row."""
  chunk = 16
  stencil = _stencil('jacobi2d.soda', iterate)
  prog, s, v = _program(stencil, _opts((fuse,), block, chunk_rows=chunk), block)
  with prog:
    k, = _fused(prog.module)
    assert _halo_lanes(k, block) == 2 * -(-fuse // v)
    extent = (2 * s + 36, 3 * chunk + 2)
    tiles, _ = prog.geometry(extent)
    assert tuple(tiles[k.name]) == (s, chunk)
    sched = prog.schedule(extent, iterate)
    assert sched.get(fuse) and sched.get(1), sched
    _check(stencil, prog, extent, seed=fuse)


DOUBLE_2D = """kernel: jacobi2d_f64
burst width: 64
unroll factor: 2
iterate: 4
input double: a(32, *)
output double: b(0, 0) = (a(0, 1) + a(1, 0) + a(0, 0) + a(-1, 0) + a(0, -1)) * 0.2
"""

# x-taps on one side only: halo lanes at the low side of a segment, none at
# the high side
ONE_SIDED_2D = """kernel: upwind2d
burst width: 64
unroll factor: 2
iterate: 6
input float: a(32, *)
output float: b(0, 0) = (a(-1, 0) + a(0, 0) + a(0, 1) + a(0, -1)) * 0.25f
"""

# a local tapped off-centre in x: its end cells cross the waves as well
TWO_STAGE_3D = """kernel: smooth3d
burst width: 64
unroll factor: 2
iterate: 4
input float: a(32, 32, *)
local float: m(0, 0, 0) = (a(-1, 0, 0) + a(0, 0, 0) + a(1, 0, 0) + a(0, -1, 0) + a(0, 1, 0) + a(0, 0, 1)) * 0.125f
output float: b(0, 0, 0) = m(0, 0, -1) * 0.25f + (m(-1, 0, 0) + m(1, 0, 0)) * 0.125f + m(0, 0, 0) * 0.25f + m(0, 0, 1) * 0.25f
"""

# (program, iterate, fused depth, waves, (halo lanes low, high), border,
# further options, rows (x planes) of the grid)
SHAPES = {
    'f64': (DOUBLE_2D, 4, 2, 2, (1, 1), None, {}, (40,)),
    'one_sided': (ONE_SIDED_2D, 6, 6, 2, (2, 0), None, {}, (40,)),
    # (tiles of 2 rows: at the default 4 the fused kernel needs 319 VGPRs and
    # the time model, which schedules these never-calibrated runs, prefers
    # four one-iteration launches on so small a grid)
    # (two stages: an iteration reaches two planes up, the grid is deeper)
    'two_stage_3d': (TWO_STAGE_3D, 4, 2, 2, (1, 1), None, dict(tile_rows=2),
                     (13, 17)),
    'jacobi3d': ('jacobi3d.soda', 4, 2, 2, (1, 1), None, {}, (9, 12)),
    'heat3d_preserve': ('heat3d.soda', 5, 2, 2, (1, 1), 'preserve', {},
                        (9, 12)),
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(SHAPES))
def test_other_shapes_of_program(built, case):
  name, iterate, fuse, block, halo, border, more, rest = SHAPES[case]
  kw = {'border': border} if border else {}
  stencil = _stencil(name, iterate, **kw)
  prog, s, v = _program(stencil, _opts((fuse,), block, **more), block)
  with prog:
    k, = _fused(prog.module)
    assert _halo_lanes(k, block) == sum(halo), (k.name, k.tile)
    if case == 'f64':
      assert v == 2
    # a row that ends in the second block's outer halo lanes, and one with a
    # third block of a few lanes
    for n0 in (2 * s - v, 2 * s + 9 * v):
      extent = (n0,) + rest
      _runs_fused(prog, extent, (fuse,))
      _check(stencil, prog, extent, seed=n0, whole=border is not None)


@pytest.mark.gpu
def test_one_iteration_kernel_on_request(built):
  """denoise3d (two inputs, one iteration, a local tapped off-centre in x)
  on segments of two waves: two blocks and nine lanes per row."""
  from soda_amd import runtime
  stencil = _stencil('denoise3d.soda', 1)
  with runtime.Program(stencil, _opts((), 2, xshare=True),
                       calibrate=False) as prog:
    k = _one_iteration_kernel(prog.module)
    assert k.name.endswith('_xb2') and k.tune['max_extent0'] == 0
    s, v = k.tile[0], k.tune['vec']
    for n0 in (s + v, 2 * s + 9 * v):
      _check(stencil, prog, (n0, 9, 12), seed=n0)


@pytest.mark.gpu
def test_runs_that_keep_a_row_range(built):
  """A cone run (`keep`) on the segmented kernels, two blocks per row: the kept
  rows equal the untrimmed run bit for bit, and the passes covered fewer
  rows."""
  import torch
  iterate, keep = 9, (40, 80)
  stencil = _stencil('jacobi2d.soda', iterate)
  prog, s, v = _program(stencil, _opts((4,), 2), 2)
  with prog:
    extent = (s + 40, 120)
    _runs_fused(prog, extent, (4,))
    ins = _inputs(stencil, extent, 7)
    src = [torch.from_numpy(ins[n]).cuda() for n in stencil.input_names]
    full = [torch.zeros_like(src[0]) for _ in stencil.output_names]
    part = [torch.full_like(src[0], 77) for _ in stencil.output_names]
    st = torch.cuda.current_stream().cuda_stream
    prog.run_device([t.data_ptr() for t in full], [t.data_ptr() for t in src],
                    extent, stream=st)
    rows_full = prog.last_rows()
    prog.run_device([t.data_ptr() for t in part], [t.data_ptr() for t in src],
                    extent, stream=st, keep=keep)
    rows_part = prog.last_rows()
    torch.cuda.synchronize()
  assert rows_part < rows_full
  lo, hi = stencil.valid_box(extent)
  box = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
  a = full[0].cpu().numpy()[box]
  b = part[0].cpu().numpy()[box]
  k0, k1 = max(keep[0], lo[-1]) - lo[-1], min(keep[1], hi[-1]) - lo[-1]
  assert k1 > k0
  assert _same_bits(b[k0:k1], a[k0:k1]).all()
  from oracle import c_oracle
  want = c_oracle.COracle(stencil, openmp=False).run(ins)
  assert _same_bits(a, want[stencil.output_names[0]][box]).all()


@pytest.mark.gpu
@pytest.mark.parametrize('seed', FUZZ_SEEDS)
def test_random_programs(built, seed):
  """Programs of fuzz's plain generator with xshare_block = 2 forced, on rows
  of a segment and nine lanes: two blocks, the second nearly empty.  (That no
  seed has an empty valid box there is checked without a GPU, above.)"""
  text, stencil = _fuzz_case(seed)
  prog, s, v = _program(stencil, _opts((2,), 2), 2)
  with prog:
    extent = _fuzz_extent(seed, stencil, s, v)
    _runs_fused(prog, extent, (2,))
    _check(stencil, prog, extent, inputs=fuzz.inputs_for(stencil, extent, seed))
