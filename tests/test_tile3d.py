"""`tile3d`: the LDS-tiled 3-D kernels that fuse more than two iterations
(soda_amd/codegen/hip/tile3d.py).  CPU tests: what lower() builds, what it
refuses, what the compiled kernels need.  GPU tests: bit for bit against the C
oracle on the valid box, nothing written outside it, through runtime.Program
(the C ABI).

GPU runs are built with calibrate=False: a tile3d pass carries no time model,
so the library's scheduler then goes deepest pass first (soda_hip.cpp
`schedule`) and the test KNOWS which kernels ran -- it asserts the schedule.
(test_first_run_times_the_passes is the exception: it is about the default.)

The seam tests at the end take their extents from the valid tile (VX, VY) of
the kernel that was built, never from literal sizes.
"""
import functools
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import fuzz

LDS_PER_CU = 160 * 1024


def _stencil(name, iterate, **kw):
  """A corpus program by file name, or one of SEAM_PROGRAMS by its name."""
  from soda_amd import core
  if name in SEAM_PROGRAMS:
    return core.from_text(SEAM_PROGRAMS[name], iterate=iterate, **kw)
  return core.from_file(soda_path(name), iterate=iterate, **kw)


def _tile3d_kernels(mod):
  return [k for k in mod.kernels if '_tile3d_' in k.name]


# ---------------------------------------------------------------------------
# CPU: structure, resources, refusals, the command line
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['heat3d.soda', 'jacobi3d.soda'])
def test_pass_structure_and_resources(built, name):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, 8)
  mod = lower.lower(stencil, lower.LowerOptions(strategy='tile3d', fuse=(4, 3)))
  assert sorted(p.fused_iters for p in mod.passes) == [1, 3, 4]
  kinds = {p.fused_iters: p.kind for p in mod.passes}
  assert kinds == {4: 'tile3d', 3: 'tile3d', 1: 'march3d'}
  code = runtime.compile_source(mod.source, '%s.hip' % stencil.app_name)
  res = runtime.kernel_resources(code)
  plan = runtime.make_plan(mod, res)        # the C ABI's view of it
  assert plan.num_passes == 3
  for p in mod.passes:
    if p.kind != 'tile3d':
      continue
    k = mod.kernels[p.kernels[0]]
    r = res[k.name]
    assert 'tile3d_T%d_' % p.fused_iters in k.name
    assert r['scratch'] == 0
    assert r['lds'] == p.traffic_model['lds_bytes'] <= LDS_PER_CU
    # the block's waves are resident together: the registers must admit its
    # share of every SIMD (4 SIMDs per CU)
    waves = k.block[0] // 64
    assert runtime.waves_per_simd(r['vgpr'] + r['agpr']) >= -(-waves // 4)
    # marching along dimension 2 with a chunk length the host must keep
    assert k.tune['axis'] == 2 and k.tune['fixed'] and \
        k.tune['fused'] == p.fused_iters
    assert k.tune['waves_per_block'] == waves
  # two blocks per CU for the flagship depth
  four = [p for p in mod.passes if p.fused_iters == 4][0]
  assert four.traffic_model['lds_bytes'] <= LDS_PER_CU // 2
  # the geometry the library derives: the chunk as declared, a schedule that
  # goes deepest first while no pass has been timed
  tiles, ns = runtime.plan_geometry(plan, (512, 512, 512))
  by_name = dict(zip((k.name for k in mod.kernels), tiles))
  for k in _tile3d_kernels(mod):
    assert by_name[k.name][:3] == k.tile[:3]
  assert runtime.plan_schedule(plan, (512, 512, 512), 8) == [2, 0, 0]
  assert runtime.plan_schedule(plan, (512, 512, 512), 9) == [2, 0, 1]
  assert runtime.plan_schedule(plan, (512, 512, 512), 7) == [1, 1, 0]


def test_depth_is_not_capped_by_the_register_kernels_limit(built):
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 12)
  mod = lower.lower(stencil, lower.LowerOptions(strategy='tile3d', fuse=(6, 4)))
  assert sorted(p.fused_iters for p in mod.passes) == [1, 4, 6]
  assert max(p.fused_iters for p in mod.passes) > lower.MAX_FUSE_3D
  # ... and is clipped to the iteration count
  mod = lower.lower(_stencil('heat3d.soda', 3),
                    lower.LowerOptions(strategy='tile3d', fuse=(6, 4)))
  assert sorted(p.fused_iters for p in mod.passes) == [1, 3]


def test_tile_options_shape_the_kernel(built):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 8)
  mod = lower.lower(stencil, lower.LowerOptions(
      strategy='tile3d', fuse=(4,), tile3d_w=128, tile3d_h=12, tile3d_waves=4))
  k, = _tile3d_kernels(mod)
  assert k.block == (256, 1, 1)
  assert k.tile[:2] == (128 - 8, 12 - 8)
  assert k.tune['tile3d'] == (128, 12)
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, 'heat3d.hip'))
  p = [p for p in mod.passes if p.kind == 'tile3d'][0]
  assert res[k.name]['lds'] == p.traffic_model['lds_bytes']
  assert res[k.name]['scratch'] == 0
  from soda_amd import util
  for bad in (dict(tile3d_w=96), dict(tile3d_h=16, tile3d_waves=3),
              dict(tile3d_h=8)):       # 8 rows: no valid row at depth 4
    with pytest.raises(util.SemanticError, match='tile3d'):
      lower.lower(stencil, lower.LowerOptions(strategy='tile3d', fuse=(4,),
                                              **bad))


def test_auto_and_march_are_unchanged():
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 8)
  assert 'tile3d' in lower.STRATEGIES
  assert lower.MAX_FUSE_3D == 2
  auto = lower.lower(stencil, lower.LowerOptions(fuse=(4,)))
  assert 'tile3d' not in auto.source
  assert max(p.fused_iters for p in auto.passes) == lower.MAX_FUSE_3D
  assert all(p.kind == 'march3d' for p in auto.passes)
  march = lower.lower(stencil, lower.LowerOptions(strategy='march', fuse=(2,)))
  assert 'tile3d' not in march.source
  assert all(p.kind == 'march3d' for p in march.passes)
  # the one-iteration pass of a tile3d module is the one `auto` builds
  t3 = lower.lower(stencil, lower.LowerOptions(strategy='tile3d', fuse=(4,)))
  one = lambda m: [m.chunks[p.kernels[0]] for p in m.passes
                   if p.fused_iters == 1]
  assert one(t3) == one(auto)


MANY_LOCALS = '''kernel: many
burst width: 64
unroll factor: 2
input dram 0 float: in(32, 32, *)
local float: a(0, 0, 0) = in(1, 0, 2) + in(-1, 0, -2)
local float: b(0, 0, 0) = a(0, 0, 2) + a(0, 0, -2)
local float: c(0, 0, 0) = b(0, 0, 2) + b(0, 0, -2)
local float: d(0, 0, 0) = c(0, 0, 2) + c(0, 0, -2)
local float: e(0, 0, 0) = d(0, 0, 2) + d(0, 0, -2)
local float: f(0, 0, 0) = e(0, 0, 2) + e(0, 0, -2)
output dram 1 float: out(0, 0, 0) = f(0, 0, 2) + f(0, 0, -2)
iterate: 6
border: ignore
cluster: none
'''


PARAM3D = """kernel: wsum3d
burst width: 64
unroll factor: 2
iterate: 5
input float: a(32, 32, *)
param float: c[2]
output float: b(0, 0, 0) = a(0, 0, -1) * c(0) + a(1, 0, 0) * c(1)
"""


# Programs for the seams of the kernel: where a chunk, a tile or a slab ends.
#   fwd3d   reaches forward only along z (m_lo = 0: nothing below a chunk)
#   back3d  reaches backward only (m_hi = 0: nothing above it)
#   u32     wraps on multiplication, shifts in zeros on division
#   i32     divides and takes remainders of negative operands (C truncates)
#   pair3d  two circulating tensors whose outputs have different delays
_SEAM_HEADER = '''kernel: %s
burst width: 64
unroll factor: 2
iterate: 6
'''
SEAM_PROGRAMS = {name: _SEAM_HEADER % name + body for name, body in {
    'fwd3d': '''input float: a(32, 32, *)
output float: b(0,0,0) = (a(0,0,0) + a(0,0,2) + a(2,0,1) + a(0,1,0)) * 0.25f
''',
    'back3d': '''input float: a(32, 32, *)
output float: b(0,0,0) = (a(0,0,-2) + a(0,0,-1) + a(-1,-2,0)) * 0.5f
''',
    'u32': '''input uint32: a(32, 32, *)
output uint32: b(0,0,0) = (a(0,0,1) * 2654435761 + a(-1,0,0)) ^ (a(0,1,-1) / 8)
''',
    'i32': '''input int32: a(32, 32, *)
output int32: b(0,0,0) = (a(0,0,1) - a(1,0,0) * 3) / 2 + a(0,-1,-1) % 7
''',
    'pair3d': '''input float: u(32, 32, *)
input float: v
local float: w(0,0,0) = u(0,0,1) - v(1,0,0)
output float: p(0,0,0) = w(0,0,-1) * 0.5f + v(0,0,2) * 0.25f
output float: q(0,0,0) = u(-1,0,0) + w(0,1,0) * 0.125f
''',
}.items()}


@functools.lru_cache(maxsize=None)
def _lowered(name, fuse, **kw):
  """The module lower() builds for a tile3d request (CPU only; the kernels a
  Program then JIT-builds from the same options are these)."""
  from soda_amd.codegen.hip import lower
  return lower.lower(_stencil(name, 13), lower.LowerOptions(
      strategy='tile3d', fuse=fuse, **kw))


def _valid_tile(name, fuse, **kw):
  """(VX, VY) of the deepest tile3d kernel: the cells of a tile it stores."""
  mod = _lowered(name, tuple(fuse), **kw)
  deepest = max((p for p in mod.passes if p.kind == 'tile3d'),
                key=lambda p: p.fused_iters)
  return mod.kernels[deepest.kernels[0]].tile[:2]


def _grid(name, fuse, mul_x, dx, mul_y, dy, planes, **kw):
  """An extent placed against the tile seams: mul valid tiles + d cells."""
  vx, vy = _valid_tile(name, fuse, **kw)
  return (mul_x * vx + dx, mul_y * vy + dy, planes)


@pytest.mark.parametrize('name', sorted(SEAM_PROGRAMS))
def test_seam_programs_structure_and_oracles(built, name):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  from oracle import c_oracle, numpy_oracle
  stencil = _stencil(name, 6)
  mod = lower.lower(stencil, lower.LowerOptions(strategy='tile3d', fuse=(4, 3)))
  assert {p.fused_iters: p.kind for p in mod.passes} == \
      {4: 'tile3d', 3: 'tile3d', 1: 'march3d'}
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, '%s.hip' % stencil.app_name))
  for p in mod.passes:
    if p.kind != 'tile3d':
      continue
    k = mod.kernels[p.kernels[0]]
    assert res[k.name]['scratch'] == 0
    assert res[k.name]['lds'] == p.traffic_model['lds_bytes'] <= LDS_PER_CU
    assert p.traffic_model['valid'] == k.tile[:2]
  # the two oracles, written independently of each other, agree on the program
  # (wrapping uint32 products, truncating int32 division, float bits)
  vx, vy = _valid_tile(name, (4, 3))
  extent = (2 * vx + 1, 2 * vy + 1, 33)
  inputs = _inputs(stencil, extent, 1)
  a = numpy_oracle.run(stencil, inputs, iterate=6)
  b = c_oracle.COracle(stencil).run(inputs, iterate=6)
  for out in stencil.output_names:
    lo, hi = stencil.valid_box(extent, out, 6)
    assert all(h > l for l, h in zip(lo, hi))
    idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
    assert np.isfinite(b[out][idx]).all() and b[out][idx].any()
    assert np.array_equal(a[out][idx].view(np.uint32),
                          b[out][idx].view(np.uint32)), out


# Tile seams: the grid's edge on a tile's edge and one cell to either side of
# it, in x and in y -- (tiles along x, dx, tiles along y, dy).  The last case
# of each list makes a launch of 8 blocks: the XCD renumbering of the blocks
# has a branch for a multiple of 8 and one for the rest.
SEAM_EXTENTS = [(2, dx, 2, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)] + \
    [(4, 0, 2, 0)]
WIDE = dict(tile3d_w=128, tile3d_h=12, tile3d_waves=4)
# two columns per lane: the grid ends inside the second column of a lane
WIDE_EXTENTS = [(1, dx, 3, 0) for dx in (-1, 0, 1)] + [(1, 1, 4, 0)]


@pytest.mark.parametrize('name,cases,kw', [
    ('fwd3d', SEAM_EXTENTS, {}), ('back3d', SEAM_EXTENTS, {}),
    ('pair3d', SEAM_EXTENTS, {}), ('heat3d.soda', WIDE_EXTENTS, WIDE)])
def test_seam_cases_take_both_branches_of_the_block_renumbering(built, name,
                                                                cases, kw):
  """`nblk % 8 == 0` and not: the GPU cases of test_tile_seams run both."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, 4)
  seen = set()
  for case in cases:
    extent = _grid(name, (4,), *case, 33, **kw)
    # (as runtime.Program lowers it: the one-iteration kernel of the module
    # is shaped for the extent)
    mod = lower.lower(stencil, runtime.resolve_options(
        stencil, lower.LowerOptions(strategy='tile3d', fuse=(4,), **kw),
        extent))
    at, = [i for i, k in enumerate(mod.kernels) if '_tile3d_T4_' in k.name]
    tile = runtime.plan_geometry(runtime.make_plan(mod), extent)[0][at]
    assert tile[:2] == _valid_tile(name, (4,), **kw)
    blocks = 1
    for n, t in zip(extent, tile):
      blocks *= -(-n // t)
    seen.add(blocks % 8 == 0)
  assert seen == {True, False}


def test_a_fixed_chunk_is_held_against_the_buffer_window(built):
  """A chunk's buffer windows must stay within 1 GiB.  The kernels clip them
  to the grid, so what counts is min(chunk, planes of the grid)."""
  from soda_amd import runtime, util
  mod = _lowered('heat3d.soda', (4,))
  plan = runtime.make_plan(mod)
  k, = _tile3d_kernels(mod)
  at = mod.kernels.index(k)
  assert k.tile[2] == 128 and k.tune['fixed']
  # 64 MiB a plane: 16 planes a GiB, 8 of them the reach of four iterations
  with pytest.raises(util.BackendError,
                     match=r'chunks of 128 planes exceed the 1 GiB buffer '
                     r'window on this extent \(at most 8\)'):
    runtime.plan_geometry(plan, (4096, 4096, 256))
  # 8 MiB a plane: at most 120 planes -- and the grid has 64
  tiles, _ = runtime.plan_geometry(plan, (2048, 1024, 64))
  assert tiles[at][:3] == k.tile[:3]
  tiles, _ = runtime.plan_geometry(plan, (2048, 1024, 120))
  assert tiles[at][:3] == k.tile[:3]
  # a grid longer than the limit is refused, however long the chunk
  for planes in (121, 128, 512):
    with pytest.raises(util.BackendError, match='1 GiB buffer window.*120'):
      runtime.plan_geometry(plan, (2048, 1024, planes))
  # a shorter fixed chunk fits it
  short = _lowered('heat3d.soda', (4,), chunk_rows=8)
  runtime.plan_geometry(runtime.make_plan(short), (2048, 1024, 512))


def test_an_empty_box_is_handed_over_inside_the_array():
  """Seven iterations of back3d lose 14 rows at the low end: on 11 rows the
  valid box is empty and starts beyond the array.  runtime.Program.run and
  Group.store used to hand that to the library, which refuses a box outside
  the array -- the run must go through and write nothing."""
  from soda_amd import runtime
  stencil = _stencil('back3d', 7)
  extent = (65, 11, 23)
  lo, hi = stencil.valid_box(extent, 'b', 7)
  assert lo[1] > extent[1] and hi[1] == extent[1]
  clo, chi = runtime.clipped_box((lo, hi), extent)
  assert all(0 <= l <= h <= e for l, h, e in zip(clo, chi, extent))
  assert clo[1] == chi[1] and (clo[0], chi[0], clo[2], chi[2]) == \
      (lo[0], hi[0], lo[2], hi[2])
  # a box that is not empty is left as it is
  box = stencil.valid_box((65, 19, 23), 'b', 7)
  assert runtime.clipped_box(box, (65, 19, 23)) == (list(box[0]), list(box[1]))
  # hi below lo (a symmetric reach): empty at lo
  heat = _stencil('heat3d.soda', 8)
  lo, hi = heat.valid_box((61, 11, 160), 'out', 8)
  assert hi[1] < lo[1] <= 11
  clo, chi = runtime.clipped_box((lo, hi), (61, 11, 160))
  assert clo[1] == chi[1] == lo[1]


def test_refusals_name_their_reason():
  from soda_amd import core, util
  from soda_amd.codegen.hip import lower, tile3d
  opts = lambda **kw: lower.LowerOptions(strategy='tile3d', fuse=(4,), **kw)
  cases = [
      (_stencil('jacobi2d.soda', 8), '3-dimensional'),
      (_stencil('denoise3d.soda', None), 'iterable'),
      (_stencil('heat3d.soda', 8, border='preserve'), 'preserve'),
      (core.from_text(open(soda_path('heat3d.soda')).read().replace(
          'float', 'double').replace('.125f', '.125').replace('.25f', '.25'),
                      iterate=8), 'double'),
  ]
  cases.append((core.from_text(PARAM3D), 'param'))
  for stencil, word in cases:
    assert word in tile3d.tile3d_supported(stencil)
    with pytest.raises(util.SemanticError, match='tile3d.*%s' % word):
      lower.lower(stencil, opts())
  assert tile3d.tile3d_supported(_stencil('heat3d.soda', 8)) is None
  # rings that cannot fit: seven tensors a level, every one read across five
  # planes (42 rings of 6 planes: 266 KB at the smallest tile) -- and the next
  # requested depth is tried before the request fails
  many = core.from_text(MANY_LOCALS)
  with pytest.raises(util.SemanticError, match='tile3d.*LDS'):
    lower.lower(many, lower.LowerOptions(strategy='tile3d', fuse=(6,),
                                         inline=False))
  mod = lower.lower(many, lower.LowerOptions(strategy='tile3d', fuse=(6, 2),
                                             inline=False))
  assert sorted(p.fused_iters for p in mod.passes) == [1, 2]
  # nothing to fuse: an explicit request hears it
  with pytest.raises(util.SemanticError, match='tile3d'):
    lower.lower(_stencil('heat3d.soda', 1), opts())
  with pytest.raises(util.SemanticError, match='strategy'):
    lower.lower(_stencil('heat3d.soda', 8),
                lower.LowerOptions(strategy='tile4d'))


def test_sodac_prints_a_tile3d_kernel(built):
  r = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', soda_path('heat3d.soda'),
       '--iterate', '8', '--hip-strategy', 'tile3d', '--hip-fuse', '4',
       '--hip-kernel', '-', '--hip-no-probe'],
      capture_output=True, text=True, cwd=ROOT)
  assert r.returncode == 0, r.stderr
  assert 'void __launch_bounds__(512) heat3d_tile3d_T4_' in r.stdout
  assert 'heat3d_march3d_T1_' in r.stdout        # the remainder pass
  assert r.stdout.count('soda_pipe_barrier();') >= 1
  # the fused step is straight-line: one barrier, no early exit
  body = r.stdout[r.stdout.index('heat3d_tile3d_T4_'):]
  body = body[:body.index('\n}\n')]
  assert body.count('soda_pipe_barrier();') == 1 and 'return' not in body
  r = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', soda_path('jacobi2d.soda'),
       '--hip-strategy', 'tile3d', '--hip-kernel', '-', '--hip-no-probe'],
      capture_output=True, text=True, cwd=ROOT)
  assert r.returncode == 1 and 'tile3d' in r.stderr


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _inputs(stencil, extent, seed=0, kind='random'):
  shape = tuple(extent[::-1])
  rng = np.random.default_rng(seed)
  out = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if kind == 'ramp':
      out[name] = np.indices(shape).sum(axis=0).astype(dt)
    elif t.is_float:
      out[name] = rng.random(shape, dtype=np.float64).astype(dt)
    elif dt.kind == 'i':
      # signed cells stay small: i32 of SEAM_PROGRAMS grows at most 2.5 times
      # an iteration, 13 iterations from 1000 stay below 2^31, so these cases
      # never wrap.  (Overflow is defined, -fwrapv on both sides: cells of the
      # whole int32 range run in tests/test_values.py.)
      out[name] = rng.integers(-1000, 1001, size=shape,
                               dtype=np.int64).astype(dt)
    else:
      info = np.iinfo(dt)
      out[name] = rng.integers(info.min, int(info.max) + 1, size=shape,
                               dtype=np.int64).astype(dt)
  return out


@functools.lru_cache(maxsize=None)
def _reference(name, extent, iterate, seed):
  """(inputs, oracle outputs) of a corpus program: computed once, shared."""
  from oracle import c_oracle
  stencil = _stencil(name, iterate)
  inputs = _inputs(stencil, extent, seed)
  want = c_oracle.COracle(stencil).run(inputs, iterate=iterate)
  for a in list(inputs.values()) + list(want.values()):
    a.setflags(write=False)
  return inputs, want


def _compare(stencil, extent, iterate, got, want, what='', empty=False):
  """The checks of tests/test_hip_parity.py `_check`.  `empty`: the case is
  KNOWN to leave no valid cell (so many iterations on so small a grid); the
  kernels still run, and all that can be asked is that nothing is written."""
  from oracle import numpy_oracle
  for name in stencil.output_names:
    lo, hi = stencil.valid_box(extent, name, iterate)
    if empty:
      assert any(h <= l for l, h in zip(lo, hi)), 'the box is not empty'
      assert not got[name].any()
      continue
    assert all(h > l for l, h in zip(lo, hi)), 'empty valid box: bad test'
    idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
    g, w = got[name][idx], want[name][idx]
    # (the reference's tolerance check counts a NaN or infinite reference cell
    # as a mismatch even against itself -- four iterations of the random
    # programs overflow in places -- so it may count what it counts there)
    assert numpy_oracle.compare(got[name], want[name], lo, hi) == \
        numpy_oracle.compare(want[name], want[name], lo, hi)
    if g.dtype.kind == 'f':
      # bit for bit; a NaN is a NaN (its sign and payload are the machine's,
      # as in tests/test_fuzz.py: equal_nan)
      nan = np.isnan(w)
      assert np.array_equal(np.isnan(g), nan)
      same = (g.view(np.uint32) == w.view(np.uint32)) | nan
    else:
      same = g == w
    assert same.all(), '%s: %d cells not bit-identical (%s)' % (
        name, (~same).sum(), what)
    # outside the box the caller's array is untouched (zeros here)
    mask = np.ones(got[name].shape, bool)
    mask[idx] = False
    assert not got[name][mask].any()


def _run(stencil, extent, opts, iterate, inputs, want, expect, empty=False,
         tile=None):
  """Runs on the GPU with the deepest-first schedule, asserts that schedule is
  `expect` ({depth: launches}) and compares with the oracle.  `tile`: the valid
  tile the extent was derived from -- the deepest kernel built must have it."""
  from soda_amd import runtime
  with runtime.Program(stencil, opts, extent=extent, calibrate=False) as prog:
    sched = {t: n for t, n in prog.schedule(extent, iterate).items() if n}
    assert sched == expect
    kinds = {p.fused_iters: p.kind for p in prog.module.passes}
    assert all(kinds[t] == 'tile3d' for t in sched if t > 1)
    if tile is not None:
      k, = [k for k in prog.module.kernels
            if '_tile3d_T%d_' % max(expect) in k.name]
      assert k.tile[:2] == tuple(tile)
    got = prog.run(inputs, iterate=iterate)
    names = [k.name for k in prog.module.kernels]
  _compare(stencil, extent, iterate, got, want, names, empty)


def _mix(iterate, depths):
  """Deepest first."""
  out = {}
  for t in sorted(set(depths) | {1}, reverse=True):
    if iterate >= t:
      out[t], iterate = iterate // t, iterate % t
  return {t: n for t, n in out.items() if n}


# T=4 of these programs warms up for 12 plane steps (8 of skew + a reach of 4):
# (130, 20, 11) is shorter than that.  Both programs reach one cell per
# iteration in every direction, so i iterations leave cells [i, n - i) of an
# extent n: (64, 9, 40) has one valid row at 4 iterations and none from 5 on,
# (130, 20, 11) no valid plane from 6 on.  Those cases still run -- every
# launch of them -- and must write nothing.
CORPUS_CASES = [(e, i) for e in [(300, 24, 40), (64, 9, 40), (516, 37, 70),
                                 (130, 20, 11)] for i in (4, 5, 8, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize('extent,iterate', CORPUS_CASES)
@pytest.mark.parametrize('name', ['heat3d.soda', 'jacobi3d.soda'])
def test_corpus_programs(built, name, extent, iterate):
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 3)
  _run(stencil, extent, lower.LowerOptions(strategy='tile3d', fuse=(4,)),
       iterate, inputs, want, _mix(iterate, (4,)),
       empty=2 * iterate >= min(extent))


@pytest.mark.gpu
@pytest.mark.parametrize('fuse,iterate', [((3,), 7), ((6,), 13)])
def test_other_depths(built, fuse, iterate):
  from soda_amd.codegen.hip import lower
  extent = (260, 70, 33)
  stencil = _stencil('heat3d.soda', iterate)
  inputs, want = _reference('heat3d.soda', extent, iterate, 5)
  _run(stencil, extent, lower.LowerOptions(strategy='tile3d', fuse=fuse),
       iterate, inputs, want, _mix(iterate, fuse))


@pytest.mark.gpu
@pytest.mark.parametrize('kw', [
    dict(tile3d_w=128, tile3d_h=12, tile3d_waves=4),
    dict(tile3d_h=32, tile3d_waves=16),
    dict(tile3d_h=16, tile3d_waves=2, chunk_rows=16),
])
def test_other_tile_shapes(built, kw):
  from soda_amd.codegen.hip import lower
  extent, iterate = (300, 24, 40), 4
  stencil = _stencil('heat3d.soda', iterate)
  inputs, want = _reference('heat3d.soda', extent, iterate, 3)
  _run(stencil, extent,
       lower.LowerOptions(strategy='tile3d', fuse=(4,), **kw), iterate,
       inputs, want, {4: 1})


@pytest.mark.gpu
def test_heat3d_ramp_is_a_fixed_point(built):
  """heat3d leaves p + q + r unchanged, bit for bit (the closed form of
  tests/test_hip_parity.py test_heat3d_ramp_is_fixed_point)."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil('heat3d.soda', 12)
  extent = (96, 40, 48)
  inputs = _inputs(stencil, extent, kind='ramp')
  with runtime.Program(stencil,
                       lower.LowerOptions(strategy='tile3d', fuse=(4,)),
                       extent=extent, calibrate=False) as prog:
    assert prog.schedule(extent, 12) == {4: 3}
    got = prog.run(inputs)['out']
  lo, hi = stencil.valid_box(extent)
  assert all(h > l for l, h in zip(lo, hi))
  idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
  assert (got[idx] == inputs['in'][idx]).all()


@pytest.mark.gpu
def test_full_size(built):
  """The BASELINE C4 grid: 512^3, two launches of the T=4 kernel."""
  from soda_amd.codegen.hip import lower
  extent, iterate = (512, 512, 512), 8
  stencil = _stencil('heat3d.soda', iterate)
  inputs, want = _reference('heat3d.soda', extent, iterate, 11)
  _run(stencil, extent, lower.LowerOptions(strategy='tile3d', fuse=(4,)),
       iterate, inputs, want, {4: 2})
  _reference.cache_clear()       # a gigabyte of arrays


FUZZ_SEEDS = (20, 136, 225, 244, 414, 434, 449, 513, 536, 571, 587, 663)
FUZZ_TENSORS = (2, 2, 4, 3, 2, 2, 4, 2, 3, 7, 5, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,tensors', list(zip(FUZZ_SEEDS, FUZZ_TENSORS)))
def test_random_programs(built, seed, tensors):
  from soda_amd import core, util
  from soda_amd.codegen.hip import lower
  from oracle import c_oracle
  extent, iterate = (96, 72, 40), 4
  stencil = core.from_text(fuzz.program(seed)[0], iterate=iterate)
  assert stencil.dim == 3 and len(stencil.symbol_table) == tensors
  opts = lower.LowerOptions(strategy='tile3d', fuse=(4, 3))
  try:
    mod = lower.lower(stencil, opts)
  except util.SemanticError as e:
    # only programs of more than three tensors, only for want of LDS
    assert tensors > 3 and 'LDS' in str(e)
    return
  deepest = max(p.fused_iters for p in mod.passes)
  assert deepest >= 3
  inputs = fuzz.inputs_for(stencil, extent, seed)
  want = c_oracle.COracle(stencil).run(inputs, iterate=iterate)
  _run(stencil, extent, opts, iterate, inputs, want,
       {4: 1} if deepest == 4 else {3: 1, 1: 1})


@pytest.mark.gpu
def test_two_virtual_slabs_equal_one_gpu(built, monkeypatch):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  # (no pass is timed: every slab's schedule goes deepest first)
  monkeypatch.setenv('SODA_HIP_NO_CALIBRATE', '1')
  extent, iterate = (300, 24, 80), 8
  stencil = _stencil('heat3d.soda', iterate)
  inputs, want = _reference('heat3d.soda', extent, iterate, 7)
  opts = lower.LowerOptions(strategy='tile3d', fuse=(4,))
  with runtime.Program(stencil, opts, extent=extent, calibrate=False) as prog:
    assert prog.schedule(extent, iterate) == {4: 2}
    single = prog.run(inputs)
  _compare(stencil, extent, iterate, single, want, 'one device')
  for overlap in (True, False):
    with runtime.Group(stencil, extent, [0, 0], opts,
                       overlap=overlap) as group:
      assert any('_tile3d_T4_' in k.name for k in group.module.kernels)
      got = group.run_host(inputs)
      st = group.stats()
    assert 4 <= st['exchange_every'] < iterate and st['exchanges'] >= 1
    for name in stencil.output_names:
      lo, hi = stencil.valid_box(extent, name, iterate)
      idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
      assert np.array_equal(got[name][idx], want[name][idx])
      assert np.array_equal(got[name][idx], single[name][idx])


# ---------------------------------------------------------------------------
# GPU: the seams -- where a tile, a chunk or a slab ends
# ---------------------------------------------------------------------------

def _tiles_for_a_valid_row(name, fuse, iterate, dy, **kw):
  """The fewest whole valid tiles along y which, with `dy` rows more, leave
  `iterate` iterations of the program a valid row."""
  stencil = _stencil(name, iterate)
  vy = _valid_tile(name, fuse, **kw)[1]

  def rows(mul):
    boxes = [stencil.valid_box((1 << 12, mul * vy + dy, 1 << 12), out, iterate)
             for out in stencil.output_names]
    return min(hi[1] - lo[1] for lo, hi in boxes)

  mul = 1
  while rows(mul) < 1:
    mul += 1
  return mul


def _seam_id(case):
  return '%dx%+d_%dy%+d' % case


@pytest.mark.gpu
@pytest.mark.parametrize('case', SEAM_EXTENTS, ids=_seam_id)
@pytest.mark.parametrize('name', ['fwd3d', 'back3d', 'pair3d'])
def test_tile_seams(built, name, case):
  """The store masks at a tile's edge: who writes the last cells of the grid
  when it ends on, one cell before and one cell behind the edge of a tile."""
  from soda_amd.codegen.hip import lower
  iterate = 4
  extent = _grid(name, (4,), *case, 33)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 13)
  _run(stencil, extent, lower.LowerOptions(strategy='tile3d', fuse=(4,)),
       iterate, inputs, want, {4: 1}, tile=_valid_tile(name, (4,)))


@pytest.mark.gpu
@pytest.mark.parametrize('case', WIDE_EXTENTS, ids=_seam_id)
def test_tile_seams_with_two_columns_per_lane(built, case):
  from soda_amd.codegen.hip import lower
  iterate = 4
  extent = _grid('heat3d.soda', (4,), *case, 33, **WIDE)
  stencil = _stencil('heat3d.soda', iterate)
  inputs, want = _reference('heat3d.soda', extent, iterate, 13)
  _run(stencil, extent,
       lower.LowerOptions(strategy='tile3d', fuse=(4,), **WIDE), iterate,
       inputs, want, {4: 1}, tile=_valid_tile('heat3d.soda', (4,), **WIDE))


# (planes per chunk, planes of the grid): whole chunks; a last chunk of one
# plane; a last chunk one plane short; chunks shorter than the warm-up (12 to
# 14 steps at depth 4); and much shorter
CHUNK_SEAMS = [(16, 32), (16, 33), (16, 31), (8, 29), (4, 23)]
# Seven iterations of back3d (two rows a level) leave a grid of VY + 3 rows no
# valid row: that case runs -- every launch of it -- and must write nothing;
# the `tall` one is the same on as many tiles more as leave it rows to compare.
CHUNK_PROGRAMS = [(n, False) for n in sorted(SEAM_PROGRAMS)] + [('back3d', True)]


@pytest.mark.gpu
@pytest.mark.parametrize('chunk,planes', CHUNK_SEAMS)
@pytest.mark.parametrize('name,tall', CHUNK_PROGRAMS)
def test_chunk_seams(built, name, tall, chunk, planes):
  """Blocks that start at m_begin > 0: the clipped input window (wlo, in_end),
  the first step and the last (start, t_end) and the rebased buffers, with a
  reach along z that is one-sided, on every cell type tile3d accepts (float,
  int32, uint32), through both depths."""
  from soda_amd.codegen.hip import lower
  iterate, fuse = 7, (4, 3)
  need = _tiles_for_a_valid_row(name, fuse, iterate, 3)
  assert tall == (need > 1) or not tall
  extent = _grid(name, fuse, 1, 5, need if tall else 1, 3, planes)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 17)
  _run(stencil, extent,
       lower.LowerOptions(strategy='tile3d', fuse=fuse, chunk_rows=chunk),
       iterate, inputs, want, {4: 1, 3: 1}, empty=need > 1 and not tall,
       tile=_valid_tile(name, fuse))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['pair3d', 'fwd3d'])
def test_chunk_seams_of_a_deep_kernel(built, name):
  """Depth 6 (18 to 21 steps of warm-up) across chunks of 16 planes, two
  launches of it and one of the remainder pass."""
  from soda_amd.codegen.hip import lower
  iterate, fuse = 13, (6,)
  mod = _lowered(name, fuse)
  assert max(p.fused_iters for p in mod.passes) == 6      # not refused for LDS
  mul = _tiles_for_a_valid_row(name, fuse, iterate, 3)
  extent = _grid(name, fuse, 1, 5, mul, 3, 61)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 19)
  _run(stencil, extent,
       lower.LowerOptions(strategy='tile3d', fuse=fuse, chunk_rows=16),
       iterate, inputs, want, {6: 2, 1: 1}, tile=_valid_tile(name, fuse))


@pytest.mark.gpu
def test_large_planes_on_a_short_grid(built):
  """Planes of 8 MiB, 12 of them, chunks of 128 as declared: the library used
  to refuse it (a 128-plane window would pass 1 GiB; the grid has no 128)."""
  from soda_amd.codegen.hip import lower
  from oracle import c_oracle
  extent, iterate = (2048, 1024, 12), 4
  stencil = _stencil('heat3d.soda', iterate)
  inputs = _inputs(stencil, extent, 23)
  want = c_oracle.COracle(stencil).run(inputs, iterate=iterate)
  _run(stencil, extent, lower.LowerOptions(strategy='tile3d', fuse=(4,)),
       iterate, inputs, want, {4: 1})


# Split launches and cone runs: (program, tall).  Eight iterations of heat3d
# leave VY + 3 rows no valid row (see CHUNK_PROGRAMS).
SLAB_PROGRAMS = [('heat3d.soda', False), ('heat3d.soda', True),
                 ('fwd3d', False)]


def _slab_case(name, tall):
  iterate, fuse = 8, (4,)
  need = _tiles_for_a_valid_row(name, fuse, iterate, 3)
  assert tall == (need > 1) or not tall
  extent = _grid(name, fuse, 1, 5, need if tall else 1, 3, 160)
  return extent, iterate, need > 1 and not tall


@pytest.mark.gpu
@pytest.mark.parametrize('name,tall', SLAB_PROGRAMS)
def test_split_launches_of_virtual_slabs(built, monkeypatch, name, tall):
  """Slabs of several 16-plane chunks: the first and the last pass of an
  exchange interval go out in two launches, each of which skips a run of
  chunks (kargs skip_from / skip_count)."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  monkeypatch.setenv('SODA_HIP_NO_CALIBRATE', '1')
  extent, iterate, empty = _slab_case(name, tall)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 29)
  opts = lower.LowerOptions(strategy='tile3d', fuse=(4,), chunk_rows=16)
  with runtime.Program(stencil, opts, extent=extent, calibrate=False) as prog:
    assert prog.schedule(extent, iterate) == {4: 2}
    single = prog.run(inputs)
  _compare(stencil, extent, iterate, single, want, 'one device', empty)
  for slabs in (2, 3):
    for overlap in (True, False):
      # (an exchange after every launch: left to itself the library takes
      # two slabs of so small a grid through all 8 iterations without one)
      with runtime.Group(stencil, extent, [0] * slabs, opts, exchange_every=4,
                         overlap=overlap) as group:
        assert any('_tile3d_T4_' in k.name for k in group.module.kernels)
        got = group.run_host(inputs)
        st = group.stats()
      assert st['exchange_every'] == 4 and st['exchanges'] == 1
      if overlap:
        assert st['split_passes'] >= 1
      what = '%d slabs, overlap %s' % (slabs, overlap)
      _compare(stencil, extent, iterate, got, want, what, empty)
      for out in stencil.output_names:
        assert np.array_equal(got[out].view(np.uint32),
                              single[out].view(np.uint32)), what


@pytest.mark.gpu
@pytest.mark.parametrize('name,tall', SLAB_PROGRAMS)
def test_runs_that_keep_a_plane_range(built, name, tall):
  """soda_hip_run_device_cone through tile3d (tests/test_hip_parity.py
  test_runs_that_keep_a_row_range_skip_the_rest): launches on a window of the
  planes, the buffers offset to it."""
  import torch
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  extent, iterate, empty = _slab_case(name, tall)
  keep = (50, 110)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 29)
  opts = lower.LowerOptions(strategy='tile3d', fuse=(4,), chunk_rows=16)
  with runtime.Program(stencil, opts, extent=extent, calibrate=False) as prog:
    assert prog.schedule(extent, iterate) == {4: 2}
    # (the shared reference arrays are read-only: copied on the way)
    src = [torch.tensor(inputs[n]).cuda() for n in stencil.input_names]
    full = [torch.zeros_like(src[0]) for _ in stencil.output_names]
    part = [torch.full_like(src[0], 77) for _ in stencil.output_names]
    s = torch.cuda.current_stream().cuda_stream
    prog.run_device([t.data_ptr() for t in full], [t.data_ptr() for t in src],
                    extent, stream=s)
    rows_full = prog.last_rows()
    prog.run_device([t.data_ptr() for t in part], [t.data_ptr() for t in src],
                    extent, stream=s, keep=keep)
    rows_part = prog.last_rows()
    torch.cuda.synchronize()
  assert rows_full == 2 * extent[2] and rows_part < rows_full
  for out, a, b in zip(stencil.output_names, full, part):
    lo, hi = stencil.valid_box(extent, out, iterate)
    assert lo[2] < keep[0] and keep[1] < hi[2]
    box = tuple(slice(l, max(l, h)) for l, h in zip(lo[::-1], hi[::-1]))
    kept = (slice(keep[0], keep[1]),) + box[1:]
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert empty == (a[kept].size == 0)
    assert np.array_equal(a[kept].view(np.uint32), b[kept].view(np.uint32))
    assert np.array_equal(b[kept].view(np.uint32),
                          want[out][kept].view(np.uint32))
    # the planes no launch of the last pass covered keep what they held
    reach_lo, reach_hi = stencil.reach_along(2)
    assert (b[:keep[0] - 4 * reach_lo] == 77).all()
    assert (b[keep[1] + 4 * reach_hi:] == 77).all()


# Nine iterations of heat3d leave 2 VY + 1 rows no valid row (CHUNK_PROGRAMS)
@pytest.mark.gpu
@pytest.mark.parametrize('name,tall', [('heat3d.soda', False),
                                       ('heat3d.soda', True), ('u32', False)])
def test_first_run_times_the_passes(built, monkeypatch, name, tall):
  """The default path: no calibrate= argument.  The first run of an extent
  times every pass on stand-in arrays (a tile3d pass has no model to fall back
  on) and is then scheduled by the clock -- whichever mix that is."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  monkeypatch.delenv('SODA_HIP_NO_CALIBRATE', raising=False)
  iterate, fuse = 9, (4, 3)
  need = max(2, _tiles_for_a_valid_row(name, fuse, iterate, 1))
  assert tall == (need > 2) or not tall
  extent = _grid(name, fuse, 2, 1, need if tall else 2, 1, 40)
  stencil = _stencil(name, iterate)
  inputs, want = _reference(name, extent, iterate, 31)
  opts = lower.LowerOptions(strategy='tile3d', fuse=fuse)
  with runtime.Program(stencil, opts, extent=extent) as prog:
    assert prog.pass_times(extent)[1] is False
    got = prog.run(inputs, iterate=iterate)
    times, measured = prog.pass_times(extent)
    sched = prog.schedule(extent, iterate)
    names = [k.name for k in prog.module.kernels]
  assert measured and sorted(times) == [1, 3, 4]
  assert all(t > 0 for t in times.values()), times
  assert sum(t * n for t, n in sched.items()) == iterate
  _compare(stencil, extent, iterate, got, want, names,
           empty=need > 2 and not tall)
