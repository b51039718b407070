"""`tile3d`: the LDS-tiled 3-D kernels that fuse more than two iterations
(soda_amd/codegen/hip/tile3d.py).  CPU tests: what lower() builds, what it
refuses, what the compiled kernels need.  GPU tests: bit for bit against the C
oracle on the valid box, nothing written outside it, through runtime.Program
(the C ABI).

GPU runs are built with calibrate=False: a tile3d pass carries no time model,
so the library's scheduler then goes deepest pass first (soda_hip.cpp
`schedule`) and the test KNOWS which kernels ran -- it asserts the schedule.
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
  from soda_amd import core
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


def _run(stencil, extent, opts, iterate, inputs, want, expect, empty=False):
  """Runs on the GPU with the deepest-first schedule, asserts that schedule is
  `expect` ({depth: launches}) and compares with the oracle."""
  from soda_amd import runtime
  with runtime.Program(stencil, opts, extent=extent, calibrate=False) as prog:
    sched = {t: n for t, n in prog.schedule(extent, iterate).items() if n}
    assert sched == expect
    kinds = {p.fused_iters: p.kind for p in prog.module.passes}
    assert all(kinds[t] == 'tile3d' for t in sched if t > 1)
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
