"""Residual of a run's last iteration (`LowerOptions.residual`,
soda_hip_run_device_residual / _until).

The four fields are sums and maxima of exact per-cell values, so every
comparison here is `==` on all of them.  Expected values come from the C
oracle at `iterate = N` and `N - 1` with the definition applied in numpy, in
the cell's dtype, over `valid_box`.

CPU: the default text is what it was, the marching kernels have twins that
compile without spilling, `<app>_residual` exists in every family, the
refusals, the plan, the box the library derives, the command line.  GPU: the
seams of the marching kernels in 2-D and 3-D (strips, chunks, tiles, a ragged
last strip), multi-stage and two-pair programs, the generic kernel behind the
other families, the whole value domain, guard bands, a live stream, a graph,
and `run_until`."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import asyncrun
import guarded
import values

SUFFIX = '_rs'

# (program, iterate, options): tests/test_batch.py FAMILIES
FAMILIES = [
    ('jacobi2d.soda', 30, dict(fuse=(13,))),
    ('heat3d.soda', 4, dict(fuse=(2,))),
    ('blur.soda', None, dict()),
    ('contrast.soda', None, dict()),                         # ldswin
    ('heat4d.soda', None, dict()),                           # direct
    ('heat3d.soda', 4, dict(strategy='tile3d', fuse=(3,))),
]

INT32_2D = '''kernel: diff32
burst width: 64
unroll factor: 2
iterate: 2
input int32: a(32, *)
output int32: b(0, 0) = a(0, 1) - a(0, -1) + a(1, 0)
'''
UINT16_2D = '''kernel: mix16
burst width: 64
unroll factor: 2
iterate: 2
input uint16: a(32, *)
output uint16: b(0, 0) = a(-1, 0) * 3 + a(1, 0) - a(0, 1)
'''
INT64_2D = '''kernel: wide64
burst width: 64
unroll factor: 2
iterate: 2
input int64: a(32, *)
output int64: b(0, 0) = a(0, 1) - a(0, -1) + a(-1, 0)
'''
FP64_2D = '''kernel: avg64
burst width: 64
unroll factor: 2
iterate: 2
input double: a(32, *)
output double: b(0, 0) = (a(0, 1) + a(0, -1) + a(1, 0) + a(-1, 0)) * 0.25
'''
LINE_1D = '''kernel: line1d
burst width: 64
unroll factor: 2
iterate: 3
input float: a(*)
output float: b(0) = (a(-1) + a(0) + a(1)) * 0.25f
'''


def _stencil(name, **kw):
  from soda_amd import core
  kw = {k: v for k, v in kw.items() if v is not None}
  if name.endswith('.soda'):
    return core.from_file(soda_path(name), **kw)
  return core.from_text(name, **kw)


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('residual', True)
  return lower.LowerOptions(**kw)


def _march(mod):
  return [k for k in mod.kernels if k.tune and 'axis' in k.tune]


# ---------------------------------------------------------------------------
# the definition, in numpy
# ---------------------------------------------------------------------------

def _delta(cur, prev):
  """(changed, unordered, max_float, max_int) of two arrays of one dtype."""
  assert cur.dtype == prev.dtype and cur.shape == prev.shape
  if cur.size == 0:
    return 0, 0, 0.0, 0
  if cur.dtype.kind == 'f':
    with np.errstate(all='ignore'):
      d = np.abs(cur - prev)            # one IEEE operation in the cell's type
    assert d.dtype == cur.dtype
    nan = np.isnan(d)
    ordered = d[~nan]
    return (int(np.count_nonzero(~(d == 0))), int(nan.sum()),
            float(ordered.max()) if ordered.size else 0.0, 0)
  if cur.dtype.itemsize < 8:
    d = np.abs(cur.astype(np.int64) - prev.astype(np.int64))
  else:
    hi, lo = np.maximum(cur, prev), np.minimum(cur, prev)
    d = hi.astype(np.uint64) - lo.astype(np.uint64)    # wraps to the exact value
  return int(np.count_nonzero(d)), 0, 0.0, int(d.max())


_ORACLES = {}


def _oracle(stencil):
  from oracle import c_oracle
  key = str(stencil)
  if key not in _ORACLES:
    _ORACLES[key] = c_oracle.COracle(stencil, openmp=False)
  return _ORACLES[key]


def _expected(stencil, ins, extent, iterate):
  """(Residual as a tuple, {output: oracle array after `iterate`})."""
  orc = _oracle(stencil)
  cur = orc.run(ins, iterate=iterate)
  prev = orc.run(ins, iterate=iterate - 1) if iterate > 1 else None
  changed = unordered = max_int = 0
  max_float = 0.0
  for i, o in zip(stencil.input_names, stencil.output_names):
    lo, hi = stencil.valid_box(extent, o, iterate)
    box = tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]
    before = prev[o] if prev is not None else np.asarray(ins[i])
    c, u, f, m = _delta(cur[o][box], before[box])
    changed, unordered = changed + c, unordered + u
    max_float, max_int = max(max_float, f), max(max_int, m)
  return (changed, unordered, max_float, max_int), cur


def _fields(res):
  return (res.changed, res.unordered, res.max_float, res.max_int)


def test_the_definition_on_the_issue_table(built):
  """jacobi2d border='preserve', shape (40, 64), default_rng(7).random(float32):
  the figures the feature's description gives, from the oracle on this CPU."""
  stencil = _stencil('jacobi2d.soda', iterate=64, border='preserve')
  ins = {'t1': np.random.default_rng(7).random((40, 64), dtype=np.float32)}
  for n, changed, max_float in ((1, 2356, 0.6604659), (16, 2356, 0.005204678),
                                (32, 2356, 0.002126694), (64, 2355, 0.000624001)):
    got, _ = _expected(stencil, ins, (64, 40), n)
    assert got[0] == changed and got[1] == 0 and got[3] == 0, (n, got)
    assert abs(got[2] - max_float) < 1e-6 * max_float, (n, got)


def test_delta_value_domain():
  f = np.float32
  cur = np.array([np.nan, np.inf, np.inf, 0.0, 1.5, 1e-45, -np.inf], f)
  prev = np.array([1.0, np.inf, -np.inf, -0.0, 1.0, 0.0, 3.0], f)
  assert _delta(cur, prev) == (6, 2, float('inf'), 0)
  a = np.array([-2**31, 5, 7], np.int32)
  b = np.array([2**31 - 1, 5, 4], np.int32)
  assert _delta(a, b) == (2, 0, 0.0, 2**32 - 1)
  a = np.array([-2**63, 1], np.int64)
  b = np.array([2**63 - 1, 1], np.int64)
  assert _delta(a, b) == (1, 0, 0.0, 2**64 - 1)


# ---------------------------------------------------------------------------
# CPU: text, twins, plan, refusals, command line
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name,iterate,kw', FAMILIES)
def test_default_text_is_unchanged(name, iterate, kw):
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=iterate)
  plain = lower.lower(stencil, lower.LowerOptions(peel=0, **kw))
  same = lower.lower(stencil, lower.LowerOptions(residual=False, peel=0, **kw))
  assert same.source == plain.source
  assert [k.name for k in same.kernels] == [k.name for k in plain.kernels]
  assert 'soda_res' not in plain.source
  assert not any(k.name.endswith(SUFFIX) or k.name.endswith('_residual')
                 for k in plain.kernels)
  assert all(k.twin == -1 for k in plain.kernels)


@pytest.mark.parametrize('name,iterate,kw', FAMILIES)
def test_every_family_has_the_generic_kernel(name, iterate, kw):
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=iterate)
  plain = lower.lower(stencil, lower.LowerOptions(peel=0, **kw))
  mod = lower.lower(stencil, _opts(peel=0, **kw))
  names = [k.name for k in mod.kernels]
  assert names[mod.residual_kernel] == '%s_residual' % stencil.app_name
  assert names.count('%s_residual' % stencil.app_name) == 1
  assert names[mod.residual_zero_kernel] == '%s_residual_zero' % stencil.app_name
  # every default kernel is still there, its text unchanged
  for k, chunk in zip(plain.kernels, plain.chunks):
    assert mod.chunks[names.index(k.name)] == chunk, k.name
  # residual kernels are kernels, not passes
  in_a_pass = {i for p in mod.passes for i in p.kernels}
  assert [p.fused_iters for p in mod.sorted_passes()] == \
      [p.fused_iters for p in plain.sorted_passes()]
  for i, k in enumerate(mod.kernels):
    if k.name.endswith(SUFFIX) or '_residual' in k.name:
      assert i not in in_a_pass, k.name


TWINS = [
    ('jacobi2d.soda', 30, dict(fuse=(13, 12, 8, 4)), None),
    ('heat3d.soda', 4, dict(fuse=(2,)), None),
    ('jacobi2d.soda', 30, dict(fuse=(8, 4)), 'preserve'),
    ('blur.soda', 2, dict(fuse=(2,)), None),
    ('coupled2d.soda', 3, dict(fuse=(3,)), None),
]


@pytest.mark.parametrize('name,iterate,kw,border', TWINS)
def test_twins_present_and_compile_without_spills(built, name, iterate, kw,
                                                  border):
  """Every marching kernel has a twin, at every depth lower() builds; the
  plain kernels' text is that of the default build; the twins compile for
  gfx950 without scratch.  (profiles/residual_regs.json records the register
  counts; the numbers asserted here are the compiled ones.)"""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=iterate, border=border)
  # the forms `auto` produces: mixh from depth 8 on, dpp below, one trip of
  # the warm-up peeled (without the trial compilations of select_peel)
  plain = lower.lower(stencil, lower.LowerOptions(peel=1, **kw))
  mod = lower.lower(stencil, _opts(peel=1, **kw))
  names = [k.name for k in mod.kernels]
  marching = [k for k in _march(mod) if not k.name.endswith(SUFFIX)]
  assert [k.name for k in marching] == [k.name for k in _march(plain)]
  assert len(marching) == len(set(min(t, iterate) for t in kw['fuse'])) + 1
  for k in marching:
    assert k.twin >= 0, '%s has no twin' % k.name
    assert names[k.twin] == k.name + SUFFIX
    assert mod.chunks[names.index(k.name)] == \
        plain.chunks[[q.name for q in plain.kernels].index(k.name)]
    assert mod.kernels[k.twin].tile == k.tile       # the same stores
  if name == 'jacobi2d.soda' and border is None:
    assert any('_mixh' in k.name for k in marching)
    assert any('_mixh' not in k.name for k in marching)
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, '%s.hip' % stencil.app_name))
  for k in marching:
    twin = res[k.name + SUFFIX]
    assert twin['scratch'] == 0, (k.name, twin)
    assert 0 < twin['vgpr'] <= 512
    assert res[k.name]['scratch'] == 0
  assert res['%s_residual' % stencil.app_name]['scratch'] == 0
  plan = runtime.make_plan(mod, res)
  for i, k in enumerate(mod.kernels):
    assert plan.kernels[i].twin == k.twin


def test_refusals():
  from soda_amd import util
  from soda_amd.codegen.hip import lower
  jac = _stencil('jacobi2d.soda', iterate=4)
  with pytest.raises(util.SemanticError, match='residual.*batch'):
    lower.lower(jac, _opts(batch=True, peel=0))
  with pytest.raises(util.SemanticError, match='residual.*banks'):
    lower.lower(jac, _opts(banks={'t1': 2}, peel=0))
  # not iterable, as tile3d_supported words it: two inputs, one output
  with pytest.raises(util.SemanticError, match='residual.*iterable'):
    lower.lower(_stencil('denoise2d.soda'), _opts(peel=0))
  # ... or one of each, of different types
  with pytest.raises(util.SemanticError, match='residual.*iterable'):
    lower.lower(_stencil('sobel2d.soda'), _opts(peel=0))
  # blur maps uint16 to uint16: iterable by that wording, and accepted
  mod = lower.lower(_stencil('blur.soda'), _opts(peel=0))
  assert mod.kernels[mod.residual_kernel].name == 'blur_residual'


def test_plan_carries_the_twins(built):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  assert runtime.ABI_VERSION == 9
  assert runtime.library().soda_hip_abi_version() == 9
  stencil = _stencil('jacobi2d.soda', iterate=8)
  mod = lower.lower(stencil, _opts(fuse=(4,), peel=0))
  plan = runtime.make_plan(mod)
  assert plan.abi_version == 9
  assert plan.residual.present == 1
  assert plan.residual.kernel == mod.residual_kernel
  assert plan.residual.zero_kernel == mod.residual_zero_kernel
  assert [plan.kernels[i].twin for i in range(plan.num_kernels)] == \
      [k.twin for k in mod.kernels]
  assert sorted(t for t in (k.twin for k in mod.kernels) if t >= 0) == \
      [i for i, k in enumerate(mod.kernels) if k.name.endswith(SUFFIX)]
  assert plan.num_kernels <= runtime.MAX_KERNELS
  assert plan.num_passes == 2                      # twins are not passes
  # check_plan accepts it (the geometry entry checks the plan first) ...
  runtime.plan_geometry(plan, (64, 32))
  # ... and refuses a twin index outside the plan
  plan.kernels[0].twin = plan.num_kernels
  with pytest.raises(Exception, match='twin'):
    runtime.plan_geometry(plan, (64, 32))
  # a plan without the option says so
  bare = runtime.make_plan(lower.lower(stencil, lower.LowerOptions(fuse=(4,),
                                                                   peel=0)))
  assert bare.residual.present == 0
  assert all(bare.kernels[i].twin == -1 for i in range(bare.num_kernels))


BOXES = [
    ('jacobi2d.soda', None, (40, 30)),
    ('jacobi2d.soda', 'preserve', (40, 30)),
    ('coupled2d.soda', None, (24, 20)),
    ('skew2d.soda', None, (40, 30)),
    ('erosion.soda', None, (64, 80)),
    ('heat3d.soda', None, (16, 12, 10)),
    (LINE_1D, None, (40,)),
]


@pytest.mark.parametrize('name,border,extent', BOXES)
def test_the_library_derives_the_valid_box(built, name, border, extent):
  """soda_hip_plan_residual_box, from the recurrence in the plan, against
  core.Stencil.valid_box, also where the box runs empty."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=2, border=border)
  assert stencil_iterable(stencil)
  plan = runtime.make_plan(lower.lower(stencil, _opts(peel=0)))
  dim, n = stencil.dim, len(stencil.output_names)
  ext = (ctypes.c_int32 * 4)(*(list(extent) + [1] * (4 - dim)))
  for iterate in (1, 2, 3, 7, 40):
    lo, hi = (ctypes.c_int32 * (n * dim))(), (ctypes.c_int32 * (n * dim))()
    runtime.check(runtime.library().soda_hip_plan_residual_box(
        ctypes.byref(plan), ext, iterate, lo, hi), 'box')
    for o, out in enumerate(stencil.output_names):
      want = runtime.clipped_box(stencil.valid_box(extent, out, iterate), extent)
      assert (list(lo[o * dim:(o + 1) * dim]),
              list(hi[o * dim:(o + 1) * dim])) == (want[0], want[1]), \
          (out, iterate)


def stencil_iterable(stencil):
  return len(stencil.input_names) == len(stencil.output_names) and \
      list(stencil.input_types) == list(stencil.output_types)


def test_sodac_prints_a_twin():
  out = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', '--hip-residual',
       '--hip-no-probe', '--hip-kernel', '-', soda_path('jacobi2d.soda')],
      cwd=ROOT, capture_output=True, text=True, check=True).stdout
  assert SUFFIX + '(soda_hip_kargs_t a, soda_hip_residual_t* soda_res' in out
  assert 'jacobi2d_residual(soda_hip_kargs_t a' in out
  plain = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', '--hip-no-probe',
       '--hip-kernel', '-', soda_path('jacobi2d.soda')],
      cwd=ROOT, capture_output=True, text=True, check=True).stdout
  assert 'soda_res' not in plain


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

class _Device:
  """Device arrays through the library's own memory calls."""

  def __init__(self):
    from soda_amd import runtime
    self.rt, self.lib, self.ptrs = runtime, runtime.library(), []

  def alloc(self, nbytes, fill=None):
    p = ctypes.c_void_p()
    self.rt.check(self.lib.soda_hip_malloc(0, max(16, nbytes), ctypes.byref(p)),
                  'malloc')
    self.ptrs.append(p)
    if fill is not None:
      self.rt.check(self.lib.soda_hip_memset(p, fill, nbytes, None), 'memset')
    return p.value

  def upload(self, arr):
    arr = np.ascontiguousarray(arr)
    p = self.alloc(arr.nbytes)
    self.rt.check(self.lib.soda_hip_memcpy_h2d(ctypes.c_void_p(p),
                                               arr.ctypes.data, arr.nbytes,
                                               None), 'h2d')
    return p

  def download(self, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    self.rt.check(self.lib.soda_hip_memcpy_d2h(out.ctypes.data,
                                               ctypes.c_void_p(ptr),
                                               out.nbytes, None), 'd2h')
    return out

  def close(self):
    for p in self.ptrs:
      self.lib.soda_hip_free(0, p)
    self.ptrs = []

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


def _inputs(stencil, extent, seed=7):
  rng = np.random.default_rng(seed)
  shape = tuple(extent[::-1])
  out = {}
  for n, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if t.is_float:
      out[n] = rng.random(shape, dtype=np.float64).astype(dt)
    else:
      out[n] = values._full(rng, shape, dt)
  return out


def _run(prog, stencil, extent, ins, iterate):
  """({output: array}, Residual, how) of one residual run on fresh arrays; the
  struct starts as 0xFF bytes (the call zeroes it itself)."""
  shape = tuple(extent[::-1])
  with _Device() as dev:
    din = [dev.upload(ins[n]) for n in stencil.input_names]
    dout = [dev.alloc(int(np.prod(shape)) * np.dtype(t.np_name).itemsize,
                      fill=0xA5) for t in stencil.output_types]
    res = dev.alloc(32, fill=0xFF)
    prog.run_device(dout, din, extent, iterate, residual=res)
    got = prog.residual(res)
    outs = {o: dev.download(p, shape, np.dtype(t.np_name))
            for o, p, t in zip(stencil.output_names, dout,
                               stencil.output_types)}
    # inputs are never written
    for n, p in zip(stencil.input_names, din):
      assert np.array_equal(
          dev.download(p, shape, ins[n].dtype).view(np.uint8),
          np.ascontiguousarray(ins[n]).view(np.uint8)), n
  return outs, got, prog.last_residual()


def _check(prog, stencil, extent, ins, iterate, how=None):
  want, cur = _expected(stencil, ins, extent, iterate)
  outs, got, mode = _run(prog, stencil, extent, ins, iterate)
  for o in stencil.output_names:
    lo, hi = stencil.valid_box(extent, o, iterate)
    box = tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]
    assert values.same_bits(outs[o][box], cur[o][box]).all(), \
        'output %s differs from the oracle (iterate %d)' % (o, iterate)
  assert _fields(got) == want, (iterate, mode, got, want)
  if how is not None:
    assert mode[0] == how, mode
  return got, mode


@pytest.fixture(scope='module')
def jacobi(built):
  """jacobi2d fuse=(13, 4), chunks of 16 rows, border ignore and preserve (the
  latter is capped at depth 8): mixh twins at 13 / 8, dpp twins at 4 / 1, a
  trip of the warm-up peeled."""
  from soda_amd import runtime
  progs = {}
  for border in ('ignore', 'preserve'):
    stencil = _stencil('jacobi2d.soda', iterate=13, border=border)
    progs[border] = (stencil, runtime.Program(
        stencil, _opts(fuse=(13, 4), chunk_rows=16, peel=1),
        calibrate=False))
  yield progs
  for _, prog in progs.values():
    prog.close()


@pytest.mark.gpu
@pytest.mark.parametrize('border', ['ignore', 'preserve'])
@pytest.mark.parametrize('cells', [520, 516])
@pytest.mark.parametrize('iterate', [1, 5, 13])
def test_2d_seams(jacobi, border, cells, iterate):
  """520 x 56 at 4 cells per lane: two full strips plus a ragged third, four
  chunks of 16 rows; 516 cells per row: another ragged lane count.  A cell in
  a strip halo, in a chunk's warm-up rows or past the row's end counts once or
  not at all.  The pass launched last is the deepest scheduled one, as its
  twin."""
  stencil, prog = jacobi[border]
  names = [k.name for k in prog.module.kernels]
  assert all(k.twin >= 0 for k in _march(prog.module)
             if not k.name.endswith(SUFFIX)), names
  extent = (cells, 56)
  ins = _inputs(stencil, extent)
  _, mode = _check(prog, stencil, extent, ins, iterate, how='twin')
  deepest = max(prog.schedule(extent, iterate))
  assert mode[1] == deepest, (mode, prog.schedule(extent, iterate))
  if iterate == 13:
    assert deepest == (13 if border == 'ignore' else 8)


@pytest.fixture(scope='module')
def heat(built):
  from soda_amd import runtime
  stencil = _stencil('heat3d.soda', iterate=3)
  extent = (136, 10, 20)
  strips = runtime.Program(stencil, _opts(fuse=(2,), chunk_rows=8, peel=1),
                           calibrate=False)
  rows = runtime.Program(stencil, _opts(fuse=(2,), chunk_rows=8, peel=1),
                         extent=extent, calibrate=False)
  yield stencil, extent, {'strips': strips, 'rows': rows}
  strips.close()
  rows.close()


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['strips', 'rows'])
@pytest.mark.parametrize('iterate', [1, 2, 3])
def test_3d_seams(heat, form, iterate):
  """heat3d 136 x 10 x 20, tiles of 4 rows (three, the last ragged), chunks of
  8 planes (three): built without an extent the fused kernel runs overlapping
  strips, built for the extent its block covers the whole row (`_xs`).  The
  whole-row twin is kept only where it compiles without spilling; where it is
  dropped the run ends in the one-iteration twin or `<app>_residual`, and the
  figures are the same."""
  stencil, extent, progs = heat
  prog = progs[form]
  fused, = [k for k in _march(prog.module)
            if k.tune['fused'] == 2 and not k.name.endswith(SUFFIX)]
  assert ('_xs' in fused.name) == (form == 'rows'), fused.name
  ins = _inputs(stencil, extent)
  _, mode = _check(prog, stencil, extent, ins, iterate)
  twins = {k.tune['fused'] for i, k in enumerate(_march(prog.module))
           if not k.name.endswith(SUFFIX) and
           prog.plan.kernels[[q.name for q in prog.module.kernels]
                             .index(k.name)].twin >= 0}
  scheduled = set(prog.schedule(extent, iterate))
  assert mode[0] == ('twin' if scheduled & twins else 'generic'), \
      (mode, scheduled, twins)
  assert 1 in twins
  if form == 'strips':
    assert 2 in twins


@pytest.mark.gpu
def test_multi_stage_program(built):
  """blur at iterate = 2: a local between the input and the output, 8 cells of
  uint16 per lane, 264 x 40."""
  from soda_amd import runtime
  stencil = _stencil('blur.soda', iterate=2)
  extent = (264, 40)
  with runtime.Program(stencil, _opts(fuse=(2,), peel=1),
                       calibrate=False) as prog:
    ins = _inputs(stencil, extent)
    for iterate in (1, 2):
      _check(prog, stencil, extent, ins, iterate, how='twin')


@pytest.mark.gpu
def test_two_pair_program(built):
  """coupled2d: two inputs, two outputs, a shared local; the struct is taken
  over both pairs, each on its own valid box."""
  from soda_amd import runtime
  stencil = _stencil('coupled2d.soda', iterate=3)
  extent = (264, 40)
  with runtime.Program(stencil, _opts(fuse=(3,), peel=1),
                       calibrate=False) as prog:
    ins = _inputs(stencil, extent)
    boxes = {stencil.valid_box(extent, o, 3) for o in stencil.output_names}
    assert len(boxes) == 2, 'the pairs should count different boxes'
    for iterate in (1, 3):
      _check(prog, stencil, extent, ins, iterate, how='twin')


GENERIC = [
    ('heat4d.soda', 2, dict(), (24, 10, 6, 5), 'direct'),
    ('heat3d.soda', 4, dict(strategy='tile3d', fuse=(3,)), (72, 12, 16),
     'tile3d'),
    ('contrast.soda', 2, dict(strategy='ldswin'), (128, 80), 'ldswin'),
    (LINE_1D, 3, dict(), (300,), 'direct'),
    ('jacobi2d.soda', 5, dict(strategy='direct', vec=4), (40, 30), 'direct'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,iterate,kw,extent,family', GENERIC,
                         ids=['heat4d', 'tile3d', 'ldswin', 'line1d',
                              'direct_v4'])
def test_generic_path(built, name, iterate, kw, extent, family):
  """Families without twins end the run in a one-iteration pass and
  `<app>_residual` over the outputs and that pass's inputs -- one launch more
  than the passes -- in 1 to 4 dimensions."""
  from soda_amd import runtime
  stencil = _stencil(name, iterate=iterate)
  with runtime.Program(stencil, _opts(peel=0, **kw), extent=extent,
                       calibrate=False) as prog:
    names = [k.name for k in prog.module.kernels]
    if family == 'tile3d':
      assert any('tile3d' in n for n in names), names
    else:
      assert any(family in n for n in names), names
      assert not any(n.endswith(SUFFIX) for n in names), names
    ins = _inputs(stencil, extent)
    for n in ((3, 4) if family == 'tile3d' else sorted({1, iterate})):
      _, mode = _check(prog, stencil, extent, ins, n)
      if family == 'tile3d':
        # 3 = one fused tile3d pass, which has no twin: the run is re-cut into
        # one-iteration passes and ends in `<app>_residual`.  4 = 3 + 1: the
        # one-iteration pass is a marching kernel's and has a twin
        assert mode == (('generic', 1) if n == 3 else ('twin', 1)), mode
        if n == 3:
          assert prog.last_launches()[0] == 3 + 1
      else:
        assert mode[0] == 'generic', mode
        launches = prog.last_launches()[0]
        one, = [p for p in prog.module.sorted_passes() if p.fused_iters == 1]
        assert launches == n * len(one.kernels) + 1, (launches, n)


@pytest.mark.gpu
def test_forced_generic_is_the_same(jacobi, monkeypatch):
  """SODA_HIP_RESIDUAL_GENERIC=1 (the A/B arm): 13 = 12 + 1 iterations, the
  last one alone, then `<app>_residual` -- the same struct as the twin's."""
  stencil, prog = jacobi['ignore']
  extent = (520, 56)
  ins = _inputs(stencil, extent)
  monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
  _, mode = _check(prog, stencil, extent, ins, 13, how='generic')
  assert mode[1] == 1


VALUE_PROGRAMS = [
    (INT32_2D, 2, dict(fuse=(2,)), (264, 24)),
    (UINT16_2D, 2, dict(fuse=(2,)), (264, 24)),
    (INT64_2D, 2, dict(fuse=(2,)), (264, 24)),
    (FP64_2D, 2, dict(fuse=(2,)), (264, 24)),
    ('ints2d.soda', 2, dict(fuse=(2,)), (272, 24)),
    ('erosion.soda', 2, dict(fuse=(2,)), (272, 64)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,iterate,kw,extent', VALUE_PROGRAMS,
                         ids=['int32', 'uint16', 'int64', 'fp64', 'ints2d',
                              'erosion'])
def test_integer_and_wide_cells(built, name, iterate, kw, extent):
  """Full-range values: max_int is exact -- above 2^31 for int32, above 2^63
  for int64 -- and a double delta keeps its own precision."""
  from soda_amd import runtime
  stencil = _stencil(name, iterate=iterate)
  with runtime.Program(stencil, _opts(peel=1, **kw), calibrate=False) as prog:
    ins = _inputs(stencil, extent, seed=11)
    for n in (1, iterate):
      got, _ = _check(prog, stencil, extent, ins, n)
      kind = str(stencil.output_types[0])
      if kind == 'int32':
        assert got.max_int > 2**31
      if kind == 'int64':
        assert got.max_int > 2**63
      if kind == 'double':
        assert got.max_float != float(np.float32(got.max_float))
        assert got.max_int == 0
      if kind in ('uint16', 'int16', 'uint8'):
        assert 0 < got.max_int <= np.iinfo(kind).max - np.iinfo(kind).min


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['nonfinite', 'tiny', 'signed'])
@pytest.mark.parametrize('border', ['ignore', 'preserve'])
def test_float_value_domain(jacobi, kind, border):
  """NaNs, both infinities, both zeros, subnormals: `unordered`, `changed`
  and `max_float` are exact, and max_float is +inf where the oracle says so."""
  stencil, prog = jacobi[border]
  extent = (520, 56)
  at = [(10, 9), (300, 20), (511, 30), (12, 9), (301, 21), (200, 40)]
  ins = values.edge_inputs(stencil, extent, 3, kind,
                           at=at if kind == 'nonfinite' else None)
  for iterate in (1, 5):
    got, _ = _check(prog, stencil, extent, ins, iterate, how='twin')
    if kind == 'nonfinite':
      assert got.unordered > 0 and got.changed >= got.unordered
      assert got.max_float == float('inf')
    else:
      assert got.unordered == 0 and 0 < got.max_float < float('inf')


@pytest.mark.gpu
@pytest.mark.parametrize('border', ['ignore', 'preserve'])
def test_all_zero_input_gives_zeros(jacobi, border):
  stencil, prog = jacobi[border]
  extent = (520, 56)
  ins = {'t1': np.zeros(extent[::-1], np.float32)}
  for iterate in (1, 13):
    got, _ = _check(prog, stencil, extent, ins, iterate, how='twin')
    assert _fields(got) == (0, 0, 0.0, 0)
  # -0.0 against +0.0 is unchanged
  ins = {'t1': np.full(extent[::-1], -0.0, np.float32)}
  got, _ = _check(prog, stencil, extent, ins, 1, how='twin')
  assert _fields(got) == (0, 0, 0.0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('border,iterate', [('ignore', 13), ('preserve', 5),
                                            ('ignore', 1)])
def test_guard_bands(jacobi, border, iterate, monkeypatch):
  """The residual entry between guard bands: no byte outside the outputs and
  the 32-byte struct is written; the struct sits between guard bytes of its
  own.  Once through a twin, once through `<app>_residual`."""
  stencil, prog = jacobi[border]
  extent = (516, 56)
  ins = _inputs(stencil, extent)
  want, cur = _expected(stencil, ins, extent, iterate)
  for generic in (False, True):
    if generic:
      monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
    with _Device() as dev:
      band = 4096
      arena = dev.alloc(2 * band + 32, fill=0xA5)
      outs, bad, _ = guarded.run(prog, stencil, extent, ins, iterate,
                                 residual=arena + band)
      assert bad is None, bad
      img = dev.download(arena, (2 * band + 32,), np.uint8)
    assert (img[:band] == 0xA5).all() and (img[band + 32:] == 0xA5).all()
    raw = img[band:band + 32].view(np.uint64)
    assert (int(raw[0]), int(raw[1]), float(raw[2:3].view(np.float64)[0]),
            int(raw[3])) == want
    assert prog.last_residual()[0] == ('generic' if generic else 'twin')
    lo, hi = stencil.valid_box(extent, None, iterate)
    box = tuple(slice(l, h) for l, h in zip(lo, hi))[::-1]
    o = stencil.output_names[0]
    assert values.same_bits(outs[o][box], cur[o][box]).all()


@pytest.mark.gpu
def test_side_stream_ahead_of_its_inputs(jacobi):
  """The entry enqueued on a live stream ahead of its inputs: the zeroing, the
  passes and the twin are all ordered on that stream."""
  stencil, prog = jacobi['ignore']
  extent = (520, 56)
  shape = extent[::-1]
  ins = _inputs(stencil, extent)
  want, cur = _expected(stencil, ins, extent, 13)
  # warm: scratch exists, the call below allocates nothing
  _run(prog, stencil, extent, ins, 13)
  out_like = {'t0': (shape, np.float32), 'soda_residual': ((4,), np.uint64)}

  def enqueue(run):
    out, res = run.outs()
    prog.run_device([out], run.ins(), extent, 13, stream=run.ptr, residual=res)

  got = asyncrun.late_fill('residual run', {'t1': ins['t1']}, out_like, enqueue)
  raw = got['soda_residual']
  assert (int(raw[0]), int(raw[1]), float(raw[2:3].view(np.float64)[0]),
          int(raw[3])) == want
  lo, hi = stencil.valid_box(extent, None, 13)
  box = tuple(slice(l, h) for l, h in zip(lo, hi))[::-1]
  assert values.same_bits(got['t0'][box], cur['t0'][box]).all()


@pytest.mark.gpu
def test_capture_and_replay(jacobi):
  """Captured after one eager call, replayed twice: both replays yield the
  eager struct -- the zeroing is part of the call -- even when the struct holds
  other bytes before each replay."""
  import torch
  stencil, prog = jacobi['preserve']
  extent = (520, 56)
  ins = _inputs(stencil, extent)
  want, _ = _expected(stencil, ins, extent, 5)
  S = torch.cuda.Stream()
  a = torch.from_numpy(ins['t1']).cuda()
  b = torch.empty_like(a)
  res = torch.full((4,), -1, dtype=torch.int64, device='cuda')
  torch.cuda.synchronize()
  prog.run_device([b.data_ptr()], [a.data_ptr()], extent, 5,
                  stream=S.cuda_stream, residual=res.data_ptr())
  S.synchronize()
  eager = res.cpu().numpy().view(np.uint64).copy()
  _, grown = prog.scratch()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=S):
    prog.run_device([b.data_ptr()], [a.data_ptr()], extent, 5,
                    stream=S.cuda_stream, residual=res.data_ptr())
  assert prog.scratch()[1] == grown
  for _ in range(2):
    res.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    again = res.cpu().numpy().view(np.uint64)
    assert np.array_equal(again, eager)
  assert (int(eager[0]), int(eager[1]),
          float(eager[2:3].view(np.float64)[0]), int(eager[3])) == want
  del g


@pytest.mark.gpu
def test_run_until(built):
  """jacobi2d border='preserve' at 64 x 40, tol 2^-8, a look every 8
  iterations: stops at the first multiple of 8 at which the oracle's residual
  is <= tol, with the oracle's outputs at that iteration bit for bit."""
  from soda_amd import runtime
  stencil = _stencil('jacobi2d.soda', iterate=8, border='preserve')
  extent = (64, 40)
  ins = {'t1': np.random.default_rng(7).random((40, 64), dtype=np.float32)}
  keep = ins['t1'].copy()
  tol = 2.0 ** -8
  stop, want, cur = None, None, None
  for n in range(8, 201, 8):
    want, cur = _expected(stencil, ins, extent, n)
    if want[1] == 0 and want[2] <= tol:
      stop = n
      break
  assert stop is not None and 16 <= stop <= 32, stop
  with runtime.Program(stencil, _opts(fuse=(8, 4), peel=1),
                       calibrate=False) as prog:
    outs, done, res = prog.run_until(ins, tol, 200, check_every=8)
    assert done == stop
    assert _fields(res) == want
    assert values.same_bits(outs['t0'], cur['t0']).all()
    assert np.array_equal(ins['t1'], keep)
    # ... an odd number of chunks and an even one both end in `outputs`
    for limit in (8, 16):
      want8, cur8 = _expected(stencil, ins, extent, limit)
      outs, done, res = prog.run_until(ins, tol, limit, check_every=8)
      assert done == limit and res.max_float > tol       # unconverged
      assert _fields(res) == want8
      assert values.same_bits(outs['t0'], cur8['t0']).all()
    # a last chunk shorter than the others
    want20, cur20 = _expected(stencil, ins, extent, 20)
    outs, done, res = prog.run_until(ins, 0.0, 20, check_every=8)
    assert done == 20 and _fields(res) == want20
    assert values.same_bits(outs['t0'], cur20['t0']).all()
    zeros = {'t1': np.zeros((40, 64), np.float32)}
    outs, done, res = prog.run_until(zeros, tol, 200, check_every=8)
    assert done == 8 and _fields(res) == (0, 0, 0.0, 0)
    assert not outs['t0'].any()


@pytest.mark.gpu
def test_run_until_shrinking_box(built):
  """border: ignore -- the cells counted are the valid box after ALL the
  iterations done so far, not that of the last chunk."""
  from soda_amd import runtime
  stencil = _stencil('jacobi2d.soda', iterate=8)
  extent = (64, 40)
  ins = _inputs(stencil, extent)
  with runtime.Program(stencil, _opts(fuse=(4,), peel=1),
                       calibrate=False) as prog:
    want, cur = _expected(stencil, ins, extent, 12)
    outs, done, res = prog.run_until(ins, 0.0, 12, check_every=4)
    assert done == 12 and _fields(res) == want
    lo, hi = stencil.valid_box(extent, None, 12)
    box = tuple(slice(l, h) for l, h in zip(lo, hi))[::-1]
    assert values.same_bits(outs['t0'][box], cur['t0'][box]).all()


@pytest.mark.gpu
def test_a_plain_program_is_refused(built):
  """The residual entries on a program built without the option:
  SODA_HIP_ERR_UNSUPPORTED, nothing launched, no byte written."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=2)
  extent = (256, 24)
  with _Device() as dev, runtime.Program(
      stencil, lower.LowerOptions(fuse=(2,), peel=0), calibrate=False) as prog:
    nbytes = 256 * 24 * 4
    a = dev.alloc(nbytes, fill=0)
    b = dev.alloc(nbytes, fill=0xA5)
    res = dev.alloc(32, fill=0xA5)
    prog.run_device([b], [a], extent)                # the handle itself is fine
    assert prog.last_launches()[0] == 1
    dev.rt.check(dev.lib.soda_hip_memset(ctypes.c_void_p(b), 0xA5, nbytes,
                                         None), 'memset')
    with pytest.raises(util.BackendError, match='(?i)unsupported|cannot serve'):
      prog.run_device([b], [a], extent, residual=res)
    assert prog.last_launches()[0] == 0
    assert prog.last_residual()[0] is None
    with pytest.raises(util.BackendError, match='residual'):
      prog.run_until({'t1': np.zeros((24, 256), np.float32)}, 0.0, 4)
    assert (dev.download(b, (nbytes,), np.uint8) == 0xA5).all()
    assert (dev.download(res, (32,), np.uint8) == 0xA5).all()
