"""Residual, exact norms and run_until on periodic and bordered domains
(DESIGN.md 4.14): the partition of a fused bordered domain, the scheme by the
numpy oracle, the interface, and on the GPU every struct against the oracle's
word for word.  Expected values: tests/domains.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, soda_path
import borders
import celltypes
import domains
import guarded
import norms
import periodic

DEPTH = 4


def _stencil(name, **kw):
  from soda_amd import core
  return core.from_file(soda_path(name), **kw)


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('peel', 0)
  return lower.LowerOptions(**kw)


def _plan(stencil, **kw):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, _opts(**kw), None, probe=False)
  return runtime.make_plan(lower.lower(stencil, opts))


# ---------------------------------------------------------------------------
# CPU: the partition
# ---------------------------------------------------------------------------

# name -> (file, LowerOptions keywords, modes, constants)
PLANS = {
    'jacobi2d': ('jacobi2d.soda', dict(fuse=(4,)), 'clamp', None),
    'jacobi2d_wrap_x': ('jacobi2d.soda', dict(fuse=(4,)), ('wrap', 'mirror'),
                        None),
    'jacobi2d_wrap_y': ('jacobi2d.soda', dict(fuse=(4,)), ('constant', 'wrap'),
                        -3.5),
    'skew2d': ('skew2d.soda', {}, ('constant', 'mirror101'), 2.0),  # one-sided
    'blur': ('blur.soda', {}, 'mirror101', None),                   # one-sided
    'coupled2d': ('coupled2d.soda', dict(fuse=(2,)), 'constant',
                  {'a': 1.5, 'b': -2.0}),
    'heat3d': ('heat3d.soda', dict(fuse=(2,)), 'clamp', None),
    'heat3d_wrap_z': ('heat3d.soda', dict(fuse=(2,)),
                      ('mirror', 'clamp', 'wrap'), None),
}


def _geometry(name, depth=DEPTH):
  from soda_amd import runtime
  fname, okw, modes, cst = PLANS[name]
  st = _stencil(fname, iterate=9)
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, modes, depth)
  return st, _plan(st, **okw), modes, cst, rlo, rhi, lo, hi


def _smallest(st, modes, rlo, rhi, depth=DEPTH, roomy=9):
  """N[d] = L + H in every wall dimension that has a strip."""
  raw = borders.per_dim(modes, st.dim)
  return tuple(2 * depth * (rlo[d] + rhi[d])
               if raw[d] != 'wrap' and rlo[d] + rhi[d] else roomy
               for d in range(st.dim))


@pytest.mark.parametrize('name', sorted(PLANS))
def test_the_boxes_partition_the_domain(built, name):
  """Painted on an integer array: every cell of the domain lies in exactly one
  box -- on a roomy extent, at N = L + H exactly, and one cell below, where
  the depth resolves to 1 and the one box is the domain."""
  from soda_amd import runtime
  st, plan, modes, _, rlo, rhi, lo, hi = _geometry(name)
  raw = borders.per_dim(modes, st.dim)
  small = _smallest(st, modes, rlo, rhi)
  for extent in (tuple(n + 7 + d for d, n in enumerate(small)), small):
    args = (plan, extent, modes, DEPTH, rlo, rhi, lo, hi)
    info, _ = runtime.border_fused_plan(*args)
    boxes = runtime.border_fused_residual_boxes(*args)
    assert boxes['depth'] == info['depth'] == DEPTH
    assert [s['dim'] for s in boxes['strips']] == [
        s['dim'] for s in info['strips']]
    assert (domains.paint(boxes, info, extent) == 1).all()
    # the numbers, restated: rims (T - 1) x reach wide whatever the chunk
    tlo, thi = boxes['trusted']
    for d in range(st.dim):
      wall = raw[d] != 'wrap'
      assert tlo[d] - info['ghost_lo'][d] == ((DEPTH - 1) * rlo[d] if wall
                                              else 0)
      assert thi[d] - info['ghost_lo'][d] == extent[d] - (
          (DEPTH - 1) * rhi[d] if wall else 0)
    for rim, strip in zip(boxes['strips'], info['strips']):
      d = strip['dim']
      assert rim['low'][1][d] - rim['low'][0][d] == (DEPTH - 1) * rlo[d]
      assert rim['high'][1][d] - rim['high'][0][d] == (DEPTH - 1) * rhi[d]
  walls = [d for d in range(st.dim) if raw[d] != 'wrap' and rlo[d] + rhi[d]]
  for d in walls:
    narrow = list(small)
    narrow[d] -= 1
    args = (plan, narrow, modes, DEPTH, rlo, rhi, lo, hi)
    info, _ = runtime.border_fused_plan(*args)
    boxes = runtime.border_fused_residual_boxes(*args)
    assert boxes['depth'] == 1 and boxes['strips'] == []
    assert boxes['trusted'] == (tuple(info['ghost_lo']), tuple(
        g + n for g, n in zip(info['ghost_lo'], narrow)))
    assert (domains.paint(boxes, info, narrow) == 1).all()


def test_a_one_sided_program_has_empty_rims(built):
  from soda_amd import runtime
  st, plan, modes, _, rlo, rhi, lo, hi = _geometry('blur')
  assert rlo == [0, 0] and rhi == [2, 2]
  extent = _smallest(st, modes, rlo, rhi)
  boxes = runtime.border_fused_residual_boxes(plan, extent, modes, DEPTH, rlo,
                                              rhi, lo, hi)
  for rim in boxes['strips']:
    d = rim['dim']
    assert rim['low'][0][d] == rim['low'][1][d]          # nothing at the low wall
    assert rim['high'][1][d] - rim['high'][0][d] == (DEPTH - 1) * 2


def test_the_partition_under_a_sanitizer(tmp_path):
  """tests/host/domain_boxes_main.cpp: hand-made 2-D and 3-D plans under every
  combination of modes, reaches, depths and extents around N = L + H, painted
  cell by cell.  Its own main, the library's sources, ASan + UBSan (`make
  domain_boxes_asan`); no GPU, nothing loaded into Python."""
  out = str(tmp_path)
  subprocess.run(['make', '-C', os.path.join(ROOT, 'soda_amd', 'csrc'),
                  'domain_boxes_asan', 'OUT=' + out], check=True,
                 capture_output=True)
  run = subprocess.run([os.path.join(out, 'domain_boxes_asan')],
                       capture_output=True, text=True, timeout=300)
  assert run.returncode == 0 and run.stdout.startswith('OK domain boxes'), (
      run.stdout + run.stderr)


def test_the_boxes_refuse_what_the_plan_refuses(built):
  from soda_amd import runtime, util
  st, plan, modes, _, rlo, rhi, lo, hi = _geometry('jacobi2d')
  for bad in (dict(depth=-1), dict(modes=(1, 9)), dict(lo=(0, 1)),
              dict(rlo=(2, 1))):
    kw = dict(depth=DEPTH, modes=modes, lo=lo, rlo=rlo)
    kw.update(bad)
    for fn in (runtime.border_fused_plan, runtime.border_fused_residual_boxes):
      with pytest.raises(util.BackendError, match='invalid'):
        fn(plan, (40, 30), kw['modes'], kw['depth'], kw['rlo'], rhi, kw['lo'],
           hi)
  with pytest.raises(util.BackendError, match='unsupported.*preserve'):
    runtime.border_fused_residual_boxes(plan, (40, 30), modes, DEPTH, rlo, rhi,
                                        lo, hi, preserve=True)


# ---------------------------------------------------------------------------
# CPU: the scheme emulated by the numpy oracle
# ---------------------------------------------------------------------------

SCHEME = [('jacobi2d', 'clamp', None), ('jacobi2d', 'mirror101', None),
          ('jacobi2d', 'constant', -3.5), ('skew2d', None, None),
          ('coupled2d', None, None), ('jacobi2d_wrap_x', None, None)]


@pytest.mark.parametrize('name,modes,cst', SCHEME, ids=[
    '%s-%s' % (n, m) for n, m, _ in SCHEME])
def test_the_scheme_by_the_oracle(built, name, modes, cst):
  """Deltas summed over exactly the returned boxes -- the interior's open-box
  states over the trusted box, every strip's bordered states over its rims --
  equal the residual and the norms of the whole domain, with 1, T - 1 and T
  iterations in the last chunk, at N = L + H."""
  from soda_amd import runtime
  st, plan, m0, c0, rlo, rhi, _, _ = _geometry(name)
  if modes is None:
    modes, cst = m0, c0
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, modes, DEPTH)
  extent = _smallest(st, modes, rlo, rhi, roomy=7)
  ins = periodic.inputs(st, extent, seed=2)
  lasts = (1, DEPTH - 1, DEPTH) if name == 'jacobi2d' else (DEPTH - 1,)
  for last in lasts:
    iterate = last if last == DEPTH else DEPTH + last
    args = (plan, extent, modes, DEPTH, rlo, rhi, lo, hi)
    info, chunks = runtime.border_fused_plan(*args, iterate)
    assert info['depth'] == DEPTH and chunks[-1] == last
    boxes = runtime.border_fused_residual_boxes(*args)
    got_res, got_norms = domains.emulate(st, ins, modes, cst, info, boxes,
                                         chunks)
    cur, prev = domains.states(st, ins, iterate, modes, cst)
    assert got_res == domains.residual_of(st, cur, prev), (name, last)
    assert got_norms == domains.norms_of(st, cur, prev), (name, last)
    assert got_res[0] > 0


def test_the_emulation_sees_a_rim_that_is_too_narrow(built):
  """No tautology: with one rim a cell short the counts differ."""
  from soda_amd import runtime
  st, plan, modes, cst, rlo, rhi, lo, hi = _geometry('jacobi2d')
  extent = _smallest(st, modes, rlo, rhi)
  ins = periodic.inputs(st, extent, seed=2)
  args = (plan, extent, modes, DEPTH, rlo, rhi, lo, hi)
  info, chunks = runtime.border_fused_plan(*args, DEPTH)
  boxes = runtime.border_fused_residual_boxes(*args)
  rim = boxes['strips'][0]
  (l, h) = rim['low']
  short = dict(rim, low=(l, (h[0] - 1,) + tuple(h[1:])))
  boxes = dict(boxes, strips=[short] + boxes['strips'][1:])
  got, _ = domains.emulate(st, ins, modes, cst, info, boxes, chunks)
  cur, prev = domains.states(st, ins, DEPTH, modes, cst)
  assert got[0] < domains.residual_of(st, cur, prev)[0]


# ---------------------------------------------------------------------------
# CPU: the interface
# ---------------------------------------------------------------------------

NEW = ['soda_hip_border_fused_residual_boxes'] + [
    'soda_hip_%s_%s' % (h, n)
    for h in ('periodic', 'border', 'border_fused')
    for n in ('run_padded_residual', 'run_padded_norms', 'run_until',
              'run_until_norm')]


def test_abi_and_names(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == runtime.ABI_VERSION == 9
  for name in NEW:
    assert name in runtime.API and hasattr(lib, name), name
  assert lib.soda_hip_sizeof(21) == ctypes.sizeof(runtime.BorderFusedBoxes)
  header = open(os.path.join(ROOT, 'include', 'soda_hip.h')).read()
  for name in NEW:
    assert name + '(' in header, name
  assert 'Not served on a torus: slabs' in header


def test_null_arguments_are_refused_without_a_gpu(built):
  from soda_amd import runtime
  lib = runtime.library()
  for name in NEW[1:]:
    argtypes = runtime.API[name][1]
    args = [0.0 if t is ctypes.c_double else 0 if t in (
        ctypes.c_int32, ctypes.c_uint64) else None for t in argtypes]
    assert getattr(lib, name)(*args) == 1, name          # SODA_HIP_ERR_INVALID
    assert 'NULL argument' in runtime.last_error()
  assert lib.soda_hip_border_fused_residual_boxes(None, None, None) == 1


class _Recorder:
  """Stands in for the library: records the entries a handle calls."""

  def __init__(self):
    self.calls = []

  def __getattr__(self, name):
    def fn(*args):
      self.calls.append((name, len(args)))
      return 0
    return fn


def test_run_padded_without_the_keywords_calls_the_old_entry():
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda', iterate=3)

  class Prog:
    stencil = st

    class _N:
      _handle = 7

    def norms(self):
      return self._N()
  for cls in (runtime.Periodic, runtime.Bordered, runtime.BorderedFused):
    h = object.__new__(cls)
    h.prog, h._lib, h._handle = Prog(), _Recorder(), None
    h.run_padded([1], [2], 3)
    h.run_padded([1], [2], 3, residual=64)
    h.run_padded([1], [2], 3, norms=64)
    assert h._lib.calls == [(cls._entry + 'run_padded', 5),
                            (cls._entry + 'run_padded_residual', 6),
                            (cls._entry + 'run_padded_norms', 7)]
    with pytest.raises(Exception, match='not both'):
      h.run_padded([1], [2], 3, residual=64, norms=64)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ct(t):
  return lambda: celltypes.stencil_of(t, 2, 'main', 9)


# program name -> (stencil, LowerOptions keywords)
PROGRAMS = {
    'jacobi2d': (lambda: _stencil('jacobi2d.soda', iterate=9),
                 dict(fuse=(4,), residual=True)),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=5),
               dict(fuse=(2,), residual=True)),
    'skew2d': (lambda: _stencil('skew2d.soda', iterate=5),
               dict(residual=True)),
    'double': (_ct('double'), dict(fuse=(4,), chunk_rows=16, residual=True)),
    'uint16': (_ct('uint16'), dict(fuse=(4,), chunk_rows=16, residual=True)),
    'plain': (lambda: _stencil('jacobi2d.soda', iterate=9), dict(fuse=(4,))),
}
_PROGRAMS = {}


@pytest.fixture(scope='module')
def programs(built):
  """Programs by name, made on first use, shared."""
  from soda_amd import runtime

  def get(name):
    if name not in _PROGRAMS:
      make, okw = PROGRAMS[name]
      _PROGRAMS[name] = runtime.Program(make(), _opts(**okw), calibrate=False)
    return _PROGRAMS[name]
  yield get
  for prog in _PROGRAMS.values():
    prog.close()
  _PROGRAMS.clear()


def _handle(prog, extent, modes, cst, depth):
  if modes is None:
    return prog.periodic(extent)
  return prog.bordered(extent, modes, cst, depth=depth)


def _parity(prog, pname, extent, modes, cst, depth, iterates, resolved=None,
            seed=0, ins=None):
  """Every struct of the handle equals the oracle's; the outputs of a residual
  and of a norms run equal the plain run's bits and the oracle's."""
  st = prog.stencil
  key = (pname, tuple(extent), seed) if ins is None else None
  if ins is None:
    ins = periodic.inputs(st, extent, seed)
  out = {}
  with _handle(prog, extent, modes, cst, depth) as h, \
      domains.Run(prog, h, ins, modes, cst) as run:
    if resolved is not None:
      assert run.info.get('depth', run.info['refill_every']) == resolved
    for n in iterates:
      cur, prev = domains.states(st, ins, n, modes, cst, key=key)
      plain = run.plain(n)
      got_r, res = run.residual(n)
      got_n, acc = run.norms(n)
      what = '%s %s %s depth %s n=%d' % (pname, extent, modes, depth, n)
      want = domains.residual_of(st, cur, prev)
      print(what, domains.fields(res), want)
      assert domains.fields(res) == want, what
      assert norms.same(acc, domains.norms_of(st, cur, prev)), what
      for o in st.output_names:
        assert periodic.same_bits(got_r[o], plain[o]), what
        assert periodic.same_bits(got_n[o], plain[o]), what
      inner = run.interior(plain)
      for o in st.output_names:
        assert periodic.same_bits(inner[o], cur[o]), what
      out[n] = (domains.fields(res), norms.fields(acc))
    for name, arr in run.inputs_now().items():       # never written
      assert periodic.same_bits(arr, run.start[name]), name
  return out


@pytest.mark.gpu
@pytest.mark.parametrize('extent', [(272, 37), (16, 16)], ids=str)
def test_torus(programs, extent):
  """(272, 37): a row crosses a wave-strip seam, the rows cross a chunk seam.
  The residual rides in the deepest fused twin."""
  prog = programs('jacobi2d')
  _parity(prog, 'jacobi2d', extent, None, None, None, (1, 4, 5, 9), resolved=4)
  assert prog.last_residual()[0] is not None


WALLS = ['clamp', 'mirror', 'mirror101', 'constant', ('wrap', 'clamp')]


@pytest.mark.gpu
@pytest.mark.parametrize('modes', WALLS, ids=str)
@pytest.mark.parametrize('extent', [(272, 37), (16, 16)], ids=str)
def test_walls_at_depth_1(programs, extent, modes):
  _parity(programs('jacobi2d'), 'jacobi2d', extent, modes, -3.5, 1,
          (1, 4, 5, 9), resolved=1)


@pytest.mark.gpu
@pytest.mark.parametrize('modes', WALLS, ids=str)
@pytest.mark.parametrize('extent,resolved', [((16, 16), 4), ((272, 37), 4),
                                             ((15, 16), 1)], ids=str)
def test_walls_fused(programs, extent, resolved, modes):
  """Depth 4: at the smallest extent that keeps it, across seams, and one cell
  below, where it resolves to 1.  The fused handle's structs equal the depth-1
  handle's."""
  prog = programs('jacobi2d')
  ns = (1, 3, 4, 5, 8)
  if modes[0] == 'wrap':            # no wall along dimension 0: 15 is no limit
    resolved = 4
  fused = _parity(prog, 'jacobi2d', extent, modes, -3.5, 4, ns,
                  resolved=resolved)
  flat = _parity(prog, 'jacobi2d', extent, modes, -3.5, 1, ns, resolved=1)
  assert fused == flat


@pytest.mark.gpu
@pytest.mark.parametrize('modes,depth,resolved', [
    (None, None, 2), ('clamp', 1, 1), ('clamp', 2, 2),
    (('mirror', 'clamp', 'wrap'), 2, 2)], ids=str)
def test_heat3d(programs, modes, depth, resolved):
  _parity(programs('heat3d'), 'heat3d', (40, 12, 12), modes, None, depth,
          (1, 2, 5), resolved=resolved)


@pytest.mark.gpu
def test_a_one_sided_program_fused(programs):
  prog = programs('skew2d')
  modes = ('constant', 'mirror101')
  fused = _parity(prog, 'skew2d', (40, 28), modes, 2.0, 2, (1, 2, 5),
                  resolved=2)
  assert fused == _parity(prog, 'skew2d', (40, 28), modes, 2.0, 1, (1, 2, 5))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['double', 'uint16'])
def test_other_cell_types(programs, name):
  prog = programs(name)
  for modes, depth, resolved in ((None, None, 4), ('mirror', 1, 1),
                                 (('constant', 'clamp'), 4, 4)):
    _parity(prog, name, (24, 21), modes, 7, depth, (1, 4, 6),
            resolved=resolved)


@pytest.mark.gpu
def test_forced_generic_is_the_same(programs, monkeypatch):
  prog = programs('jacobi2d')
  monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
  for modes, depth in ((None, None), ('clamp', 4)):
    _parity(prog, 'jacobi2d', (272, 37), modes, None, depth, (5,))
    assert prog.last_residual()[0] == 'generic'


@pytest.mark.gpu
@pytest.mark.parametrize('modes,depth', [(None, None), ('clamp', 1),
                                         ('clamp', 4), ('mirror', 4)], ids=str)
def test_non_finite_cells_next_to_a_wall(programs, modes, depth):
  """A NaN and an inf at the walls and in the corner -- the source cells of
  the frame: `unordered` and `infinite` count domain cells once, never a ghost
  copy of one."""
  prog = programs('jacobi2d')
  extent = (24, 20)
  ins = periodic.inputs(prog.stencil, extent, 3)
  a = ins['t1']
  a[0, 0], a[0, 7], a[19, 23] = np.nan, np.inf, -np.inf
  a[9, 0], a[12, 23] = np.inf, np.nan
  got = _parity(prog, 'jacobi2d', extent, modes, None, depth, (1, 2, 5),
                ins=ins)
  for n, (res, acc) in got.items():
    assert res[1] > 0 and acc['unordered'] == res[1], n
  assert got[1][1]['infinite'] > 0


# -- run_until ----------------------------------------------------------------

def _cpu_until(st, ins, modes, tol, max_iterate, check_every, norm):
  """(iterations done, cur, prev) of the CPU loop under the same stop rule."""
  done = 0
  while done < max_iterate:
    done += min(check_every, max_iterate - done)
    cur, prev = domains.states(st, ins, done, modes, None, key='until')
    if norm is None:
      res = domains.residual_of(st, cur, prev)
      stop = res[1] == 0 and res[2] <= tol and res[3] <= 0
    else:
      want = domains.norms_of(st, cur, prev)
      value = norms.expected_value(want, norm)
      if norm == 'l2':
        value = math.sqrt(value)
      stop = not want['unordered'] and not want['infinite'] and value <= tol
    if stop:
      break
  return done, cur, prev


@pytest.mark.gpu
@pytest.mark.parametrize('norm,tol,tight', [(None, 0.5, 0.01),
                                            ('l2', 4.0, 0.1)], ids=str)
@pytest.mark.parametrize('depth', [1, 4])
def test_run_until(programs, depth, norm, tol, tight):
  """A 32 x 24 clamped jacobi2d: iterations done, struct and output bits equal
  the CPU loop's, which stops strictly inside max_iterate (the oracle's
  residual is 0.26 and its L2 norm 2.26 after 8 iterations); one run under a
  tolerance it does not reach ends at max_iterate, in a shorter last chunk."""
  prog = programs('jacobi2d')
  st = prog.stencil
  extent = (32, 24)
  ins = periodic.inputs(st, extent, 1)
  keep = ins['t1'].copy()
  for tol, limit in ((tol, 60), (tight, 10)):
    done, cur, prev = _cpu_until(st, ins, 'clamp', tol, limit, 4, norm)
    assert (4 < done < 60) if limit == 60 else done == 10, done
    outs, got_done, last = prog.run_bordered_until(
        ins, 'clamp', tol, limit, depth=depth, check_every=4, norm=norm)
    print(depth, norm, limit, done, got_done)
    assert got_done == done
    if norm is None:
      assert domains.fields(last) == domains.residual_of(st, cur, prev)
    else:
      assert norms.same(last, domains.norms_of(st, cur, prev))
    assert periodic.same_bits(outs['t0'], cur['t0'])
    assert np.array_equal(ins['t1'], keep)


@pytest.mark.gpu
def test_run_until_on_a_torus(programs):
  prog = programs('jacobi2d')
  st = prog.stencil
  ins = periodic.inputs(st, (32, 24), 1)
  for norm, tol in ((None, 0.5), ('l1', 200.0)):
    done = 0
    while done < 60:
      done += 4
      cur, prev = domains.states(st, ins, done, None, None, key='torus')
      if norm is None:
        res = domains.residual_of(st, cur, prev)
        if res[2] <= tol:
          break
      elif norms.expected_value(domains.norms_of(st, cur, prev), 'l1') <= tol:
        break
    assert 4 < done < 60
    outs, got_done, last = prog.run_periodic_until(ins, tol, 60, check_every=4,
                                                   norm=norm)
    assert got_done == done
    if norm is None:
      assert domains.fields(last) == domains.residual_of(st, cur, prev)
    else:
      assert norms.same(last, domains.norms_of(st, cur, prev))
    assert periodic.same_bits(outs['t0'], cur['t0'])


# -- contracts ------------------------------------------------------------------

class _PaddedEntry:
  """The padded entry with run_device's call shape, for tests/guarded.py."""

  def __init__(self, prog, handle):
    self.device, self.handle = prog.device, handle

  def run_device(self, outputs, inputs, extent, iterate=None, **kw):
    self.handle.run_padded(outputs, inputs, iterate, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('modes,depth', [(None, None), ('mirror101', 1),
                                         ('mirror101', 4)], ids=str)
@pytest.mark.parametrize('which', ['residual', 'norms'])
def test_guard_bands(programs, modes, depth, which):
  """No byte outside the padded outputs and the struct is written; the inputs
  are unchanged."""
  prog = programs('jacobi2d')
  st = prog.stencil
  extent, n = (40, 30), 5
  ins = periodic.inputs(st, extent, 4)
  cur, prev = domains.states(st, ins, n, modes, None)
  size = 32 if which == 'residual' else 840
  with _handle(prog, extent, modes, None, depth) as h, \
      norms.Device(prog.device) as dev:
    info = h.info()
    start = domains.extended(st, ins, info, modes, None)
    band = 4096
    arena = dev.alloc(2 * band + size, fill=0xA5)
    outs, bad, _ = guarded.run(_PaddedEntry(prog, h), st, info['padded'],
                               start, n, **{which: arena + band})
    assert bad is None, bad
    img = dev.download(arena, (2 * band + size,), np.uint8)
    assert (img[:band] == 0xA5).all() and (img[band + size:] == 0xA5).all()
    if which == 'residual':
      assert domains.raw_fields(img[band:band + 32]) == \
          domains.residual_of(st, cur, prev)
    else:
      assert norms.same(prog.norms().fetch(arena + band),
                        domains.norms_of(st, cur, prev))
    got = np.ascontiguousarray(periodic.interior(outs['t0'], info))
    assert periodic.same_bits(got, cur['t0'])


@pytest.mark.gpu
@pytest.mark.parametrize('modes,depth', [(None, None), ('clamp', 4)], ids=str)
def test_captured_and_replayed(programs, modes, depth):
  """Captured after one eager call on the caller's stream, replayed twice: each
  replay zeroes and refills the struct."""
  import torch
  prog = programs('jacobi2d')
  st = prog.stencil
  extent, n = (40, 30), 7
  ins = periodic.inputs(st, extent, 4)
  cur, prev = domains.states(st, ins, n, modes, None)
  want = domains.residual_of(st, cur, prev)
  S = torch.cuda.Stream()
  with _handle(prog, extent, modes, None, depth) as h:
    info = h.info()
    start = domains.extended(st, ins, info, modes, None)['t1']
    a = torch.from_numpy(start).cuda()
    b = torch.empty_like(a)
    res = torch.full((4,), -1, dtype=torch.int64, device='cuda')
    call = lambda: h.run_padded([b.data_ptr()], [a.data_ptr()], n,
                                stream=S.cuda_stream, residual=res.data_ptr())
    torch.cuda.synchronize()
    call()
    S.synchronize()
    assert domains.raw_fields(res.cpu().numpy()) == want
    warm, held = prog.scratch(), info['scratch_bytes']
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
      call()
    for _ in range(2):
      res.fill_(-1)
      b.fill_(float('nan'))
      torch.cuda.synchronize()
      g.replay()
      torch.cuda.synchronize()
      assert domains.raw_fields(res.cpu().numpy()) == want
      got = np.ascontiguousarray(periodic.interior(b.cpu().numpy(), info))
      assert periodic.same_bits(got, cur['t0'])
    assert prog.scratch() == warm and h.info()['scratch_bytes'] == held
    del g


@pytest.mark.gpu
def test_refusals_leave_the_arena_untouched(programs):
  from soda_amd import util
  extent = (40, 30)
  for pname, modes, depth in (('plain', 'clamp', 4), ('plain', None, None),
                              ('jacobi2d', 'clamp', 4),
                              ('jacobi2d', 'clamp', 1)):
    prog = programs(pname)
    st = prog.stencil
    ins = periodic.inputs(st, extent, 4)
    with _handle(prog, extent, modes, None, depth) as h, \
        norms.Device(prog.device) as dev:
      info = h.info()
      start = domains.extended(st, ins, info, modes, None)['t1']
      a = dev.upload(start)
      b = dev.alloc(start.nbytes, fill=0xA5)
      res = dev.alloc(1024, fill=0xA5)
      held = info['scratch_bytes']
      if pname == 'plain':
        tries = [(dict(residual=res), 4, 'unsupported.*residual'),
                 (dict(norms=res), 4, 'unsupported.*residual')]
      else:
        tries = [(dict(residual=res), 0, 'invalid.*iterate < 1'),
                 (dict(residual=res + 4), 4, 'invalid.*aligned'),
                 (dict(residual=b + 64), 4, 'invalid.*overlaps an output'),
                 (dict(norms=b + 64), 4, 'invalid.*overlaps an output')]
      for kw, n, match in tries:
        with pytest.raises(util.BackendError, match='(?s)' + match):
          h.run_padded([b], [a], n, **kw)
      with pytest.raises(util.BackendError, match='invalid'):
        h.run_until([b], [a], 0.0, 0)
      if pname == 'plain':
        with pytest.raises(util.BackendError, match='unsupported'):
          h.run_until([b], [a], 0.0, 4)
      assert (dev.download(b, (start.nbytes,), np.uint8) == 0xA5).all()
      assert (dev.download(res, (1024,), np.uint8) == 0xA5).all()
      assert periodic.same_bits(dev.download(a, start.shape, start.dtype),
                                start)
      assert h.info()['scratch_bytes'] == held
