"""soda_hip_run_device between guard bands (tests/guarded.py): no byte outside
the outputs.

Nearly every GPU parity test goes through `Program.run`, where the library
allocates the device arrays itself and copies back the valid box only.  Here
the caller's tensors lie in one arena, apart by guards, off the addresses an
allocator hands out; a case asserts

* the valid box is the C oracle's (single-threaded) bit for bit;
* no byte of the arena outside the output arrays changed -- the guards, and the
  inputs and param arrays through multi-pass ping-pong runs;
* the kernel family the case is about is the one that ran, and the deepest
  pass of the program is scheduled.

The guards next to an input hold NaN / -1 bytes and the oracle of every case
is finite on the compared box (asserted without a GPU, and again where the GPU
case runs): a NaN in a GPU result is a read of a guard and nothing else.

Shapes: two strips and nine lanes along x (2 S + 9 V of the deepest kernel),
three chunks and a ragged one along the marched dimension, a ragged last tile
along any other.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

from conftest import soda_path
import fuzz
import guarded
import values
import test_values as tv

SMOOTH1D = ('kernel: smooth1d\nburst width: 64\nunroll factor: 2\niterate: 3\n'
            'input float: a\n'
            'output float: b(0) = (a(-1) + a(0) * 2.0f + a(1)) * 0.25f\n')


def _x(s, v):
  return 2 * s + 9 * v


# name -> (program, stencil keywords, LowerOptions, grid(S, V of the deepest
# kernel), a tag of that kernel's name)
CASES = {
    # ---- marching 2-D: chunks of 16 rows, 16 + 16 + 16 + 5
    'jacobi2d_T13': ('jacobi2d.soda', dict(iterate=15),
                     dict(fuse=(13,), chunk_rows=16),
                     lambda s, v: (_x(s, v), 53), '_T13_'),
    'jacobi2d_pipe4': ('jacobi2d.soda', dict(iterate=9),
                       dict(fuse=(4,), pipe=4, chunk_rows=16),
                       lambda s, v: (_x(s, v), 53), '_pipe4'),
    'coupled2d': ('coupled2d.soda', dict(iterate=3),
                  dict(fuse=(2,), chunk_rows=16),
                  lambda s, v: (_x(s, v), 53), 'march2d_T2_'),
    'ints2d': ('ints2d.soda', {}, dict(chunk_rows=16),
               lambda s, v: (_x(s, v), 53), 'march2d_T1_'),
    # (three launches of the one-iteration kernel: the time model never
    # schedules winsum2d's three-iteration kernel, 24 warm-up rows a chunk)
    'winsum2d': ('winsum2d.soda', {}, dict(fuse=(), chunk_rows=16),
                 lambda s, v: (_x(s, v), 53), 'march2d_T1_'),
    'erosion': ('erosion.soda', {}, dict(chunk_rows=16),
                lambda s, v: (_x(s, v), 53), 'march2d_T1_'),
    'denoise2d': ('denoise2d.soda', {}, dict(chunk_rows=16),
                  lambda s, v: (_x(s, v), 53), 'march2d_T1_'),
    'conv2d': ('conv2d.soda', {}, dict(fuse=(2,), chunk_rows=16),
               lambda s, v: (_x(s, v), 53), 'march2d_T2_'),
    # ---- marching 3-D: tiles of 4 rows (4 + 4 + 1), chunks of 4 planes
    # (4 + 4 + 4 + 2)
    'heat3d': ('heat3d.soda', dict(iterate=3), dict(fuse=(2,), chunk_rows=4),
               lambda s, v: (_x(s, v), 9, 14), 'march3d_T2_'),
    # (rows a whole block covers: row_cells is the row length)
    'heat3d_xshare': ('heat3d.soda', dict(iterate=3),
                      dict(fuse=(2,), chunk_rows=4, xshare=True),
                      lambda s, v: (s + 9 * v, 9, 14), '_xs'),
    'heat3d_xb2': ('heat3d.soda', dict(iterate=3),
                   dict(fuse=(2,), chunk_rows=4, xshare_block=2),
                   lambda s, v: (_x(s, v), 9, 14), '_xb2'),
    # ---- tile3d: valid tiles of S x 10 cells (10 + 10 + 3), chunks of 4
    'heat3d_tile3d': ('heat3d.soda', dict(iterate=4),
                      dict(strategy='tile3d', fuse=(3,), chunk_rows=4),
                      lambda s, v: (_x(s, v), 23, 14), '_tile3d_T3_'),
    # ---- `border: preserve`: the whole array is defined and compared
    'jacobi2d_preserve_auto': ('jacobi2d.soda',
                               dict(iterate=3, border='preserve'),
                               dict(strategy='auto', fuse=(2,), chunk_rows=16),
                               lambda s, v: (_x(s, v), 53), 'march2d_T2_'),
    'jacobi2d_preserve_direct': ('jacobi2d.soda',
                                 dict(iterate=3, border='preserve'),
                                 dict(strategy='direct', fuse=(2,)),
                                 lambda s, v: (_x(s, v), 7), '_direct_'),
    'heat3d_preserve_auto': ('heat3d.soda', dict(iterate=2, border='preserve'),
                             dict(strategy='auto', fuse=(2,), chunk_rows=4),
                             lambda s, v: (_x(s, v), 9, 14), 'march3d_T2_'),
    'heat3d_preserve_direct': ('heat3d.soda',
                               dict(iterate=2, border='preserve'),
                               dict(strategy='direct', fuse=(2,)),
                               lambda s, v: (_x(s, v), 5, 6), '_direct_'),
}

# ---- direct: plain pointers, a whole fragment stored behind `x < extent[0]`.
# Each at the full vector width, at a row length that halves it down to two
# cells (extent[0] % 4 == 2) and at an odd one (one cell per thread).
DIRECT = {
    'blur': ('blur.soda', {}, lambda x: (x, 7)),            # uint16, a local
    'skew2d': ('skew2d.soda', {}, lambda x: (x, 8)),        # off-centre store
    'heat3d': ('heat3d.soda', dict(iterate=2), lambda x: (x, 5, 6)),
    'heat4d': ('heat4d.soda', dict(iterate=2), lambda x: (x, 5, 6, 5)),
    'smooth1d': (SMOOTH1D, {}, lambda x: (x,)),
}
for _name, (_soda, _skw, _grid) in DIRECT.items():
  for _vec in ('full', 2, 1):
    CASES['direct_%s_v%s' % (_name, _vec)] = (
        _soda, _skw, dict(strategy='direct', _vec=_vec),
        (lambda g: lambda s, v: g(_x(s, v)))(_grid), '_direct_')

# (program of tests/test_values.py, inputs).  WIDE_FLOAT takes the root of
# a(10, 3) + 1: on `signed` cells, a quarter of which lie below -1, NO seed
# gives a finite oracle.  That case runs as the others do, bit for bit with
# the NaNs where the oracle has them -- shown below to be exactly the cells
# with a negative radicand -- and once more on the same cells without their
# signs, where the oracle is finite and a NaN is a read of a guard.
LDSWIN = (('wideint', 'full'), ('widefloat', 'signed'), ('widefloat', 'positive'))
SEED = 77


def _kind(stencil):
  return 'signed' if any(t.is_float for t in stencil.input_types) else 'full'


@functools.lru_cache(maxsize=None)
def _stencil(name):
  from soda_amd import core
  soda, skw = CASES[name][:2]
  if '\n' in soda:
    return core.from_text(soda, **skw)
  return core.from_file(soda_path(soda), **skw)


def _lowered(stencil, kw, extent, probe):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, lower.LowerOptions(**kw), extent,
                                 probe=probe)
  return lower.lower(stencil, opts)


@functools.lru_cache(maxsize=None)
def _setup(name, probe=False):
  """(stencil, LowerOptions keywords, extent, extent to build the program for
  or None) of a named case.  The grid is that of the deepest kernel of the
  module built WITHOUT an extent -- the default vector width, strips that do
  not know the row length -- wherever such a program runs the grid; where the
  row length reduces the vector width the program is built for the grid, and
  the grid is that of ITS deepest kernel (the width follows the row length,
  the row length the width: to the fixed point)."""
  stencil = _stencil(name)
  kw = dict(CASES[name][2])
  grid = CASES[name][3]
  want_vec = kw.pop('_vec', None)
  if name == 'heat3d_xshare':
    # rows a whole block covers, sized from the plain kernel
    k = tv._deepest(_lowered(stencil, dict(kw, xshare=False), None, probe))
    kw['row_cells'] = grid(k.tile[0], k.tune['vec'])[0]
  first = dict(kw, vec=want_vec) if want_vec in (1, 2) else kw
  mod = _lowered(stencil, first, None, probe)
  k = tv._deepest(mod)
  extent = grid(k.tile[0], (k.tune or {}).get('vec', 1))
  if name == 'heat3d_xshare':
    extent = (kw['row_cells'],) + tuple(extent[1:])
  widest = max((q.tune or {}).get('vec', 1) for q in mod.kernels)
  if want_vec not in (1, 2) and extent[0] % widest == 0:
    return stencil, kw, tuple(extent), None
  for _ in range(4):
    k = tv._deepest(_lowered(stencil, kw, extent, probe))
    new = grid(k.tile[0], (k.tune or {}).get('vec', 1))
    if new == extent:
      break
    extent = new
  else:
    raise AssertionError('%s: no stable grid' % name)
  if want_vec in (1, 2):
    assert (k.tune or {}).get('vec', 1) == want_vec, (name, k.tune)
    assert extent[0] % 4 == 2 if want_vec == 2 else extent[0] % 2 == 1
  return stencil, kw, tuple(extent), tuple(extent)


def _finite(stencil, extent, want, iterate=None, whole=False):
  return all(np.isfinite(want[o][idx]).all()
             for o, idx in tv._boxes(stencil, extent, iterate, whole)
             if want[o].dtype.kind == 'f')


@functools.lru_cache(maxsize=None)
def _reference(stencil, extent, seed, iterate=None):
  """(inputs, C oracle outputs): computed once, shared, read-only."""
  ins = tv._readonly(values.edge_inputs(stencil, extent, seed, _kind(stencil)))
  return ins, tv._readonly(tv._oracle(stencil).run(ins, iterate=iterate))


# ---- random programs: the first usable seeds of tests/test_values.py whose
# oracle is finite on the compared box; NOT_FINITE lists the seeds of its full
# sets (--fuzz-budget 2.5) that are passed over for that reason, found by
# running the oracle on every one of them and checked below.
NOT_FINITE = {'plain': (9, 26, 43), 'preserve': (9, 26, 43), 'window': ()}
RANDOM_COUNT = {'plain': 12, 'preserve': 8, 'window': 4}


def _random_seeds(gen):
  usable = [s for s in tv.GENERATORS[gen] if s not in NOT_FINITE[gen]]
  n = max(4, int(round(RANDOM_COUNT[gen] * fuzz.budget())))
  return usable[:n]


RANDOM = [(g, s) for g in ('plain', 'preserve', 'window')
          for s in _random_seeds(g)]


def _random_reference(gen, seed):
  text, stencil, extent = tv._case(gen, seed)
  return (stencil, extent) + _reference(stencil, extent, seed)


@functools.lru_cache(maxsize=None)
def _ldswin_setup(name, kind):
  """(stencil, extent, inputs, C oracle outputs)."""
  text, stencil, seed = tv._ldswin_case(name)
  k, = tv._ldswin_module(stencil).kernels
  extent = tuple(tv._ldswin_shape(k)[0])
  if kind != 'positive':
    return (stencil, extent) + _reference(stencil, extent, seed)
  ins = {n: np.abs(a) for n, a in _reference(stencil, extent, seed)[0].items()}
  return stencil, extent, tv._readonly(ins), \
      tv._readonly(tv._oracle(stencil).run(ins))


# ---------------------------------------------------------------------------
# CPU: the helper
# ---------------------------------------------------------------------------

LAYOUT_CASES = ['jacobi2d_T13', 'coupled2d', 'ints2d', 'conv2d', 'heat3d',
                'direct_blur_v1', 'direct_heat4d_v2', 'direct_smooth1d_v1']


@pytest.mark.parametrize('name', LAYOUT_CASES)
def test_layout_invariants(built, name):
  stencil, kw, extent, _ = _setup(name)
  lay = guarded.layout(stencil, extent)
  roles = [t.role for t in lay.tensors]
  n_in, n_prm = len(stencil.input_names), len(stencil.param_stmts)
  assert roles == ['input'] * n_in + ['param'] * n_prm + \
      ['output'] * len(stencil.output_names)
  assert len(lay.guards) == len(lay.tensors) + 1
  end = 0
  for k, (g, t) in enumerate(zip(lay.guards, lay.tensors)):
    # guard k, then tensor k: back to back, nothing overlaps
    assert g.start == end and g.start + g.nbytes == t.start
    assert t.start % 16 == 0 and t.start % 64 != 0, (t.name, t.start)
    assert t.nbytes == int(np.prod(t.shape)) * t.dtype.itemsize
    assert t.shape == (extent[::-1] if t.role != 'param' else t.shape)
    # the guard's size: of BOTH neighbours, without the lead
    lead = guarded.DEFAULT_LEADS[k % 4]
    assert lead % 16 == 0 and lead % 64 != 0
    for n in lay.tensors[max(k - 1, 0):k + 1]:
      row = n.shape[-1] * n.dtype.itemsize
      need = max(4096, 2 * row)
      if stencil.dim >= 3 and n.role != 'param':
        need = max(4096, n.shape[-2] * row + row)
      assert g.nbytes - lead >= need, (k, n.name, g.nbytes, need)
    touches_read = t.role != 'output' or (k and roles[k - 1] != 'output')
    assert g.fill == (0xFF if touches_read else 0xA5), (k, g.fill)
    end = t.start + t.nbytes
  last = lay.guards[-1]
  assert last.start == end and last.start + last.nbytes == lay.nbytes
  t = lay.tensors[-1]
  row = t.shape[-1] * t.dtype.itemsize
  assert last.nbytes >= max(4096, 2 * row if stencil.dim < 3 else
                            t.shape[-2] * row + row)
  assert last.fill == 0xA5 and lay.nbytes % 16 == 0
  # the image: data in the inputs and params, the fills everywhere else
  ins = values.edge_inputs(stencil, extent, SEED, _kind(stencil))
  img = guarded.image(lay, ins)
  for t in lay.tensors:
    if t.role == 'output':
      assert (img[t.start:t.start + t.nbytes] == 0xA5).all()
    else:
      assert values.same_bits(guarded.read(lay, img, t.name),
                              np.asarray(ins[t.name]).reshape(t.shape)).all()
  for g in lay.guards:
    assert (img[g.start:g.start + g.nbytes] == g.fill).all()
  # ... where 0xFF is a NaN or the type's -1 / maximum
  for dt in (np.float32, np.float64):
    assert np.isnan(np.frombuffer(b'\xff' * 8, dt)).all()
  assert np.frombuffer(b'\xff' * 2, np.int16)[0] == -1
  assert np.frombuffer(b'\xff' * 2, np.uint16)[0] == 65535
  assert guarded.check(img, img.copy(), lay) is None


def test_check_names_every_planted_violation(built):
  stencil, kw, extent, _ = _setup('conv2d')      # an input, two params
  lay = guarded.layout(stencil, extent)
  ins = values.edge_inputs(stencil, extent, SEED, 'signed')
  before = guarded.image(lay, ins)
  by_name = {t.name: t for t in lay.tensors}
  img, w, out = by_name['img'], by_name['w'], by_name['out']
  row = out.row_bytes

  def planted(at, n=1):
    after = before.copy()
    after[at:at + n] ^= 0x40
    return guarded.check(before, after, lay)

  # writes INSIDE the output are its own business
  assert planted(out.start) is None and planted(out.start + out.nbytes - 1) is None
  assert planted(out.start - 1) == ('before', 'out', -1, -1, extent[0] - 1, 1)
  assert planted(out.start + out.nbytes) == \
      ('behind', 'out', out.nbytes, extent[1], 0, 1)
  # one stray fragment right behind the last cell
  assert planted(out.start + out.nbytes, 16) == \
      ('behind', 'out', out.nbytes, extent[1], 0, 16)
  # a whole row before the first cell
  assert planted(out.start - row, 4)[:5] == ('before', 'out', -row, -1, 0)
  cell = (3 * extent[0] + 5) * 4 + 2
  assert planted(img.start + cell) == ('input', 'img', cell, 3, 5, 1)
  assert planted(w.start + 4 * 4 + 1) == ('param', 'w', 17, 0, 4, 1)
  assert planted(0)[:2] == ('before', 'img')
  assert planted(lay.nbytes - 1)[:2] == ('behind', 'out')
  # the first one is named, all are counted
  after = before.copy()
  after[img.start + 40] ^= 1
  after[out.start - 3] ^= 1
  after[out.start + 8] ^= 1
  assert guarded.check(before, after, lay) == ('input', 'img', 40, 0, 10, 2)
  # a guard between two outputs names the nearer one
  st2, _, ext2, _ = _setup('coupled2d')
  lay2 = guarded.layout(st2, ext2)
  b2 = guarded.image(lay2, values.edge_inputs(st2, ext2, SEED, 'signed'))
  a2, o2 = {t.name: t for t in lay2.tensors}['a2'], lay2.tensors[-1]
  after = b2.copy()
  after[a2.start + a2.nbytes + 2] = 0
  assert guarded.check(b2, after, lay2)[:3] == ('behind', 'a2', a2.nbytes + 2)
  after = b2.copy()
  after[o2.start - 16:o2.start] = 0
  assert guarded.check(b2, after, lay2)[:3] == ('before', 'b2', -16)


# ---------------------------------------------------------------------------
# CPU: the oracle of every GPU case is finite on the compared box
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(CASES))
def test_oracle_is_finite_on_named_cases(built, name):
  stencil, kw, extent, _ = _setup(name)
  whole = bool(stencil.preserve_border)
  lo, hi = stencil.valid_box(extent)
  assert all(h > l for l, h in zip(lo, hi)), (extent, lo, hi)
  ins, want = _reference(stencil, extent, SEED)
  assert all(np.isfinite(a).all() for a in ins.values() if a.dtype.kind == 'f')
  assert _finite(stencil, extent, want, whole=whole)


@pytest.mark.parametrize('name,kind', LDSWIN)
def test_oracle_is_finite_on_ldswin_cases(built, name, kind):
  stencil, extent, ins, want = _ldswin_setup(name, kind)
  if (name, kind) != ('widefloat', 'signed'):
    assert _finite(stencil, extent, want)
    return
  # b(1, -1) = ... + sqrt(a(10, 3) + 1.0f) + ...: cell (x, y) of b takes the
  # root of a(x + 9, y + 4) + 1; everything else in it is finite on cells of
  # [-2, 2].  The oracle is NaN exactly where that radicand is negative.
  (o, idx), = tv._boxes(stencil, extent)
  a = ins['a']
  radicand = a[idx[0].start + 4:idx[0].stop + 4,
               idx[1].start + 9:idx[1].stop + 9] + np.float32(1.0)
  box = want[o][idx]
  assert radicand.shape == box.shape
  assert np.array_equal(np.isnan(box), radicand < 0)
  assert np.isfinite(box[radicand >= 0]).all()
  assert 0.15 < np.isnan(box).mean() < 0.35


@pytest.mark.parametrize('gen,seed', RANDOM)
def test_oracle_is_finite_on_random_cases(built, gen, seed):
  stencil, extent, ins, want = _random_reference(gen, seed)
  assert _finite(stencil, extent, want, whole=gen == 'preserve')


def test_seeds_passed_over_are_not_finite(built):
  """Every seed NOT_FINITE names is usable, and its oracle is not finite:
  nothing is left out for another reason."""
  for gen, seeds in NOT_FINITE.items():
    assert len(_random_seeds(gen)) >= 4
    for seed in seeds:
      if tv._case(gen, seed) is None:
        raise AssertionError('%s seed %d is not usable anyway' % (gen, seed))
      stencil, extent, ins, want = _random_reference(gen, seed)
      assert not _finite(stencil, extent, want, whole=gen == 'preserve'), \
          (gen, seed)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _program(stencil, extent, **kw):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  return runtime.Program(stencil, lower.LowerOptions(**kw), extent=extent,
                         calibrate=False)


def _guarded_case(prog, stencil, extent, ins, want, what, iterate=None,
                  whole=False, leads=None, finite=True, **run_kw):
  assert not finite or _finite(stencil, extent, want, iterate, whole), what
  got, bad, images = guarded.run(prog, stencil, extent, ins, iterate,
                                 leads=leads, **run_kw)
  assert bad is None, '%s on %s: a byte outside the outputs changed: %s' % (
      what, tuple(extent), (bad,))
  tv._assert_same(stencil, extent, got, want, what, iterate, whole)
  return got, images


def _deepest_is_scheduled(prog, extent, iterate):
  """The programs here are built with calibrate=False: which kernels a case
  runs is then the time model's choice, the same in every session.  Where the
  model leaves the deepest pass out, the clock is asked, as the library itself
  asks it on the first run of an extent by default (Program.calibrate: measured
  launch times outrank the model); the pass must be scheduled then, and the
  run that follows takes that schedule."""
  deepest = max(p.fused_iters for p in prog.module.passes)
  if deepest == 1:
    return
  modelled = prog.pass_times(extent)[0]
  if not prog.schedule(extent, iterate).get(deepest):
    measured = prog.calibrate(extent)
    print('deepest %d: modelled us %s, measured us %s, schedule %s' % (
        deepest, modelled, measured, prog.schedule(extent, iterate)))
  assert prog.schedule(extent, iterate).get(deepest), \
      (prog.schedule(extent, iterate), modelled, prog.pass_times(extent))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_gpu_named_cases_between_guards(built, name):
  stencil, kw, extent, build_for = _setup(name, probe=True)
  whole = bool(stencil.preserve_border)
  tag = CASES[name][4]
  ins, want = _reference(stencil, extent, SEED)
  with _program(stencil, build_for, **kw) as prog:
    k = tv._deepest(prog.module)
    names = [q.name for q in prog.module.kernels]
    assert tag in k.name, names
    s, v = k.tile[0], (k.tune or {}).get('vec', 1)
    if name == 'heat3d_xshare':
      assert extent[0] == kw['row_cells']
    else:
      assert CASES[name][3](s, v) == extent, (s, v, extent)
    if kw.get('strategy') == 'direct':
      assert all('_direct_' in n for n in names), names
      want_vec = CASES[name][2].get('_vec')
      if want_vec in (1, 2):
        assert v == want_vec and extent[0] % (2 * want_vec)
    else:
      # three chunks and a ragged one; a ragged last tile beside them
      tile = prog.geometry(extent)[0][k.name]
      ax = stencil.dim - 1
      assert tile[ax] == kw['chunk_rows']
      assert extent[ax] > 3 * tile[ax] and extent[ax] % tile[ax], tile
      assert extent[0] > tile[0] or name == 'heat3d_xshare'
      for d in range(1, ax):
        assert extent[d] > tile[d] and extent[d] % tile[d], tile
    _deepest_is_scheduled(prog, extent, stencil.iterate)
    _guarded_case(prog, stencil, extent, ins, want, '%s (%s)' % (name, names),
                  whole=whole)


@pytest.mark.gpu
@pytest.mark.parametrize('name,kind', LDSWIN)
def test_gpu_ldswin_between_guards(built, name, kind):
  """Two quads per lane stored whole inside the box, cell by cell at its
  edges: one full tile and a ragged one each way."""
  stencil, extent, ins, want = _ldswin_setup(name, kind)
  with _program(stencil, extent, strategy='ldswin') as prog:
    k, = prog.module.kernels
    assert 'ldswin' in k.name
    assert tuple(tv._ldswin_shape(k)[0]) == extent
    assert prog.geometry(extent)[0][k.name][:2] == k.tile[:2]
    _guarded_case(prog, stencil, extent, ins, want,
                  '%s, %s (%s)' % (name, kind, k.name),
                  finite=(name, kind) != ('widefloat', 'signed'))


@pytest.mark.gpu
@pytest.mark.parametrize('gen,seed', RANDOM)
def test_gpu_random_programs_between_guards(built, gen, seed):
  """Through the family `auto` picks and through `direct`, on the grids of
  tests/test_values.py.

  (plain seed 2 is the case the clock decides: on its 64 x 17 x 13 grid the
  model prices the two-iteration kernel at 36.5 us and the one-iteration
  kernel at 12.8 us, schedule {1: 2}; measured, three calibrations: 8.8 us
  and 6.1 us a launch, schedule {2: 1}, which is what then runs between the
  guards.)"""
  stencil, extent, ins, want = _random_reference(gen, seed)
  text = tv._case(gen, seed)[0]
  for kw in tv.AUTO_AND_DIRECT:
    with _program(stencil, extent, **kw) as prog:
      names = [k.name for k in prog.module.kernels]
      if kw['strategy'] == 'direct':
        assert all('_direct_' in n for n in names), names
      _deepest_is_scheduled(prog, extent, stencil.iterate)
      _guarded_case(prog, stencil, extent, ins, want,
                    '%s seed %d, %s (%s)\n%s' % (gen, seed, kw, names, text),
                    whole=gen == 'preserve')
      deepest = max(p.fused_iters for p in prog.module.passes)
      # ... and that pass did run: launches of the first (deepest) pass
      assert deepest == 1 or prog.last_launches()[1] > 0, prog.last_launches()


# ---- one handle, several extents --------------------------------------------

SEVERAL = {
    # name -> (case whose program it is, extents A, B < A, C > A)
    'jacobi2d': ('jacobi2d.soda', dict(iterate=9), dict(fuse=(4,)),
                 ((520, 61), (264, 40), (776, 75))),
    'heat3d': ('heat3d.soda', dict(iterate=3), dict(fuse=(2,)),
               ((264, 9, 14), (132, 6, 9), (520, 11, 17))),
    'blur': ('blur.soda', {}, dict(strategy='direct'),
             ((2056, 7), (1032, 5), (4104, 9))),
}
SEVERAL_ITERATE = {'jacobi2d': (9, 6, 9, 7), 'heat3d': (3, 2, 3, 4),
                   'blur': (1, 1, 1, 1)}


@functools.lru_cache(maxsize=None)
def _several_stencil(name):
  from soda_amd import core
  soda, skw = SEVERAL[name][:2]
  return core.from_file(soda_path(soda), **skw)


def _several_runs(name):
  a, b, c = SEVERAL[name][3]
  return list(zip((a, b, a, c), SEVERAL_ITERATE[name]))


@pytest.mark.parametrize('name', sorted(SEVERAL))
def test_oracle_is_finite_on_several_extents(built, name):
  stencil = _several_stencil(name)
  for extent, iterate in _several_runs(name):
    ins, want = _reference(stencil, extent, SEED, iterate)
    assert _finite(stencil, extent, want, iterate), (extent, iterate)
  assert {i % 2 for i in SEVERAL_ITERATE[name]} == \
      ({0, 1} if stencil.iterate > 1 else {1})


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(SEVERAL))
def test_gpu_one_handle_several_extents(built, name):
  """A, a smaller B, A again and a larger C on ONE program built without an
  extent, iterate counts of both parities: the ping-pong temporaries and the
  locals' scratch are reused, outgrown and regrown.  Each run is the oracle's;
  the second A is the first bit for bit."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _several_stencil(name)
  seen = {}
  with runtime.Program(stencil, lower.LowerOptions(**SEVERAL[name][2]),
                       calibrate=False) as prog:
    for extent, iterate in _several_runs(name):
      ins, want = _reference(stencil, extent, SEED, iterate)
      got, _ = _guarded_case(prog, stencil, extent, ins, want,
                             '%s on %s x %d' % (name, extent, iterate), iterate)
      if (extent, iterate) in seen:
        for (o, idx) in tv._boxes(stencil, extent, iterate):
          assert values.same_bits(got[o][idx], seen[extent, iterate][o][idx]).all()
      seen[extent, iterate] = got
  assert len(seen) == 3


# ---- keep= -------------------------------------------------------------------

KEEP = {
    'jacobi2d': ('jacobi2d.soda', (520, 400), 17, (4,), (150, 400)),
    'heat3d': ('heat3d.soda', (256, 24, 90), 10, (2,), (30, 60)),
}


@functools.lru_cache(maxsize=None)
def _keep_stencil(name):
  from soda_amd import core
  return core.from_file(soda_path(KEEP[name][0]), iterate=KEEP[name][2])


@pytest.mark.parametrize('name', sorted(KEEP))
def test_oracle_is_finite_on_keep_cases(built, name):
  stencil = _keep_stencil(name)
  ins, want = _reference(stencil, KEEP[name][1], SEED)
  assert _finite(stencil, KEEP[name][1], want)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(KEEP))
def test_gpu_keep_leaves_far_rows_alone(built, name):
  """soda_hip_run_device_cone between guards: the kept rows are the oracle's,
  no byte outside the outputs changes, and -- include/soda_hip.h -- rows
  further than (deepest fused_iters x reach) from [keep_lo, keep_hi) are left
  as they were: they still hold the 0xA5 fill."""
  soda, extent, iterate, fuse, keep = KEEP[name]
  stencil = _keep_stencil(name)
  ins, want = _reference(stencil, extent, SEED)
  assert _finite(stencil, extent, want)
  with _program(stencil, extent, fuse=fuse) as prog:
    deepest = max(p.fused_iters for p in prog.module.passes)
    assert deepest == fuse[0]
    _deepest_is_scheduled(prog, extent, iterate)
    got, bad, (before, after, lay) = guarded.run(prog, stencil, extent, ins,
                                                 iterate, keep=keep)
    launches = sum(prog.schedule(extent, iterate).values())
    assert launches >= 3 and prog.last_rows() < launches * extent[-1]
  assert bad is None, (bad,)
  out = stencil.output_names[0]
  lo, hi = stencil.valid_box(extent)
  box = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
  k0, k1 = max(keep[0], lo[-1]) - lo[-1], min(keep[1], hi[-1]) - lo[-1]
  assert k1 > k0
  same = values.same_bits(got[out][box][k0:k1], want[out][box][k0:k1])
  assert same.all(), '%d kept cells differ' % int((~same).sum())
  reach_lo, reach_hi = stencil.reach_along(stencil.dim - 1)
  far_lo = keep[0] - deepest * reach_lo
  far_hi = keep[1] + deepest * reach_hi
  raw = got[out].view(np.uint8).reshape(extent[-1], -1)
  for what, rows in (('below', raw[:max(far_lo, 0)]),
                     ('above', raw[min(far_hi, extent[-1]):])):
    touched = np.flatnonzero((rows != guarded.FILL_WRITE).any(axis=1))
    assert not touched.size, \
        'rows %s the cone were written: %d of them, first %d, last %d' % (
            what, touched.size, touched[0], touched[-1])
  assert far_lo > 0 or far_hi < extent[-1]


# ---- the two refusals -----------------------------------------------------------

def _refused(prog, arena, outputs, inputs, extent, iterate, text, **kw):
  from soda_amd import util
  with pytest.raises(util.BackendError) as err:
    prog.run_device(outputs, inputs, extent, iterate, **kw)
  assert text in str(err.value) and 'nothing was launched' in str(err.value), \
      str(err.value)
  after = arena.download()
  assert (after == arena.before).all(), 'a refused call wrote to the arena'


REFUSAL_ENTRIES = {'run_device': {}, 'keep': dict(keep=(10, 30))}


@pytest.mark.gpu
@pytest.mark.parametrize('entry', sorted(REFUSAL_ENTRIES))
def test_gpu_overlapping_tensors_are_refused(built, entry):
  """An output one row into its input, two outputs that overlap: refused with
  SODA_HIP_ERR_INVALID before anything is launched."""
  from soda_amd import core
  run_kw = REFUSAL_ENTRIES[entry]
  stencil = core.from_file(soda_path('coupled2d.soda'), iterate=3)
  extent = (264, 40)
  ins = values.edge_inputs(stencil, extent, SEED, 'signed')
  lay = guarded.layout(stencil, extent)
  row = extent[0] * 4
  with _program(stencil, extent, fuse=(2,)) as prog, \
      guarded.Arena(prog, lay, ins) as arena:
    a, b = arena.inputs()
    a2, b2 = arena.outputs()
    _refused(prog, arena, [a + row, b2], [a, b], extent, 3,
             'an output overlaps an input', **run_kw)
    _refused(prog, arena, [a2, b - row], [a, b], extent, 3,
             'an output overlaps an input', **run_kw)
    _refused(prog, arena, [a2, a2 + row], [a, b], extent, 3,
             'two outputs overlap', **run_kw)
    # the last byte of one is the first of the other
    size = extent[0] * extent[1] * 4
    _refused(prog, arena, [a2, a2 + size - 16], [a, b], extent, 3,
             'two outputs overlap', **run_kw)
    # ... and tensors that only touch are fine: checked without a launch by the
    # layout itself, whose guards are what separates them


@pytest.mark.gpu
@pytest.mark.parametrize('entry', sorted(REFUSAL_ENTRIES))
def test_gpu_misaligned_tensors_are_refused(built, entry):
  """A float tensor 4 bytes off with four cells per lane, a uint8 tensor one
  byte off with sixteen: refused, nothing launched.  No kernel ever runs on an
  address that breaks the rule; the same 4 bytes with ONE cell per lane (an
  odd row length) keep it, and that run is the oracle's between guards."""
  from soda_amd import core
  run_kw = REFUSAL_ENTRIES[entry]
  stencil = core.from_file(soda_path('jacobi2d.soda'), iterate=3)
  extent = (264, 40)
  ins = values.edge_inputs(stencil, extent, SEED, 'signed')
  lay = guarded.layout(stencil, extent)
  with _program(stencil, extent, fuse=(2,)) as prog, \
      guarded.Arena(prog, lay, ins) as arena:
    assert tv._deepest(prog.module).tune['vec'] == 4
    (i,), (o,) = arena.inputs(), arena.outputs()
    for outs, inps, which in (([o + 4], [i], 'output 0'),
                              ([o], [i + 4], 'input 0'),
                              ([o + 8], [i + 8], 'input 0')):
      _refused(prog, arena, outs, inps, extent, 3,
               '%s at' % which, **run_kw)
      _refused(prog, arena, outs, inps, extent, 3,
               'is not aligned to 16 bytes', **run_kw)
  bytes_ = core.from_text(
      'kernel: bytes\nburst width: 64\nunroll factor: 2\niterate: 2\n'
      'input uint8: a(32, *)\n'
      'output uint8: b(0, 0) = (a(-1, 0) + a(1, 0) + a(0, -1) + a(0, 1)) / 4\n')
  extent8 = (544, 40)
  ins8 = values.edge_inputs(bytes_, extent8, SEED, 'full')
  lay8 = guarded.layout(bytes_, extent8)
  for kw in (dict(fuse=(2,)), dict(strategy='direct')):
    with _program(bytes_, extent8, **kw) as prog, \
        guarded.Arena(prog, lay8, ins8) as arena:
      assert max((k.tune or {}).get('vec', 1)
                 for k in prog.module.kernels) == 16
      (i,), (o,) = arena.inputs(), arena.outputs()
      _refused(prog, arena, [o + 1], [i], extent8, 2,
               'is not aligned to 16 bytes', **run_kw)
      _refused(prog, arena, [o], [i + 1], extent8, 2,
               'is not aligned to 16 bytes', **run_kw)
  # one cell per lane: 4-byte alignment is all a float tensor needs
  odd = (263, 40)
  ins1, want1 = _reference(stencil, odd, SEED, 3)
  keep_kw = dict(run_kw)
  with _program(stencil, odd, fuse=(2,)) as prog:
    assert max((k.tune or {}).get('vec', 1) for k in prog.module.kernels) == 1
    got, bad, _ = guarded.run(prog, stencil, odd, ins1, 3, leads=(20, 52),
                              **keep_kw)
  assert bad is None, (bad,)
  if entry == 'keep':
    lo, hi = stencil.valid_box(odd)
    rows = slice(max(lo[1], 10), min(hi[1], 30))
    same = values.same_bits(got['t0'][rows, lo[0]:hi[0]],
                            want1['t0'][rows, lo[0]:hi[0]])
    assert same.all()
  else:
    tv._assert_same(stencil, odd, got, want1, 'vec 1 at +4 bytes', 3)
