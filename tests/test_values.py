"""Parity on the whole value domain (tests/values.py): signed, extreme, tiny
and non-finite cells.

The rest of the suite varies SHAPES; its random programs see floats in
[0.25, 2) and integers in [0, 200].  Here the same programs, the corpus kernels
at their seams, the `ldswin` family, a batch and one small program per operator
group run on negative numbers, both zeros, subnormals, infinities, NaNs and
integers of the whole range (the arithmetic wraps: -fwrapv on both sides), and
are compared with `values.same_bits`, which tells -0.0 from +0.0.

CPU: the classes hold what they claim; the two oracles agree on every case
the GPU tests run; how many random-program cases the NaN-share condition
leaves out; the float mode of the JIT's kernel descriptors.  GPU: bit for bit
against c_oracle.COracle(openmp=False).

The NaN-share condition (not a tolerance): a (seed, class) case of a random
program is left out when more than a quarter of an output's valid box is NaN
in the C oracle -- it would compare almost nothing -- and at most one case in
ten may be left out per generator.  An operator table may be NaN in at most
half of its compared cells."""
import functools
import struct

import numpy as np
import pytest

from conftest import soda_path
import fuzz
import fuzz_nest
import values

NAN_SHARE_LEFT_OUT = 0.25
NAN_SHARE_TABLE = 0.5


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(gen, seed):
  """(text, stencil, extent) of a random program, or None where the generator
  produced an invalid program or one with an empty valid box."""
  from soda_amd import core, util
  border = None
  if gen == 'plain':
    text, dim, _ = fuzz.program(seed)
    extent = fuzz.extent_for(seed, dim)
  elif gen == 'rich':
    text, dim, _ = fuzz.program(seed, rich=True)
    extent = fuzz.extent_for(seed, dim)
  elif gen == 'preserve':
    text, dim, _ = fuzz.program(seed)
    extent = fuzz.extent_for(seed, dim)
    border = 'preserve'
  elif gen == 'window':
    text, dim, _ = fuzz.window_program(seed)
    extent = fuzz.window_extent_for(seed, dim)
  elif gen == 'wide':
    prog, extent = fuzz_nest.program(seed, 'wide')
    text = prog.soda_text()
  else:
    raise ValueError(gen)
  try:
    if border:
      stencil = core.from_text(text, border=border)
      stencil.check_preserve()
    else:
      stencil = core.from_text(text)
  except util.SodaError:
    return None
  lo, hi = stencil.valid_box(extent)
  if not all(h > l for l, h in zip(lo, hi)):
    return None
  return text, stencil, tuple(int(e) for e in extent)


def _usable(gen, seeds):
  return [s for s in seeds if _case(gen, s) is not None]


# The sets scale with --fuzz-budget like those of tests/test_fuzz.py; the full
# sets are the seeds both oracles were compared on, class by class, when the
# classes were chosen.
PLAIN_SEEDS = _usable('plain', fuzz.budget_seeds(24, 60))
RICH_SEEDS = _usable('rich', fuzz.budget_seeds(16, 40))
PRESERVE_SEEDS = _usable('preserve', fuzz.budget_seeds(24, 60))
# (109, 177, 283, 326, 454: the min / max windows tools/fuzz_scan.py found)
WINDOW_SEEDS = _usable('window', fuzz.budget_seeds(12, 24,
                                                   pinned=(109, 177, 283, 326,
                                                           454)))
# iterated, fusable, one cell to either side along x (tests/test_fuzz.py
# XSHARE_SEEDS) and accepted by xshare_block = 2 (tests/test_xshare_block.py):
# 2-D and 3-D, double / float / uint8 / int32 cells
XSHARE_SEEDS = (304, 594, 663, 1129, 434)
# 3-D programs of the plain generator `tile3d` accepts at four iterations
# (tests/test_tile3d.py FUZZ_SEEDS, those of at most three tensors)
TILE3D_SEEDS = (20, 136, 414, 434)
TILE3D_EXTENT, TILE3D_ITERATE = (96, 72, 40), 4
WIDE_SEEDS = _usable('wide', range(0, 6))

GENERATORS = {'plain': PLAIN_SEEDS, 'rich': RICH_SEEDS,
              'preserve': PRESERVE_SEEDS, 'window': WINDOW_SEEDS}


def _readonly(arrays):
  for a in arrays.values():
    a.setflags(write=False)
  return arrays


@functools.lru_cache(maxsize=None)
def _oracle(stencil):
  from oracle import c_oracle
  return c_oracle.COracle(stencil, openmp=False)


@functools.lru_cache(maxsize=None)
def _reference(gen, seed, kind):
  """(inputs, C oracle outputs) of a random-program case: computed once,
  shared, read-only."""
  text, stencil, extent = _case(gen, seed)
  ins = _readonly(values.edge_inputs(stencil, extent, seed, kind))
  return ins, _readonly(_oracle(stencil).run(ins))


def _boxes(stencil, extent, iterate=None, whole=False):
  for o in stencil.output_names:
    if whole:
      yield o, (slice(None),) * stencil.dim
      continue
    lo, hi = stencil.valid_box(extent, o, iterate)
    assert all(h > l for l, h in zip(lo, hi)), 'empty valid box: bad test'
    yield o, tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))


def _nan_share(stencil, extent, want, iterate=None, whole=False):
  return max(values.nan_share(want[o][idx])
             for o, idx in _boxes(stencil, extent, iterate, whole))


def _left_out(gen, seed, kind):
  text, stencil, extent = _case(gen, seed)
  want = _reference(gen, seed, kind)[1]
  return _nan_share(stencil, extent, want, whole=gen == 'preserve') > \
      NAN_SHARE_LEFT_OUT


def _classes(gen, seed):
  text, stencil, extent = _case(gen, seed)
  return values.classes_for(stencil, text)


def _assert_same(stencil, extent, got, want, what, iterate=None, whole=False):
  for o, idx in _boxes(stencil, extent, iterate, whole):
    g, w = got[o][idx], want[o][idx]
    same = values.same_bits(g, w)
    if not same.all():
      at = np.argwhere(~same)[0]
      raise AssertionError(
          '%s, output %s on %s: %d of %d cells differ, first at %s: got %r, '
          'want %r' % (what, o, tuple(extent), int((~same).sum()), same.size,
                       tuple(at[::-1]), g[tuple(at)], w[tuple(at)]))


def _seam_cells(stencil, extent, strip, chunk, iterate=None, strict=True):
  """Six cells (x, y[, z]) where a kernel hands data over: the last column of
  one strip and the first of the next (+inf next to -inf: they meet within one
  iteration); the last row / plane of one chunk and the first of the next; the
  first and the last cell of the valid box.  A strip or chunk longer than the
  grid puts its pair in the middle instead.  `strict=False`: None on a grid
  too small for six distinct cells."""
  dim = stencil.dim
  assert dim >= 2
  lo, hi = stencil.valid_box(extent, stencil.output_names[0], iterate)
  mid = [(l + h) // 2 for l, h in zip(lo, hi)]
  sx = strip if 1 < strip < extent[0] else extent[0] // 2
  cz = chunk if 1 < chunk < extent[-1] else extent[-1] // 2
  row = mid[-1] if mid[-1] not in (cz - 1, cz) else min(cz + 1, extent[-1] - 1)
  a, b = list(mid), list(mid)
  a[0], b[0], a[-1], b[-1] = sx - 1, sx, row, row
  c, d = list(mid), list(mid)
  c[0], d[0], c[-1], d[-1] = sx - 1, sx - 1, cz - 1, cz
  cells = [tuple(a), tuple(b), tuple(c), tuple(d), tuple(lo),
           tuple(h - 1 for h in hi)]
  ok = len(set(cells)) == 6 and all(0 <= v < e for cell in cells
                                    for v, e in zip(cell, extent))
  assert ok or not strict, cells
  return cells if ok else None


# ---------------------------------------------------------------------------
# CPU: the classes hold what they claim
# ---------------------------------------------------------------------------

def _typed(kinds):
  from soda_amd import core
  lines = ['kernel: typed', 'burst width: 64', 'unroll factor: 2', 'iterate: 1']
  for i, t in enumerate(kinds):
    lines.append('input %s: t%d%s' % (t, i, '(32, *)' if i == 0 else ''))
  lines.append('output %s: o(0, 0) = t0(0, 0) + t0(1, 0)' % kinds[0])
  return core.from_text('\n'.join(lines) + '\n')


@pytest.mark.parametrize('t', ['float', 'double'])
def test_float_classes_hold_what_they_claim(t):
  stencil = _typed([t, t])
  extent = (64, 20)                 # the smallest grid fuzz.extent_for gives
  dt = np.dtype(stencil.input_types[0].np_name)
  info = np.finfo(dt)
  for name in stencil.input_names:
    x = values.edge_inputs(stencil, extent, 3, 'signed')[name]
    assert x.dtype == dt and x.shape == extent[::-1]
    nz = x[x != 0]
    assert (np.abs(nz) >= 0.25).all() and (np.abs(nz) <= 2.0).all()
    assert (nz < 0).any() and (nz > 0).any()
    zeros = x[x == 0]
    assert (np.signbit(zeros)).any() and (~np.signbit(zeros)).any()
    assert np.isfinite(x).all()
    y = values.edge_inputs(stencil, extent, 3, 'tiny')[name]
    sub = (y != 0) & (np.abs(y) < info.smallest_normal)
    assert 0.2 < sub.mean() < 0.6, sub.mean()
    assert (np.abs(y[~sub & (y != 0)]) <= 2.0).all()
    if info.nmant < 29:      # k reaches past the mantissa: the first normals
      assert ((np.abs(y) >= info.smallest_normal) &
              (np.abs(y) < info.smallest_normal * 2.0 ** 12)).any()
    at = [(0, 0), (63, 19), (31, 7), (32, 7), (5, 15), (5, 16)]
    z = values.edge_inputs(stencil, extent, 3, 'nonfinite', at=at)[name]
    assert sorted(values.nonfinite_cells(z)) == sorted(at)
    for (cx, cy), v in zip(at, values.NONFINITE):
      assert values.same_bits(z[cy, cx], np.array(v, dt)), (cx, cy)
    placed = values.edge_inputs(stencil, extent, 3, 'nonfinite')[name]
    assert len(values.nonfinite_cells(placed)) == 6
    assert int(np.isnan(placed).sum()) == 2
    assert int((placed == np.inf).sum()) == int((placed == -np.inf).sum()) == 2


@pytest.mark.parametrize('t', fuzz.INT_TYPES + ['uint32'])
def test_full_holds_the_ends_of_the_range(t):
  stencil = _typed([t])
  for extent in ((64, 20), (300, 24)):
    x = values.edge_inputs(stencil, extent, 5, 'full')['t0']
    info = np.iinfo(x.dtype)
    assert x.dtype == np.dtype(stencil.input_types[0].np_name)
    for v in (info.min, info.max, 0, 1, -1 if info.min < 0 else info.max - 1):
      assert (x == v).any(), v
    # uniform over the whole range: every eighth of it is drawn from
    width = (int(info.max) - int(info.min) + 1) // 8
    hit = {(int(v) - int(info.min)) // width for v in x.reshape(-1)}
    assert hit == set(range(8)), hit
    # an integer tensor is `full` in every class
    y = values.edge_inputs(stencil, extent, 5, 'tiny')['t0']
    assert np.array_equal(x, y)


def test_the_draw_is_deterministic_in_the_seed():
  stencil = _typed(['float', 'double'])
  ints = _typed(['int16', 'uint8'])
  for st, kinds in ((stencil, values.FLOAT_CLASSES), (ints, values.INT_CLASSES)):
    for kind in kinds:
      a = values.edge_inputs(st, (100, 30), 11, kind)
      b = values.edge_inputs(st, (100, 30), 11, kind)
      c = values.edge_inputs(st, (100, 30), 12, kind)
      for n in st.input_names:
        assert values.same_bits(a[n], b[n]).all()
        assert not values.same_bits(a[n], c[n]).all()
  # one tensor's cells are not another's
  a = values.edge_inputs(_typed(['float', 'float']), (100, 30), 11, 'signed')
  assert not values.same_bits(a['t0'], a['t1']).all()


def test_same_bits_tells_what_array_equal_does_not():
  for dt in (np.float32, np.float64):
    sub = np.finfo(dt).smallest_subnormal
    a = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, sub, 1.0], dt)
    assert values.same_bits(a, a.copy()).all()
    assert values.same_bits(a, -a).tolist() == [False] * 2 + [True] + [False] * 4
    b = a.copy()
    b[5] = 0.0                                   # a flushed subnormal
    assert values.same_bits(a, b).tolist() == [True] * 5 + [False, True]
    assert np.array_equal(np.array([0.0], dt), np.array([-0.0], dt),
                          equal_nan=True)        # what the old comparison saw
    assert not values.same_bits(np.array([np.nan], dt), np.array([1.0], dt))[0]
    assert not values.same_bits(np.array([1.0], dt), np.array([np.nan], dt))[0]
  i = np.array([-1, 0, 255], np.int16)
  assert values.same_bits(i, i.copy()).all()
  assert values.same_bits(i, i + 1).tolist() == [False] * 3


def test_special_values_and_tables():
  for t in ('float', 'double'):
    s = values.special_values(np.dtype({'float': 'f4', 'double': 'f8'}[t]))
    info = np.finfo(s.dtype)
    for v in (0.0, info.smallest_subnormal, info.smallest_normal, info.max,
              np.inf, 1.0):
      assert (s == v).any() and (s == -v).any(), v
    assert np.signbit(s[s == 0]).any() and int(np.isnan(s).sum()) == 1
    assert len({x.tobytes() for x in s}) == len(s)
  for t, n in (('uint8', 12), ('int16', 27), ('uint16', 15), ('int32', 27)):
    s = values.special_values(np.dtype(t))
    info = np.iinfo(s.dtype)
    assert len(set(s.tolist())) == len(s) == n, (t, len(s))
    assert {info.min, info.max, 0, 1, 100}.issubset(s.tolist())
  stencil = _typed(['int16', 'int16'])
  ins = values.table_inputs(stencil, (40, 33))
  s = values.special_values(np.int16)
  pairs = {(int(a), int(b)) for a, b in zip(ins['t0'].reshape(-1),
                                            ins['t1'].reshape(-1))}
  assert pairs == {(int(a), int(b)) for a in s for b in s}


def test_the_generators_reach_every_type_and_class():
  kinds = set()
  for gen, seeds in GENERATORS.items():
    assert len(seeds) >= 4, gen
    for seed in seeds:
      kinds |= {str(t) for t in _case(gen, seed)[1].input_types}
  assert kinds >= set(fuzz.FLOAT_TYPES + fuzz.INT_TYPES), kinds
  # at least one window seed per input type of the window generator
  assert {str(_case('window', s)[1].input_types[0])
          for s in WINDOW_SEEDS} == set(fuzz.WINDOW_TYPES)
  assert {109, 177, 283, 326, 454} <= set(WINDOW_SEEDS)
  # the rich generator's float -> int32 casts keep `nonfinite` out, and only
  # there
  with_casts = [s for s in RICH_SEEDS
                if 'nonfinite' not in _classes('rich', s) and
                _classes('rich', s) != values.INT_CLASSES]
  assert with_casts and all('int32(' in _case('rich', s)[0] for s in with_casts)
  assert any(_classes('rich', s) == values.FLOAT_CLASSES for s in RICH_SEEDS)
  assert all(_classes('plain', s) in (values.FLOAT_CLASSES, values.INT_CLASSES)
             for s in PLAIN_SEEDS)


# ---------------------------------------------------------------------------
# CPU: the two oracles agree wherever the GPU is compared with one of them
# ---------------------------------------------------------------------------

def _oracles_agree(stencil, ins, what, iterate=None):
  from oracle import numpy_oracle
  a = numpy_oracle.run(stencil, ins, **({} if iterate is None else
                                        {'iterate': iterate}))
  b = _oracle(stencil).run(ins, iterate=iterate)
  for o in stencil.output_names:
    same = values.same_bits(a[o], b[o])
    assert same.all(), '%s, output %s: %d cells differ' % (
        what, o, int((~same).sum()))
  return b


@pytest.mark.parametrize('gen,seed', [(g, s) for g in ('plain', 'rich', 'window')
                                      for s in GENERATORS[g]])
def test_oracles_agree_on_random_programs(built, gen, seed):
  text, stencil, extent = _case(gen, seed)
  if gen == 'window':              # as tests/test_fuzz.py: a corner of the grid
    small = tuple(min(e, 70) for e in extent)
    lo, hi = stencil.valid_box(small)
    if all(h > l for l, h in zip(lo, hi)):
      extent = small
  for kind in _classes(gen, seed):
    ins = values.edge_inputs(stencil, extent, seed, kind)
    _oracles_agree(stencil, ins, '%s seed %d, %s\n%s' % (gen, seed, kind, text))


@pytest.mark.parametrize('seed', PRESERVE_SEEDS)
def test_oracles_agree_with_preserved_border(built, seed):
  text, stencil, extent = _case('preserve', seed)
  for kind in _classes('preserve', seed):
    ins = values.edge_inputs(stencil, extent, seed, kind)
    _oracles_agree(stencil, ins, 'seed %d, %s\n%s' % (seed, kind, text))


def test_few_cases_are_left_out_for_their_nan_share(built):
  """At most one (seed, class) case in ten per generator.  (Plain seed 43, a
  cubic iterated three times, is 85-100 % NaN in the oracle in every float
  class; the rich and window generators have no such program among their first
  40 and 24 seeds.)"""
  for gen, seeds in GENERATORS.items():
    cases = [(s, k) for s in seeds for k in _classes(gen, s)]
    out = [c for c in cases if _left_out(gen, *c)]
    print('%s: %d cases, left out: %s' % (gen, len(cases), out))
    assert len(out) * 10 <= len(cases), (gen, out)
    if gen == 'window':
      assert not out


# ---------------------------------------------------------------------------
# ldswin programs, corpus kernels, operator tables: texts and CPU halves
# ---------------------------------------------------------------------------

# (tests/test_hip_parity.py WIDE_INT / WIDE_FLOAT: taps on both sides of the
# cell with a folded local; an off-centre store with a division and a root)
WIDE_INT = """kernel: wideint
burst width: 64
unroll factor: 2
iterate: 1
input int32: a(64, *)
local int32: s(0, 0) = a(-6, -3) * 3 + a(-2, -1) * 5 - a(0, 0) + a(3, 1) * 7 + a(7, 2)
output int32: b(0, 0) = s(0, 0) / 3 + a(-5, 2) * a(6, -3) - a(1, 0)
"""

WIDE_FLOAT = """kernel: widefloat
burst width: 64
unroll factor: 2
iterate: 1
input float: a(64, *)
output float: b(1, -1) = (a(-9, -2) + a(12, 0) * 0.25f) * (a(0, 1) - a(3, -4) / (1.5f + a(2, 2) * a(2, 2))) + sqrt(a(10, 3) + 1.0f) + a(-1, -1) * a(11, -4)
"""

LDSWIN_CASES = ['wideint', 'widefloat'] + ['wide%d' % s for s in WIDE_SEEDS]


@functools.lru_cache(maxsize=None)
def _ldswin_case(name):
  """(text, stencil, seed)."""
  from soda_amd import core
  if name.startswith('wide') and name[4:].isdigit():
    seed = int(name[4:])
    text = _case('wide', seed)[0]
  else:
    seed, text = {'wideint': (901, WIDE_INT), 'widefloat': (902, WIDE_FLOAT)}[name]
  return text, core.from_text(text), seed


def _ldswin_module(stencil):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(
      stencil, lower.LowerOptions(strategy='ldswin'), None, probe=False)
  return lower.lower(stencil, opts)


def _ldswin_shape(k):
  """(extent, step, live rows) of an ldswin kernel `..._S<step>_R<ring>_C..`:
  one full tile and a ragged one each way."""
  import re
  m = re.search(r'_ldswin_V\d+_S(\d+)_R(\d+)_C', k.name)
  step, ring = int(m.group(1)), int(m.group(2))
  return (k.tile[0] + 40, k.tile[1] + 11), step, ring - step


def _ldswin_cells(stencil, k):
  """The last quad of the first block's columns and the first column of the
  next block, in input rows past the `live` rows a block loads before its
  first step: rows filed in the ring while a step computes.  Then the first
  and the last cell of the valid box."""
  extent, step, live = _ldswin_shape(k)
  lo, hi = stencil.valid_box(extent)
  w = k.tile[0]
  r1, r2 = live + 1, live + step + 2
  assert r2 + step < extent[1] and w < extent[0]
  cells = [(w - 4, r1), (w - 1, r1 + 1), (w, r2), (w - 2, r2 + step),
           tuple(lo), tuple(h - 1 for h in hi)]
  assert len(set(cells)) == 6
  return extent, cells


@pytest.mark.parametrize('name', LDSWIN_CASES)
def test_oracles_agree_on_ldswin_programs(built, name):
  text, stencil, seed = _ldswin_case(name)
  mod = _ldswin_module(stencil)
  assert [p.kind for p in mod.passes] == ['ldswin']
  extent, cells = _ldswin_cells(stencil, mod.kernels[0])
  for kind in values.classes_for(stencil, text):
    ins = values.edge_inputs(stencil, extent, seed, kind, at=cells)
    _oracles_agree(stencil, ins, '%s, %s' % (name, kind))


_TABLE_HEAD = '''kernel: %s
burst width: 64
unroll factor: 2
iterate: 1
input %s: a(32, *)
input %s: b
'''


def _table_text(group, t):
  """One tiny program per operator group on two tensors of type `t`: every
  expression an output of its own, so that no result hides another."""
  f = {'float': 'f', 'double': ''}.get(t)
  other = {'float': 'double', 'double': 'float'}.get(t)
  exprs = {
      # ---- floats
      'fdiv': ['a(0, 0) / b(0, 0)', 'b(-1, 0) / a(1, 0)'],
      'sqrt': ['sqrt(a(0, 0)) + sqrt(b(0, 0) * b(0, 0))'],
      'fminmax': ['min(a(0, 0), b(0, 0))', 'max(a(0, 0), b(0, 0))',
                  'min(b(1, 0), a(-1, 0))', 'max(b(1, 0), a(-1, 0))'],
      'fselect': ['select(a(0, 0) < b(0, 0), a(0, 0), b(0, 0))',
                  'select(a(0, 0) == b(0, 0), a(1, 0), b(0, 1))',
                  'select(a(0, 0) < b(0, 0) || b(1, 0) == a(-1, 0), '
                  'a(-1, 0), b(1, 0))'],
      'fcast': ['%s(%s(a(0, 0)))' % (t, other),
                '%s(%s(a(-1, 0)) * %s(b(0, 0)))' % (t, other, other)],
      'fround': ['floor(a(0, 0))', 'ceil(a(0, 0))', 'fabs(b(0, 0))',
                 'abs(a(1, 0))', 'floor(a(-1, 0) * 0.5%s) + ceil(b(0, 0))' % f],
      'fzero': ['(a(0, 0) + b(0, 0)) * 0.5%s + (a(0, 0) - a(0, 0)) + '
                'b(0, 0) * 0.0%s' % (f, f)],
      # ---- integers
      'idiv': ['a(-1, 0) / 3', 'a(1, 0) % 7', 'b(0, 1) / 2', 'b(0, -1) % 8'],
      'imul': ['a(0, 0) * b(0, 0)', 'a(-1, 0) * b(1, 0) * 3 + a(1, 0)'],
      'ineg': ['abs(a(0, 0))', '-a(0, 0)', 'abs(a(-1, 0) - b(0, 0))',
               '-(a(1, 0) * b(0, 0))'],
      'iminmax': ['min(a(0, 0), 100)', 'max(b(0, 0), 7)',
                  'max(min(a(-1, 0), b(1, 0)), 3)'],
      'iselect': ['select(a(0, 0) < b(0, 0), a(0, 0), b(0, 0))',
                  'select(a(0, 0) == b(0, 0) || a(1, 0) > b(0, 1), a(1, 0), '
                  'b(0, 1))'],
      'ibits': ['a(0, 0) & b(0, 0)', 'a(0, 0) | b(1, 0)', 'a(-1, 0) ^ b(0, 0)'],
      'iwide': ['%s(int64(a(0, 0)) * 100003 %% 1009)' % t,
                '%s(int64(a(-1, 0)) * int64(b(0, 0)) / 5)' % t],
      'isum7': [' + '.join('a(%d, 0)' % d for d in range(-3, 4))],
  }[group]
  lines = [_TABLE_HEAD % ('%s_%s' % (group, t), t, t)]
  for i, e in enumerate(exprs):
    lines.append('output %s: o%d(0, 0) = %s\n' % (t, i, e))
  return ''.join(lines)


FLOAT_GROUPS = ['fdiv', 'sqrt', 'fminmax', 'fselect', 'fcast', 'fround',
                'fzero']
INT_GROUPS = ['idiv', 'imul', 'ineg', 'iminmax', 'iselect', 'ibits', 'iwide',
              'isum7']
TABLES = [(g, t) for t in fuzz.FLOAT_TYPES for g in FLOAT_GROUPS] + \
    [(g, t) for t in fuzz.INT_TYPES for g in INT_GROUPS]
TABLE_ROWS = 48          # the longest table has 37 values; 3 rows of border


@functools.lru_cache(maxsize=None)
def _table_stencil(group, t):
  from soda_amd import core
  return core.from_text(_table_text(group, t))


def _table_extent(k):
  """Two strips and a bit (nine lanes): halo lanes carry special values too."""
  return (2 * k.tile[0] + 9 * (k.tune or {}).get('vec', 4), TABLE_ROWS)


def _table_reference(stencil, extent):
  ins = values.table_inputs(stencil, extent)
  n = len(values.special_values(ins['a'].dtype))
  for o, idx in _boxes(stencil, extent):
    assert all(s.stop - s.start >= n for s in idx), 'not every pair meets'
  want = _oracle(stencil).run(ins)
  assert _nan_share(stencil, extent, want) <= NAN_SHARE_TABLE
  return ins, want


@pytest.mark.parametrize('group,t', TABLES)
def test_oracles_agree_on_operator_tables(built, group, t):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _table_stencil(group, t)
  mod = lower.lower(stencil, runtime.resolve_options(
      stencil, lower.LowerOptions(fuse=(2,)), None, probe=False))
  extent = _table_extent(mod.kernels[0])
  ins, want = _table_reference(stencil, extent)
  got = _oracles_agree(stencil, ins, '%s %s' % (group, t))
  share = _nan_share(stencil, extent, got)
  print('%s %s on %s: NaN share %.3f' % (group, t, extent, share))
  assert share <= NAN_SHARE_TABLE
  if t in fuzz.FLOAT_TYPES and group != 'fround':
    assert share > 0           # the tables do reach the non-finite results


# (program, iterate, options, grid from the deepest kernel's (S, V)): the
# shapes of tests/test_batch.py
CORPUS = {
    'jacobi2d_T13': ('jacobi2d.soda', 15, dict(fuse=(13,), chunk_rows=16),
                     lambda s, v: (2 * s + 36, 50)),
    'jacobi2d_pipe4': ('jacobi2d.soda', 15, dict(fuse=(4,), pipe=4,
                                                 chunk_rows=16),
                       lambda s, v: (2 * s + 36, 50)),
    'heat3d': ('heat3d.soda', 3, dict(fuse=(2,)),
               lambda s, v: (s + 9 * v, 9, 12)),
    'heat3d_xshare': ('heat3d.soda', 3, dict(fuse=(2,), xshare=True),
                      lambda s, v: (s + 9 * v, 9, 12)),
    'heat3d_xb2': ('heat3d.soda', 3, dict(fuse=(2,), xshare_block=2),
                   lambda s, v: (s + 9 * v, 9, 12)),
    'heat3d_tile3d': ('heat3d.soda', 4, dict(strategy='tile3d', fuse=(3,)),
                      lambda s, v: (100, 20, 9)),
    'denoise2d': ('denoise2d.soda', None, dict(), lambda s, v: (72, 40)),
    # param arrays: the weights hold both zeros and a subnormal -- and, in the
    # one-iteration case, an infinity (every cell is then +inf, -inf or NaN by
    # the sign of the cell the infinite weight multiplies)
    'conv2d': ('conv2d.soda', None, dict(fuse=(2,)), lambda s, v: (264, 33)),
    'conv2d_inf': ('conv2d.soda', 1, dict(), lambda s, v: (264, 33)),
}


def _corpus_stencil(name):
  from soda_amd import core
  soda, iterate, kw, grid = CORPUS[name]
  extra = {} if iterate is None else {'iterate': iterate}
  return core.from_file(soda_path(soda), **extra)


def _deepest(mod):
  return max(mod.kernels, key=lambda k: (k.tune or {}).get('fused', 0))


def _corpus_inputs(name, stencil, extent, strip, chunk, kind):
  cells = _seam_cells(stencil, extent, strip, chunk) \
      if kind == 'nonfinite' else None
  ins = values.edge_inputs(stencil, extent, 77, kind, at=cells)
  if 'w' in ins:
    w = ins['w'].copy()
    w.reshape(-1)[[0, 2, 4]] = [0.0, -0.0,
                                5 * np.finfo(w.dtype).smallest_subnormal]
    if name == 'conv2d_inf':
      w.reshape(-1)[8] = np.inf
    ins['w'] = w
  return ins


@pytest.mark.parametrize('name', sorted(CORPUS))
def test_oracles_agree_on_corpus_kernels(built, name):
  """On the grids of the GPU test, the non-finite cells at the seams of the
  module as it is lowered without trial compilations."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  soda, iterate, kw, grid = CORPUS[name]
  stencil = _corpus_stencil(name)
  mod = lower.lower(stencil, runtime.resolve_options(
      stencil, lower.LowerOptions(**dict(kw, row_cells=None)), None,
      probe=False))
  k = _deepest(mod)
  extent = grid(k.tile[0], (k.tune or {}).get('vec', 4))
  for kind in values.FLOAT_CLASSES:
    ins = _corpus_inputs(name, stencil, extent, k.tile[0],
                         k.tile[stencil.dim - 1], kind)
    want = _oracles_agree(stencil, ins, '%s, %s' % (name, kind))
    share = _nan_share(stencil, extent, want)
    print('%s %s on %s: NaN share %.3f' % (name, kind, extent, share))
    if name == 'conv2d_inf':
      assert 0 < share < 0.1        # 0 * inf, in the 2 % of cells that are zero
      assert not np.isfinite(want['out'][1:-1, 1:-1]).any()
    elif kind == 'nonfinite':
      assert 0 < share < 1          # the infinities meet; most cells stay finite
    else:
      assert share == 0


SEAM_I32 = '''kernel: i32
burst width: 64
unroll factor: 2
iterate: 6
input int32: a(32, 32, *)
output int32: b(0,0,0) = (a(0,0,1) - a(1,0,0) * 3) / 2 + a(0,-1,-1) % 7
'''
# (tests/test_tile3d.py test_chunk_seams_of_a_deep_kernel: depth 6 across
# chunks of 16 planes, two launches of it and one of the remainder pass)
SEAM_FUSE, SEAM_ITERATE, SEAM_PLANES, SEAM_CHUNK = (6,), 13, 61, 16


@functools.lru_cache(maxsize=None)
def _seam_case():
  """(stencil, extent, valid tile): one valid tile and five cells along x, as
  many tiles along y as leave 13 iterations a valid row, and three rows."""
  from soda_amd import core
  from soda_amd.codegen.hip import lower
  stencil = core.from_text(SEAM_I32, iterate=SEAM_ITERATE)
  mod = lower.lower(stencil, lower.LowerOptions(strategy='tile3d',
                                                fuse=SEAM_FUSE))
  deepest = max((p for p in mod.passes if p.kind == 'tile3d'),
                key=lambda p: p.fused_iters)
  assert deepest.fused_iters == 6
  vx, vy = mod.kernels[deepest.kernels[0]].tile[:2]
  mul = 1
  while True:
    extent = (vx + 5, mul * vy + 3, SEAM_PLANES)
    lo, hi = stencil.valid_box(extent, 'b', SEAM_ITERATE)
    if all(h > l for l, h in zip(lo, hi)):
      return stencil, extent, (vx, vy)
    mul += 1


def test_oracles_agree_on_wrapping_int32_at_depth_13(built):
  """13 iterations of (a - 3 b) / 2 + c % 7 on cells of the whole int32 range:
  the arithmetic wraps in every iteration, and both oracles wrap alike."""
  stencil, extent, _ = _seam_case()
  ins = values.edge_inputs(stencil, extent, 19, 'full')
  # the first iteration already leaves int32: a - 3 b computed in 64 bits
  a = ins['a'].astype(np.int64)
  exact = a[2:, :, :-1] - 3 * a[1:-1, :, 1:]
  assert (np.abs(exact) > 2 ** 31).mean() > 0.3
  _oracles_agree(stencil, ins, 'i32 seam', iterate=SEAM_ITERATE)


# ---------------------------------------------------------------------------
# CPU: the float mode of the kernels the JIT builds
# ---------------------------------------------------------------------------

DOUBLE_MODULE = '''kernel: dmode
burst width: 64
unroll factor: 2
iterate: 2
input double: a(32, *)
output double: b(0, 0) = (a(-1, 0) + a(1, 0) + a(0, -1) + a(0, 1)) * 0.25
'''


def _float_modes(code):
  """{kernel: (round 32, round 16/64, denorm 32, denorm 16/64)} from the
  kernel descriptors of a code object: `<kernel>.kd` is 64 bytes, its
  COMPUTE_PGM_RSRC1 word sits at byte 48 and holds FLOAT_ROUND_MODE_32 in bits
  12-13, FLOAT_ROUND_MODE_16_64 in 14-15, FLOAT_DENORM_MODE_32 in 16-17 and
  FLOAT_DENORM_MODE_16_64 in 18-19 (LLVM's AMDGPU usage guide, "Kernel
  Descriptor"; hsa/amd_hsa_kernel_code.h)."""
  from soda_amd import isa
  out = {}
  for name, sym in isa._symbols(code).items():
    if not name.endswith('.kd'):
      continue
    kd = isa._symbol_bytes(code, sym)
    assert len(kd) == 64, (name, len(kd))
    rsrc1, = struct.unpack_from('<I', kd, 48)
    out[name[:-3]] = tuple((rsrc1 >> b) & 3 for b in (12, 14, 16, 18))
  return out


@pytest.mark.parametrize('name', ['float', 'double', 'ldswin'])
def test_jit_kernels_keep_subnormals_and_round_to_nearest(built, name):
  """hipcc's default for gfx950 is to keep fp32 and fp16/64 subnormals; that
  hiprtc, with runtime.COMPILE_OPTIONS, does the same is what the `tiny` cases
  rest on.  Read from the mode word of every kernel descriptor, built as
  runtime.Program builds a module."""
  from soda_amd import core, runtime
  from soda_amd.codegen.hip import lower
  stencil, opts = {
      'float': lambda: (core.from_file(soda_path('jacobi2d.soda'), iterate=6),
                        lower.LowerOptions(fuse=(4,))),
      'double': lambda: (core.from_text(DOUBLE_MODULE),
                         lower.LowerOptions(fuse=(2,))),
      'ldswin': lambda: (core.from_text(WIDE_FLOAT),
                         lower.LowerOptions(strategy='ldswin')),
  }[name]()
  mod = lower.lower(stencil, runtime.resolve_options(stencil, opts, None))
  code = runtime.compile_source(mod.source, '%s.hip' % stencil.app_name)
  modes = _float_modes(code)
  assert set(modes) == {k.name for k in mod.kernels}, modes
  if name == 'ldswin':
    assert all('ldswin' in k for k in modes)
  NEAREST, NO_FLUSH = 0, 3
  for kernel, mode in modes.items():
    assert mode == (NEAREST, NEAREST, NO_FLUSH, NO_FLUSH), (kernel, mode)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _program(stencil, extent=None, **kw):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  if extent is None:
    return runtime.Program(stencil, lower.LowerOptions(**kw), calibrate=False)
  return runtime.Program(stencil, lower.LowerOptions(**kw), extent=extent)


def _run_classes(gen, seed, variants, whole=False):
  """Every class of a random-program case on ONE Program per variant."""
  text, stencil, extent = _case(gen, seed)
  kinds = [k for k in _classes(gen, seed) if not _left_out(gen, seed, k)]
  ran = 0
  for kw in variants:
    with _program(stencil, extent, **kw) as prog:
      names = [k.name for k in prog.module.kernels]
      for kind in kinds:
        ins, want = _reference(gen, seed, kind)
        got = prog.run(dict(ins))
        _assert_same(stencil, extent, got, want, '%s seed %d, %s, %s (%s)\n%s' %
                     (gen, seed, kind, kw, names, text), whole=whole)
        ran += 1
      if 'nonfinite' in kinds and stencil.dim >= 2:
        # ... and once more with the six cells at THIS module's seams
        k = _deepest(prog.module)
        cells = _seam_cells(stencil, extent, k.tile[0],
                            prog.geometry(extent)[0][k.name][stencil.dim - 1],
                            strict=False)
        if cells is None:
          continue
        ins = values.edge_inputs(stencil, extent, seed, 'nonfinite', at=cells)
        want = _oracle(stencil).run(ins)
        if _nan_share(stencil, extent, want, whole=whole) > NAN_SHARE_LEFT_OUT:
          continue
        _assert_same(stencil, extent, prog.run(ins), want,
                     '%s seed %d, nonfinite at the seams %s, %s (%s)\n%s' %
                     (gen, seed, cells, kw, names, text), whole=whole)
  return ran


AUTO_AND_DIRECT = (dict(strategy='auto', fuse=(2,)),
                   dict(strategy='direct', fuse=(2,)))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', PLAIN_SEEDS)
def test_gpu_plain_programs(built, seed):
  _run_classes('plain', seed, AUTO_AND_DIRECT)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', RICH_SEEDS)
def test_gpu_rich_programs(built, seed):
  _run_classes('rich', seed, AUTO_AND_DIRECT)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', PRESERVE_SEEDS)
def test_gpu_programs_with_preserved_border(built, seed):
  """The WHOLE grid is defined: border cells pass through with their bits."""
  _run_classes('preserve', seed, AUTO_AND_DIRECT, whole=True)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', WINDOW_SEEDS)
def test_gpu_window_programs(built, seed):
  """Sliding sums, joint dimension-0 windows and power-of-two chains on
  integers of the whole range; `direct` shares none of the rewrites."""
  assert _run_classes('window', seed, AUTO_AND_DIRECT) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('seed', XSHARE_SEEDS)
def test_gpu_shared_rows(built, seed):
  """x-halos through LDS, on whole rows (xshare) and on segments of two waves
  (xshare_block = 2: a segment and nine lanes per row)."""
  from soda_amd import runtime
  text, stencil, extent = _case('plain', seed)
  kinds = values.classes_for(stencil, text)
  with _program(stencil, extent, fuse=(2,), xshare=True) as prog:
    names = [k.name for k in prog.module.kernels]
    assert any('_xs' in n for n in names), names
    for kind in kinds:
      ins = values.edge_inputs(stencil, extent, seed, kind)
      want = _oracle(stencil).run(ins)
      _assert_same(stencil, extent, prog.run(ins), want,
                   'seed %d, %s, xshare (%s)' % (seed, kind, names))
  with _program(stencil, fuse=(2,), xshare_block=2) as prog:
    k = _deepest(prog.module)
    assert '_xb2' in k.name, k.name
    extent = (k.tile[0] + 9 * k.tune['vec'],) + tuple(extent[1:])
    assert prog.schedule(extent, stencil.iterate).get(2)
    for kind in kinds:
      cells = _seam_cells(stencil, extent, k.tile[0],
                          prog.geometry(extent)[0][k.name][stencil.dim - 1]) \
          if kind == 'nonfinite' else None
      ins = values.edge_inputs(stencil, extent, seed, kind, at=cells)
      want = _oracle(stencil).run(ins)
      _assert_same(stencil, extent, prog.run(ins), want,
                   'seed %d, %s, xshare_block=2 (%s)' % (seed, kind, k.name))


@pytest.mark.gpu
@pytest.mark.parametrize('seed', TILE3D_SEEDS)
def test_gpu_tile3d_random_programs(built, seed):
  from soda_amd import core
  text = fuzz.program(seed)[0]
  extent, iterate = TILE3D_EXTENT, TILE3D_ITERATE
  stencil = core.from_text(text, iterate=iterate)
  assert stencil.dim == 3
  ran = 0
  with _program(stencil, extent, strategy='tile3d', fuse=(4, 3)) as prog:
    kinds = {p.fused_iters: p.kind for p in prog.module.passes}
    assert 'tile3d' in kinds.values(), kinds
    for kind in values.classes_for(stencil, text):
      ins = values.edge_inputs(stencil, extent, seed, kind)
      want = _oracle(stencil).run(ins, iterate=iterate)
      if _nan_share(stencil, extent, want, iterate) > NAN_SHARE_LEFT_OUT:
        continue
      _assert_same(stencil, extent, prog.run(ins, iterate=iterate), want,
                   'seed %d, %s, tile3d %s' % (seed, kind, kinds), iterate)
      ran += 1
  assert ran


def test_tile3d_random_cases_are_not_left_out(built):
  """Of the classes the tile3d seeds run in, at most one in ten is dropped for
  its NaN share (four iterations of a product-heavy program overflow)."""
  from soda_amd import core
  cases, out = 0, []
  for seed in TILE3D_SEEDS:
    text = fuzz.program(seed)[0]
    stencil = core.from_text(text, iterate=TILE3D_ITERATE)
    for kind in values.classes_for(stencil, text):
      ins = values.edge_inputs(stencil, TILE3D_EXTENT, seed, kind)
      want = _oracles_agree(stencil, ins, 'seed %d %s' % (seed, kind),
                            iterate=TILE3D_ITERATE)
      cases += 1
      if _nan_share(stencil, TILE3D_EXTENT, want, TILE3D_ITERATE) > \
          NAN_SHARE_LEFT_OUT:
        out.append((seed, kind))
  print('tile3d: %d cases, left out: %s' % (cases, out))
  assert len(out) * 10 <= cases, out


@pytest.mark.gpu
def test_gpu_tile3d_wrapping_int32_across_chunk_seams(built):
  """Full-range int32 cells through depth 6 twice and the remainder pass,
  chunks of 16 planes: every iteration wraps, on both sides alike."""
  stencil, extent, tile = _seam_case()
  ins = values.edge_inputs(stencil, extent, 19, 'full')
  want = _oracle(stencil).run(ins, iterate=SEAM_ITERATE)
  with _program(stencil, extent, strategy='tile3d', fuse=SEAM_FUSE,
                chunk_rows=SEAM_CHUNK) as prog:
    sched = {t: n for t, n in prog.schedule(extent, SEAM_ITERATE).items() if n}
    assert sched == {6: 2, 1: 1}
    k, = [k for k in prog.module.kernels if '_tile3d_T6_' in k.name]
    assert k.tile[:2] == tuple(tile)
    got = prog.run(ins, iterate=SEAM_ITERATE)
  _assert_same(stencil, extent, got, want, 'i32 at depth 6', SEAM_ITERATE)


@pytest.mark.gpu
@pytest.mark.parametrize('name', LDSWIN_CASES)
def test_gpu_ldswin(built, name):
  """One full tile and a ragged one each way; the non-finite cells in the last
  quad of a block's columns, in ring rows filed while a step computes."""
  text, stencil, seed = _ldswin_case(name)
  with _program(stencil, strategy='ldswin') as prog:
    k, = prog.module.kernels
    assert 'ldswin' in k.name
    extent, cells = _ldswin_cells(stencil, k)
    assert prog.geometry(extent)[0][k.name][:2] == k.tile[:2]
    for kind in values.classes_for(stencil, text):
      ins = values.edge_inputs(stencil, extent, seed, kind, at=cells)
      want = _oracle(stencil).run(ins)
      _assert_same(stencil, extent, prog.run(ins), want,
                   '%s, %s (%s)' % (name, kind, k.name))


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CORPUS))
def test_gpu_corpus_kernels_at_their_seams(built, name):
  """Two strips and a bit, several chunks: the non-finite cells on both sides
  of a strip seam and of a chunk seam and in the corners of the valid box.
  Where +inf and -inf meet within the fused depth the oracle is NaN, and it
  must be the same cells on the GPU; everywhere else the bits match."""
  soda, iterate, kw, grid = CORPUS[name]
  stencil = _corpus_stencil(name)
  iterate = stencil.iterate
  if name == 'heat3d_xshare':         # rows a whole block covers
    with _program(stencil, fuse=(2,)) as plain:
      k = _deepest(plain.module)
      kw = dict(kw, row_cells=k.tile[0] + 9 * k.tune['vec'])
  with _program(stencil, **kw) as prog:
    k = _deepest(prog.module)
    tag = {'jacobi2d_pipe4': '_pipe4', 'heat3d_xshare': '_xs',
           'heat3d_xb2': '_xb2', 'heat3d_tile3d': 'tile3d'}.get(name)
    if tag:
      assert tag in k.name, k.name
    if name == 'denoise2d':
      assert 'rsqrt' in prog.module.source
    s, v = k.tile[0], (k.tune or {}).get('vec', 4)
    if name == 'heat3d_xshare':
      extent = (kw['row_cells'], 9, 12)
    else:
      extent = grid(s, v)
    chunk = prog.geometry(extent)[0][k.name][stencil.dim - 1]
    if 'chunk_rows' in kw:
      assert chunk == kw['chunk_rows']
    deepest = max(p.fused_iters for p in prog.module.passes)
    if deepest > 1:
      assert prog.schedule(extent, iterate).get(deepest)
    for kind in values.FLOAT_CLASSES:
      ins = _corpus_inputs(name, stencil, extent, s, chunk, kind)
      want = _oracle(stencil).run(ins)
      assert 0 <= _nan_share(stencil, extent, want) < 1
      _assert_same(stencil, extent, prog.run(ins), want,
                   '%s, %s (%s)' % (name, kind, k.name))


GUARD = 0xA5


def _guarded_batch(stencil, prog, extent, batch, iterate, ins):
  """tests/test_batch.py `_guarded_run`: the device entry on output buffers
  one item longer at each end, handed the address of the second item; the two
  guard items must keep their fill pattern."""
  import ctypes
  from soda_amd import runtime
  lib, ptrs = runtime.library(), []

  def alloc(nbytes):
    p = ctypes.c_void_p()
    runtime.check(lib.soda_hip_malloc(prog.device, nbytes, ctypes.byref(p)),
                  'malloc')
    ptrs.append(p)
    return p

  try:
    shape = tuple(extent[::-1])
    d_in = []
    for n in stencil.input_names:
      arr = np.ascontiguousarray(ins[n])
      p = alloc(arr.nbytes)
      runtime.check(lib.soda_hip_memcpy_h2d(p, arr.ctypes.data, arr.nbytes,
                                            None), 'h2d')
      d_in.append(p.value)
    d_out, item = [], []
    for t in stencil.output_types:
      item.append(int(np.prod(shape)) * np.dtype(t.np_name).itemsize)
      p = alloc((batch + 2) * item[-1])
      runtime.check(lib.soda_hip_memset(p, GUARD, (batch + 2) * item[-1],
                                        None), 'memset')
      d_out.append(p.value)
    runtime.check(lib.soda_hip_stream_synchronize(None), 'sync')
    prog.run_device([p + b for p, b in zip(d_out, item)], d_in, extent,
                    iterate, batch=batch)
    runtime.check(lib.soda_hip_stream_synchronize(None), 'sync')
    got = {}
    for o, t, p in zip(stencil.output_names, stencil.output_types, d_out):
      full = np.empty((batch + 2,) + shape, np.dtype(t.np_name))
      runtime.check(lib.soda_hip_memcpy_d2h(full.ctypes.data, p, full.nbytes,
                                            None), 'd2h')
      raw = full.view(np.uint8)
      assert (raw[0] == GUARD).all(), 'the item BEFORE the batch was written'
      assert (raw[-1] == GUARD).all(), 'the item BEHIND the batch was written'
      got[o] = full[1:-1]
    return got
  finally:
    for p in ptrs:
      lib.soda_hip_free(prog.device, p)


@pytest.mark.gpu
def test_gpu_a_batch_keeps_its_items_apart(built):
  """Item 0 holds infinities and NaNs, item 1 subnormals, item 2 neither: each
  matches its own oracle run, so no NaN and no subnormal crossed an item
  boundary."""
  from soda_amd import core
  iterate, kinds = 9, ('nonfinite', 'tiny', 'signed')
  stencil = core.from_file(soda_path('jacobi2d.soda'), iterate=iterate)
  with _program(stencil, fuse=(4,), batch=True) as prog:
    k = _deepest(prog.module)
    extent = (k.tile[0] + 44, 40)
    chunk = prog.geometry(extent, batch=3)[0][k.name][1]
    cells = _seam_cells(stencil, extent, k.tile[0], chunk)
    items = [values.edge_inputs(stencil, extent, 31 + i, kind, at=cells)
             for i, kind in enumerate(kinds)]
    want = [_oracle(stencil).run(item) for item in items]
    ins = {'t1': np.stack([item['t1'] for item in items])}
    assert prog.schedule(extent, iterate, 3) == {4: 2, 1: 1}
    for what, got in (('run_batch', prog.run_batch(ins)),
                      ('run_device', _guarded_batch(stencil, prog, extent, 3,
                                                    iterate, ins))):
      for i, kind in enumerate(kinds):
        _assert_same(stencil, extent, {'t0': got['t0'][i]}, want[i],
                     '%s, item %d (%s)' % (what, i, kind))
  (_, idx), = _boxes(stencil, extent)
  assert np.isnan(want[0]['t0'][idx]).any()
  assert np.isfinite(want[1]['t0'][idx]).all()
  assert np.isfinite(want[2]['t0'][idx]).all()
  small = np.abs(items[1]['t1'])
  assert ((small > 0) & (small < np.finfo(np.float32).smallest_normal)).any()
  assert np.isfinite(items[2]['t1']).all()


@pytest.mark.gpu
@pytest.mark.parametrize('group,t', TABLES)
def test_gpu_operator_tables(built, group, t):
  """Every ordered pair of special values through every operator of the group,
  on two strips and a bit, through the family `auto` picks and through
  `direct`."""
  stencil = _table_stencil(group, t)
  with _program(stencil, strategy='auto', fuse=(2,)) as auto:
    extent = _table_extent(auto.module.kernels[0])
    ins, want = _table_reference(stencil, extent)
    got = auto.run(ins)
    names = [k.name for k in auto.module.kernels]
  _assert_same(stencil, extent, got, want, '%s %s, auto (%s)' % (group, t, names))
  with _program(stencil, strategy='direct') as direct:
    got = direct.run(ins)
  _assert_same(stencil, extent, got, want, '%s %s, direct' % (group, t))
