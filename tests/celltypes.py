"""The ten native cell types as tests/test_celltypes.py runs them through every
form of the kernels: the types, one program per type and dimension (and a
second integer one with comparisons), the rows -- a form each -- with what it
means for a row to be in force, the two families that refuse by cell size, the
grids, and a hand-written templated C++ loop nest per program that knows
nothing of soda_amd or the oracles.

Nothing here needs a GPU; lowering needs neither the library nor a compiler."""
import collections
import ctypes
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np

import knobs

TYPES = ('int8', 'uint8', 'int16', 'uint16', 'int32', 'uint32', 'int64',
         'uint64', 'float', 'double')
FLOATS = ('float', 'double')
INTS = tuple(t for t in TYPES if t not in FLOATS)
SIZE = {'int8': 1, 'uint8': 1, 'int16': 2, 'uint16': 2, 'int32': 4,
        'uint32': 4, 'int64': 8, 'uint64': 8, 'float': 4, 'double': 8}
# their rows on the movement forms move the same bits as int32 / int64: those
# scale with the budget (SHARE of them at 1, all from 1 / SHARE on)
SAME_BITS_AS = {'uint32': 'int32', 'uint64': 'int64'}
SHARE = 0.25
SEED = knobs.SEED

# ---------------------------------------------------------------------------
# programs: (kind, dim) -> (expression of the program text, the same in C++
# over the taps A(dx, dy[, dz]) for the nest).  `main`: promotion of narrow
# cells to int and truncation on store, signed against unsigned division and
# remainder by a constant (a multiply-high sequence for 64-bit cells), wrap-
# around under -fwrapv.  `cmp`: a comparison between two taps, min and abs --
# unsigned comparison is in force for uint32 / uint64.
# ---------------------------------------------------------------------------

EXPR = {
    ('int', 2): '(a(0, 1) * 3 + a(1, 0) - a(-1, 0) * 5) / 4 + '
                '(a(0, -1) ^ a(0, 0)) % 7',
    ('int', 3): '(a(0, 0, 1) * 3 + a(1, 0, 0) - a(-1, 0, 0) * 5) / 4 + '
                '(a(0, -1, 0) ^ a(0, 1, 0)) % 7 + a(0, 0, -1)',
    ('cmp', 2): 'select(a(0, 1) > a(0, -1), min(a(1, 0), a(-1, 0)), '
                'abs(a(0, 0) - a(1, 0))) + a(0, 0) / 3',
    ('cmp', 3): 'select(a(0, 0, 1) > a(0, 0, -1), min(a(1, 0, 0), a(-1, 0, 0), '
                'a(0, 1, 0)), abs(a(0, 0, 0) - a(0, -1, 0))) + a(0, 0, 0) / 3',
    ('flt', 2): '(a(0, 1) + a(1, 0) + a(0, 0) + a(-1, 0) + a(0, -1)) * 0.2%s',
    ('flt', 3): '(a(0, 0, 1) + a(0, 1, 0) + a(1, 0, 0) + a(0, 0, 0) + '
                'a(-1, 0, 0) + a(0, -1, 0) + a(0, 0, -1)) * 0.125%s',
}
# the nest's own copy: taps and C++ text, written by hand
NEST = {
    ('int', 2): ([(0, 1), (1, 0), (-1, 0), (0, -1), (0, 0)],
                 '(A(0, 1) * 3 + A(1, 0) - A(-1, 0) * 5) / 4 + '
                 '(A(0, -1) ^ A(0, 0)) % 7'),
    ('int', 3): ([(0, 0, 1), (1, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 1, 0),
                  (0, 0, -1)],
                 '(A(0, 0, 1) * 3 + A(1, 0, 0) - A(-1, 0, 0) * 5) / 4 + '
                 '(A(0, -1, 0) ^ A(0, 1, 0)) % 7 + A(0, 0, -1)'),
    ('cmp', 2): ([(0, 1), (0, -1), (1, 0), (-1, 0), (0, 0)],
                 '(A(0, 1) > A(0, -1) ? lesser(A(1, 0), A(-1, 0)) : '
                 'magnitude(A(0, 0) - A(1, 0))) + A(0, 0) / 3'),
    ('cmp', 3): ([(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0),
                  (0, 0, 0), (0, -1, 0)],
                 '(A(0, 0, 1) > A(0, 0, -1) ? '
                 'lesser(lesser(A(1, 0, 0), A(-1, 0, 0)), A(0, 1, 0)) : '
                 'magnitude(A(0, 0, 0) - A(0, -1, 0))) + A(0, 0, 0) / 3'),
    ('flt', 2): ([(0, 1), (1, 0), (0, 0), (-1, 0), (0, -1)],
                 '(A(0, 1) + A(1, 0) + A(0, 0) + A(-1, 0) + A(0, -1)) * T(0.2)'),
    ('flt', 3): ([(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 0, 0), (-1, 0, 0),
                  (0, -1, 0), (0, 0, -1)],
                 '(A(0, 0, 1) + A(0, 1, 0) + A(1, 0, 0) + A(0, 0, 0) + '
                 'A(-1, 0, 0) + A(0, -1, 0) + A(0, 0, -1)) * T(0.125)'),
}
ITERATE = {2: 9, 3: 3}
# fixed LowerOptions, as knobs.PROGRAMS has them for jacobi2d_T4 and heat3d;
# `peel` as knobs.PEEL_PIN, on every row: no trial compilations
BASE = {2: dict(fuse=(4,), chunk_rows=16, peel=0),
        3: dict(fuse=(2,), chunk_rows=4, peel=1)}
KINDS = ('main', 'cmp')


def expr_key(t, kind):
  return 'flt' if t in FLOATS else ('int' if kind == 'main' else 'cmp')


def programs():
  """Every (type, dimension, kind) there is a program for."""
  return [(t, dim, kind) for dim in (2, 3) for t in TYPES for kind in KINDS
          if kind == 'main' or t in INTS]


def text(t, dim, kind='main', iterate=None):
  e = EXPR[expr_key(t, kind), dim]
  if t in FLOATS:
    e = e % ('f' if t == 'float' else '')
  return ('kernel: ct%s%dd_%s\nburst width: 64\nunroll factor: 2\n'
          'iterate: %d\ninput %s: a(%s*)\noutput %s: b(%s) = %s\n' % (
              '' if kind == 'main' else kind, dim, t, iterate or ITERATE[dim],
              t, '32, ' * (dim - 1), t, ', '.join(['0'] * dim), e))


@functools.lru_cache(maxsize=None)
def stencil_of(t, dim, kind='main', iterate=None):
  from soda_amd import core
  return core.from_text(text(t, dim, kind, iterate))


# ---------------------------------------------------------------------------
# rows: one form each
# ---------------------------------------------------------------------------

class Row(collections.namedtuple('Row', 'name dim items tag base')):
  """`kw` (kept as its sorted `items`): LowerOptions keywords beside BASE;
  `tag`: what the deepest kernel's name carries; `base`: every type runs it
  whatever the budget."""
  __slots__ = ()

  @classmethod
  def of(cls, name, dim, kw, tag, base):
    return cls(name, dim, tuple(sorted(kw.items())), tag, base)

  @property
  def kw(self):
    return dict(self.items)


ROWS = [
    Row.of('fused', 2, {}, '_T4_', True),
    Row.of('mixh', 2, dict(lane_shift='mixh'), '_mixh_', False),
    Row.of('pipe2', 2, dict(pipe=2), '_pipe2x2', False),
    Row.of('pipe4', 2, dict(pipe=4), '_pipe4x2', False),
    Row.of('waves_x2', 2, dict(waves_x=2), '_W2x1_', False),
    Row.of('waves_y2', 2, dict(waves_y=2), '_W1x2_', False),
    # (`row_cells`: the grid's width, keywords())
    Row.of('xshare', 2, dict(xshare=True, fuse=(2,)), '_xs', False),
    Row.of('xshare_block4', 2, dict(xshare_block=4), '_xb4', False),
    Row.of('vec1', 2, dict(vec=1), '_V1_', False),
    Row.of('vec2', 2, dict(vec=2), '_V2_', False),
    Row.of('direct', 2, dict(strategy='direct'), '_direct_', True),
    Row.of('batch', 2, dict(batch=True), '_bt', True),
    Row.of('residual', 2, dict(residual=True), '_rs', True),
    Row.of('fused', 3, {}, '_T2_', True),
    Row.of('xshare', 3, dict(xshare=True), '_xs', False),
    Row.of('xshare_block2', 3, dict(xshare_block=2), '_xb2', False),
    Row.of('direct', 3, dict(strategy='direct'), '_direct_', True),
    Row.of('batch', 3, dict(batch=True), '_bt', True),
    Row.of('residual', 3, dict(residual=True), '_rs', True),
]
ROW = {(r.name, r.dim): r for r in ROWS}
BATCH = 3
# rows without chunks: 2 S + 9 V cells by a few rows more than the iterations
# take away (tests/test_device_entry.py DIRECT)
DIRECT_ROWS = {2: (25,), 3: (9, 8)}
# the model does not schedule the deepest pass of these (type, row name, dim)
# alone: they run with the companion beside them.  Exact both ways
# (tests/test_celltypes.py)
UNSCHEDULED = {(t, name, 2) for t in ('int8', 'uint8')
               for name in ('fused', 'mixh', 'waves_x2', 'waves_y2',
                            'xshare_block4', 'batch', 'residual')}
UNSCHEDULED_COMPANION = {'vec': 8}


# residual rows whose deepest `_rs` twin spills ((type, dim) -> bytes of
# scratch): the library does not launch a twin that spills, such a run ends in
# the one-iteration twin.  Exact both ways (tests/test_celltypes.py)
SPILLING_TWIN = {('int32', 3): 20, ('int64', 3): 12}


# static LDS of a row's deepest kernel that shares x-halos between its waves,
# bytes by cell size, as hipcc 6 lays it out: halo cells of every wave seam,
# fused level and row (plane row in 3-D) in flight, and a few flag bytes.
# Pinned so that a halo sized for another cell width shows
SHARED_LDS = {
    ('xshare', 2): {1: 25, 2: 50, 4: 84, 8: 152},
    ('xshare_block4', 2): {1: 113, 2: 178, 4: 308, 8: 568},
    ('xshare', 3): {1: 145, 2: 274, 4: 532, 8: 1048},
    ('xshare_block2', 3): {1: 145, 2: 274, 4: 532, 8: 1048},
}


def unscheduled(t, row, kind='main'):
  """(the `cmp` programs are scheduled at sixteen cells a lane as well)"""
  return kind == 'main' and (t, row.name, row.dim) in UNSCHEDULED


def row_id(t, row, kind='main'):
  return '%s-%dd-%s%s' % (t, row.dim, row.name,
                          '' if kind == 'main' else '-' + kind)


def depth(row):
  return dict(BASE[row.dim], **row.kw)['fuse'][0]


def _lower(st, kw, extent, probe):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(st, lower.LowerOptions(**kw), extent,
                                 probe=probe)
  return lower.lower(st, opts)


def deepest(mod):
  """knobs.deepest, and the one kernel of a `direct` module."""
  return max(mod.kernels, key=lambda k: (k.tune or {}).get('fused') or 0)


@functools.lru_cache(maxsize=None)
def keywords_of(t, row, kind='main', alone=False):
  """LowerOptions keywords of a row for a type.  An `xshare` row names the row
  length its block covers: one strip of the plain kernel and nine lanes, as
  tests/test_device_entry.py sizes heat3d_xshare."""
  kw = dict(BASE[row.dim], **row.kw)
  if unscheduled(t, row, kind) and not alone:
    kw.update(UNSCHEDULED_COMPANION)
  if row.name == 'xshare':
    k = deepest(_lower(stencil_of(t, row.dim, kind), dict(kw, xshare=False),
                       None, False))
    kw['row_cells'] = k.tile[0] + 9 * k.tune['vec']
  return kw


def keywords(t, row, kind='main', alone=False):
  return dict(keywords_of(t, row, kind, alone))


@functools.lru_cache(maxsize=None)
def lowered(t, row, kind='main', extent=None, probe=False, alone=False):
  """The module of a row; `alone`: without the companion of UNSCHEDULED."""
  return _lower(stencil_of(t, row.dim, kind), keywords(t, row, kind, alone),
                extent, probe)


def in_force(t, row, mod, kind='main'):
  """Asserts that `mod` is the form the row asks for: the deepest kernel's
  name carries the tag, its depth is the one asked for, and where its
  descriptor has an entry for the form the entry agrees with the tag."""
  k = deepest(mod)
  name, tune = k.name, k.tune or {}
  names = [q.name for q in mod.kernels]
  tagged = names[k.twin] if row.name == 'residual' and k.twin >= 0 else name
  assert row.tag in tagged + '_', (row.tag, names)
  if row.name == 'direct':
    assert all('_direct_' in n for n in names) and \
        not tune.get('fused'), names
    assert tune['vec'] * SIZE[t] == 16, tune
    return
  assert tune['fused'] == depth(row) and '_T%d_' % depth(row) in name, names
  assert ('_mixh' in name) == (tune['lane_shift'] == 'mixh') == \
      (row.name == 'mixh'), name
  assert ('_pipe' in name) == (tune['pipe'] > 1) == \
      (row.name in ('pipe2', 'pipe4')), name
  if tune['pipe'] > 1:
    assert '_pipe%dx2' % tune['pipe'] in name and \
        tune['waves_per_block'] == tune['pipe'] == row.kw['pipe'], tune
    assert tune['lds_rings'] > 0, tune
  wx, wy = row.kw.get('waves_x', 1), row.kw.get('waves_y', 1)
  assert '_W%dx%d_' % (wx, wy) in name, name
  if row.dim == 2:
    assert tune['waves_along'] == wy and k.tile[1] == 16 * wy, (tune, k.tile)
  if wx * wy > 1:
    assert tune['waves_per_block'] == wx * wy, tune
  assert '_V%d_' % tune['vec'] in name and tune['vec'] * SIZE[t] <= 16, name
  if 'vec' in row.kw:
    assert tune['vec'] == min(row.kw['vec'], 16 // SIZE[t]), tune
  assert ('_xs' in name) == (row.name == 'xshare'), name
  if row.name == 'xshare':
    cells = keywords_of(t, row, kind)['row_cells']
    waves = tune['waves_per_block']
    assert name.endswith('_xs%d' % waves) and 1 <= waves <= 4, name
    per_wave = 64 * tune['vec']
    assert tune['max_extent0'] == k.tile[0] == waves * per_wave, tune
    assert (waves - 1) * per_wave < cells < waves * per_wave, (cells, tune)
  assert ('_xb' in name) == row.name.startswith('xshare_block'), name
  if row.name.startswith('xshare_block'):
    assert tune['waves_per_block'] == row.kw['xshare_block'], tune
    assert name.endswith('_xb%d' % row.kw['xshare_block']), name
  assert all(n.endswith('_bt') for n in names) == \
      any(n.endswith('_bt') for n in names) == (row.name == 'batch'), names
  assert any(n.endswith('_rs') for n in names) == (row.name == 'residual')
  if row.name == 'residual':
    assert k.twin >= 0 and names[k.twin] == name + '_rs', names
    assert mod.kernels[k.twin].tile == k.tile


# ---------------------------------------------------------------------------
# the two families that take some cell types only: (strategy, LowerOptions)
# -> (the types accepted, the refusal's text).  Exact both ways.
# ---------------------------------------------------------------------------

REFUSING = {
    'ldswin': (dict(strategy='ldswin'), 2,
               ('int32', 'uint32', 'float'), 'ldswin handles 4-byte cells'),
    'tile3d': (dict(strategy='tile3d', fuse=(2,)), 3,
               ('int32', 'uint32', 'float'),
               'tile3d handles float, int32 and uint32 cells'),
}


def refusal(family, t):
  """None if `family` takes cells of type `t`, else the text it refuses with."""
  kw, dim, takes, why = REFUSING[family]
  return None if t in takes else why


# ---------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def setup(t, row, kind='main', probe=False, alone=False):
  """(extent, extent to build the program for or None): knobs.setup on the
  module the row builds -- 2 S + 9 V cells of its deepest kernel along x,
  seven chunks and a ragged one.  An `xshare` row is as wide as `row_cells`
  says; an `xshare_block` row's S is the block's, so two blocks and a ragged
  third; a `direct` row has no chunks (DIRECT_ROWS)."""
  what = row_id(t, row, kind)
  width = None
  if row.name == 'xshare':
    cells = keywords_of(t, row, kind)['row_cells']
    width = lambda k: cells
  extent, build_for = knobs.settle(
      row.dim, lambda e: lowered(t, row, kind, e, probe, alone), what, width,
      deepest)
  if row.name == 'direct':
    assert build_for is None, what
    extent = (extent[0],) + DIRECT_ROWS[row.dim]
  return extent, build_for


def module_for(t, row, kind='main', probe=False, alone=False):
  extent, build_for = setup(t, row, kind, probe, alone)
  return lowered(t, row, kind, build_for, probe, alone), extent


# rows of the unsigned narrow types that scale with the budget as well -- set
# if the file's cold run takes more than a fifth of the rest of the GPU
# suite's ("Cell types": 179 s against a fifth of 781 s)
NARROW_UNSIGNED = ('uint8', 'uint16')
NARROW_ROWS = ('mixh', 'pipe4', 'waves_x2', 'waves_y2')
NARROW_UNDER_BUDGET = True


def always(t, row):
  """Does the GPU case of (type, row) run whatever the budget?"""
  if row.base:
    return True
  if NARROW_UNDER_BUDGET and t in NARROW_UNSIGNED and row.name in NARROW_ROWS:
    return False
  return t not in SAME_BITS_AS


def picks(cases, budget):
  """The budget's share of `cases`, evenly spread, as knobs.pair_picks."""
  total = len(cases)
  n = min(total, int(round(total * SHARE * max(0.0, budget))))
  return [cases[int(i * total / float(n))] for i in range(n)]


# ---------------------------------------------------------------------------
# wire: the 2-D program at two iterations on 2 and on 4 banks
# ---------------------------------------------------------------------------

BANKS = (2, 4)
WIRE_ROWS = 20
# (cell size, banks) whose dense program has no banked form: two 8-byte cells
# a lane are no whole group of four banks
NOT_BANKED = {(8, 4)}


@functools.lru_cache(maxsize=None)
def wire_tile(t, nb):
  """2 S + 9 V of the two-iteration kernel, rounded up to whole cycles of the
  stream (burst width / cell width x banks elements): a tile row that is not
  has no dense view, and the call runs the linear form."""
  st = stencil_of(t, 2, 'main', 2)
  k = deepest(_lower(st, dict(fuse=(2,), peel=0), None, False))
  assert k.tune['fused'] == 2
  per_cycle = 64 // (8 * SIZE[t]) * nb
  assert per_cycle <= k.tune['vec'] * 2
  return -(-(2 * k.tile[0] + 9 * k.tune['vec']) // per_cycle) * per_cycle


def wire_extent(t, nb):
  return (2 * wire_tile(t, nb) + wire_tile(t, nb) // 3, WIRE_ROWS)


# ---------------------------------------------------------------------------
# the reference of its own: one templated loop nest per program, g++
# ---------------------------------------------------------------------------

C_TYPE = {t: ('%s_t' % t if t in INTS else t) for t in TYPES}
NEST_FLAGS = ['-O2', '-ffp-contract=off', '-fwrapv', '-fPIC', '-shared']

_NEST_HEAD = '''\
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <type_traits>

// the lesser of two values and the magnitude of one, in the type the usual
// arithmetic conversions give the operands
template <class A, class B>
static inline auto lesser(A a, B b)
    -> typename std::decay<decltype(b < a ? b : a)>::type {
  return b < a ? b : a;
}
template <class A>
static inline auto magnitude(A a)
    -> typename std::decay<decltype(a < 0 ? -a : a)>::type {
  return a < 0 ? -a : a;
}
'''

_NEST_BODY = '''
// %(what)s: `iterate` sweeps, each over the cells whose taps all lie in the box
// of the sweep before; box[0 .. D) / box[D .. 2 D) receive the last one
template <class T>
static int %(fn)s(const T* in, T* out, const int64_t* n, int iterate,
%(pad)s int64_t* box) {
  enum { D = %(dim)d };
  static const int taps[][D] = {%(taps)s};
  int64_t below[D], above[D], stride[D], cells = 1;
  for (int d = 0; d < D; ++d) {
    below[d] = above[d] = 0;
    for (const auto& tap : taps) {
      if (-tap[d] > below[d]) below[d] = -tap[d];
      if (tap[d] > above[d]) above[d] = tap[d];
    }
    stride[d] = cells;
    cells *= n[d];
  }
  T* spare[2] = {nullptr, nullptr};
  for (int i = 0; i < 2 && i < iterate - 1; ++i) {
    spare[i] = static_cast<T*>(std::calloc(cells, sizeof(T)));
    if (!spare[i]) return 1;
  }
  std::memset(out, 0, cells * sizeof(T));
  const T* cur = in;
  int64_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
  for (int it = 0; it < iterate; ++it) {
    T* dst = it == iterate - 1 ? out : spare[it & 1];
    for (int d = 0; d < D; ++d) {
      lo[d] = (it + 1) * below[d];
      hi[d] = n[d] - (it + 1) * above[d];
    }
    for (int64_t z = lo[2]; z < hi[2]; ++z)
      for (int64_t y = lo[1]; y < hi[1]; ++y)
        for (int64_t x = lo[0]; x < hi[0]; ++x) {
          const int64_t at = x + y * stride[1]%(zterm)s;
#define A(...) cur[at + offset(stride, __VA_ARGS__)]
          dst[at] = static_cast<T>(%(expr)s);
#undef A
        }
    cur = dst;
  }
  for (int d = 0; d < D; ++d) {
    box[d] = lo[d];
    box[D + d] = hi[d];
  }
  std::free(spare[0]);
  std::free(spare[1]);
  return 0;
}
'''

_NEST_OFFSETS = '''
static inline int64_t offset(const int64_t* s, int dx, int dy) {
  return dx + dy * s[1];
}
static inline int64_t offset(const int64_t* s, int dx, int dy, int dz) {
  return dx + dy * s[1] + dz * s[2];
}
'''


def nest_source():
  out = [_NEST_HEAD, _NEST_OFFSETS]
  for (key, dim), (taps, expr) in sorted(NEST.items()):
    fn = 'nest_%s%dd' % (key, dim)
    out.append(_NEST_BODY % dict(
        what='%s, %d-D' % (key, dim), fn=fn, pad=' ' * (len(fn) + 10), dim=dim,
        taps=', '.join('{%s}' % ', '.join(map(str, tp)) for tp in taps),
        zterm=' + z * stride[2]' if dim == 3 else '', expr=expr))
    for t in (FLOATS if key == 'flt' else INTS):
      out.append('extern "C" int %s_%s(const void* in, void* out, '
                 'const int64_t* n, int iterate, int64_t* box) {\n'
                 '  return %s<%s>(static_cast<const %s*>(in), '
                 'static_cast<%s*>(out), n, iterate, box);\n}\n' % (
                     fn, t, fn, C_TYPE[t], C_TYPE[t], C_TYPE[t]))
  return '\n'.join(out)


_BUILD_DIR = None


@functools.lru_cache(maxsize=None)
def _nest_library():
  """Compiled as tests/fuzz_nest.py compiles its nests, with the C oracle's
  flags."""
  global _BUILD_DIR
  if _BUILD_DIR is None:
    _BUILD_DIR = tempfile.mkdtemp(prefix='soda_celltypes_')
  source = nest_source()
  key = hashlib.sha1(source.encode()).hexdigest()[:20]
  so = os.path.join(_BUILD_DIR, 'nest_%s.so' % key)
  src = os.path.join(_BUILD_DIR, 'nest_%s.cpp' % key)
  with open(src, 'w') as f:
    f.write(source)
  subprocess.run(['g++'] + NEST_FLAGS + ['-o', so, src], check=True,
                 capture_output=True)
  return ctypes.CDLL(so)


def nest_run(t, dim, kind, a, iterate=None):
  """(result shaped like `a`, (lo, hi) of the box the nest computed)."""
  a = np.ascontiguousarray(a)
  assert a.dtype == np.dtype(_np_name(t)) and a.ndim == dim
  fn = getattr(_nest_library(), 'nest_%s%dd_%s' % (expr_key(t, kind), dim, t))
  fn.restype = ctypes.c_int
  fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                 ctypes.POINTER(ctypes.c_int64), ctypes.c_int,
                 ctypes.POINTER(ctypes.c_int64)]
  out = np.empty_like(a)
  n = (ctypes.c_int64 * dim)(*a.shape[::-1])
  box = (ctypes.c_int64 * (2 * dim))()
  if fn(a.ctypes.data, out.ctypes.data, n, iterate or ITERATE[dim], box):
    raise MemoryError('nest: calloc failed')
  return out, (tuple(box[:dim]), tuple(box[dim:]))


def _np_name(t):
  return {'float': 'float32', 'double': 'float64'}.get(t, t)
