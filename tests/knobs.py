"""The options of the marching kernels (LowerOptions) as tests/test_knobs.py
sweeps them: the ledger of every option, the programs and their grids, the rows
-- every value alone, every admissible pair in a covering array -- and what it
means for a value to be in force.  tools/fuzz_scan.py draws its `options` scan
from the same value lists.

Nothing here needs a GPU; lowering needs neither the library nor a compiler."""
import functools
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SODA_DIRS = (os.path.join(ROOT, 'tests', 'golden', 'soda'),
             os.path.join(ROOT, 'tests', 'golden'))

# ---------------------------------------------------------------------------
# the ledger: every field of LowerOptions, one decision each
# ---------------------------------------------------------------------------

# option -> its values, the default FIRST.  `peel`: 'deepest' stands for the
# dict {deepest fusion depth of the program: 1}; `reg_budget`: 'lean' for the
# program's REG_BUDGET_LEAN.
SWEPT = {
    'lane_shift': (None, 'dpp', 'mixh'),
    'pipe': (None, 2, 4),
    'pipe_rows': (2, 1, 4, 8),
    'peel': (None, 0, 1, 'deepest'),
    'prefetch': (None, 1, 2, 4, 8),
    'waves_x': (1, 2),
    'waves_y': (1, 2, 4),
    'nt_store': (None, True, False),
    'nt_load': (None, True, False),
    'xcd_swizzle': (True, False),
    'edge_loads': (True, False),
    'align_lanes': (None, 2, 4, 8),
    'occupancy': (0, 1, 2),
    'min_waves': (0, 2, 3),
    'tile_rows': (None, 1, 2, 4),
    'vec': (None, 2, 1),
    'reg_budget': (None, 'lean'),
    'windows': (None, False),
    'inline': (None, False),
}

# option -> (the test file that owns it, the word that file knows it by)
ELSEWHERE = {
    'strategy': ('test_hip_parity.py', 'strategy'),
    'fuse': ('test_hip_parity.py', 'fuse'),
    'chunk_rows': ('test_hip_parity.py', 'chunk_rows'),
    'xshare': ('test_xshare_block.py', 'xshare'),
    'row_cells': ('test_xshare_block.py', 'row_cells'),
    'xshare_block': ('test_xshare_block.py', 'xshare_block'),
    'tile3d_w': ('test_tile3d.py', 'tile3d_w'),
    'tile3d_h': ('test_tile3d.py', 'tile3d_h'),
    'tile3d_waves': ('test_tile3d.py', 'tile3d_waves'),
    'banks': ('test_wire_banked.py', 'banks'),
    # (set by the stream layer from the reference host's delay, never by a
    # caller: the test named here runs a delayed input, `lead=4`)
    'bank_lead': ('test_wire_banked.py',
                  'test_misaligned_banks_take_the_copy_path'),
    'batch': ('test_batch.py', 'batch'),
    'residual': ('test_residual.py', 'residual'),
}

DIAGNOSTIC = {
    'stamps': 'tools/timeline.py alone sets it: the kernel then writes clock '
              'stamps through a sixteenth buffer no plain run supplies',
}

LEDGER = dict(
    [(o, ('swept', v)) for o, v in SWEPT.items()] +
    [(o, ('elsewhere',) + v) for o, v in ELSEWHERE.items()] +
    [(o, ('diagnostic', v)) for o, v in DIAGNOSTIC.items()])

# the value lists tools/fuzz_scan.py adds to its `options` scan
SCAN_VALUES = {o: SWEPT[o] for o in ('pipe_rows', 'align_lanes', 'occupancy',
                                     'min_waves', 'waves_x')}

# ---------------------------------------------------------------------------
# programs
# ---------------------------------------------------------------------------

_2D = ('lane_shift', 'pipe', 'pipe_rows', 'peel', 'prefetch', 'waves_x',
       'waves_y', 'nt_store', 'nt_load', 'xcd_swizzle', 'edge_loads',
       'align_lanes', 'occupancy', 'min_waves', 'vec', 'reg_budget')
# (one iteration: no fused kernel to pipeline, no warm-up worth peeling)
_2D_ONE = tuple(o for o in _2D if o not in ('pipe', 'pipe_rows', 'peel'))
# (a 3-D block is one wave whatever `waves_x` says: its only trace there is
# the kernel's name)
_3D = ('pipe', 'pipe_rows', 'peel', 'prefetch', 'nt_store', 'nt_load',
       'xcd_swizzle', 'edge_loads', 'align_lanes', 'occupancy', 'min_waves',
       'tile_rows', 'vec', 'reg_budget')

# name -> (program, stencil keywords, fixed LowerOptions, options swept, pairs?)
PROGRAMS = {
    'jacobi2d_T12': ('jacobi2d.soda', dict(iterate=13),
                     dict(fuse=(12,), chunk_rows=16), _2D, True),
    'jacobi2d_T4': ('jacobi2d.soda', dict(iterate=9),
                    dict(fuse=(4,), chunk_rows=16), _2D, True),
    'blur': ('blur.soda', dict(iterate=4),
             dict(fuse=(4,), chunk_rows=16), _2D, True),
    'coupled2d': ('coupled2d.soda', dict(iterate=4),
                  dict(fuse=(2,), chunk_rows=16), _2D, True),
    'ints2d': ('ints2d.soda', {}, dict(chunk_rows=16), _2D_ONE, True),
    'heat3d': ('heat3d.soda', dict(iterate=3),
               dict(fuse=(2,), chunk_rows=4), _3D, True),
    'erosion': ('erosion.soda', {}, dict(chunk_rows=16), ('windows',), False),
    'xcorr': ('xcorr.soda', {}, dict(chunk_rows=16), ('windows',), False),
    'denoise2d': ('denoise2d.soda', {}, dict(chunk_rows=16), ('inline',),
                  False),
}

# estimated registers (LowerOptions.reg_budget) at which the shape ladder of
# lower() leaves the default shape of the one-iteration kernel for a leaner
# one: below the estimate of the default shape, chosen from the ladder's own
# estimates (`est_window_regs`; tests/test_knobs.py asserts that the shape
# moves)
REG_BUDGET_LEAN = {'jacobi2d_T12': 40, 'jacobi2d_T4': 40, 'blur': 40,
                   'coupled2d': 80, 'ints2d': 24, 'heat3d': 100}

# trips of the warm-up peeled where a row leaves `peel` alone: none, what
# resolve_options answers without trial compilations -- but one in 3-D.  On
# chunks of 4 planes the unpeeled two-iteration kernel of heat3d computes 8
# plane steps for 4: more than twice the one-iteration kernel's time in the
# launch-time model (9.94 against 2 x 4.83 us) and on the clock (12.98
# against 2 x 6.22 us), so no run would schedule it; with its one trip peeled
# the model prices it at 7.18 against 2 x 4.08 us.
PEEL_PIN = {'heat3d': 1}
# ... which leaves the rows that take the trip back, `peel=0` and `prefetch=2`
# (two planes in flight leave no trip worth peeling: 9.94 against 2 x 4.08
# us).  Alone, their GPU case would test the one-iteration kernel only, and
# longer chunks make the model's verdict worse (13.6 against 2 x 5.6 us at 8
# planes).  So these two values run on the GPU, whatever the budget, with two
# cells per lane beside them (HELD: the model then prices the unpipelined
# fused kernel at 4.91 / 6.31 against 2 x 3.36 / 3.74 us); the rows without
# the companion are lowered, checked and compiled.  tests/test_knobs.py holds
# the list exact both ways against the model, which is deterministic.
UNSCHEDULED = {('heat3d', (('peel', 0),)), ('heat3d', (('prefetch', 2),))}
UNSCHEDULED_COMPANION = {'vec': 2}
# single rows that leave the deepest kernel as the default row has it (the
# key of NO_EFFECT in_force answers with): lowered, checked and compiled, not
# run on the GPU alone.  Exact both ways (tests/test_knobs.py).  `pipe_rows`
# runs with `pipe=2` beside it instead (HELD)
NO_EFFECT_ALONE = {
    'jacobi2d_T12': [('pipe_rows', 1), ('pipe_rows', 4), ('pipe_rows', 8),
                     ('edge_loads', False), ('align_lanes', 2),
                     ('align_lanes', 4), ('align_lanes', 8)],
    'jacobi2d_T4': [('pipe_rows', 1), ('pipe_rows', 4), ('pipe_rows', 8),
                    ('edge_loads', False), ('align_lanes', 2)],
    'blur': [('pipe_rows', 1), ('pipe_rows', 4), ('pipe_rows', 8),
             ('edge_loads', False)],
    'coupled2d': [('pipe_rows', 1), ('pipe_rows', 4), ('pipe_rows', 8),
                  ('edge_loads', False), ('align_lanes', 2)],
    'ints2d': [('edge_loads', False), ('align_lanes', 2)],
    'heat3d': [('pipe_rows', 1), ('pipe_rows', 4), ('pipe_rows', 8),
               ('edge_loads', False), ('align_lanes', 2)],
}

SEED = 77
RAGGED = {2: 5, 3: 2}       # rows / planes of the last chunk


def soda_path(name):
  for d in SODA_DIRS:
    if os.path.exists(os.path.join(d, name)):
      return os.path.join(d, name)
  raise FileNotFoundError(name)


@functools.lru_cache(maxsize=None)
def stencil_of(prog):
  from soda_amd import core
  soda, skw = PROGRAMS[prog][:2]
  return core.from_file(soda_path(soda), **skw)


def deepest_depth(prog):
  st = stencil_of(prog)
  fuse = PROGRAMS[prog][2].get('fuse', ())
  return max([min(t, st.iterate) for t in fuse] + [1])


def options_of(prog):
  return PROGRAMS[prog][3]


def values_of(prog, option):
  return SWEPT[option]


def keywords(prog, row):
  """LowerOptions keywords of a row ({option: value}, defaults left out).
  `peel=None` lets runtime.select_peel choose from trial compilations, several
  a kernel: the default row alone pays for them -- and runs what they choose
  -- every other row that leaves `peel` alone takes PEEL_PIN."""
  kw = dict(PROGRAMS[prog][2])
  if row and 'peel' not in row:
    kw['peel'] = PEEL_PIN.get(prog, 0)
  for o, v in row.items():
    if o == 'peel' and v == 'deepest':
      v = {deepest_depth(prog): 1}
    if o == 'reg_budget' and v == 'lean':
      v = REG_BUDGET_LEAN[prog]
    kw[o] = v
  return kw


def row_id(row):
  def text(v):
    return str(v).replace(' ', '')
  return '+'.join('%s=%s' % (o, text(row[o])) for o in sorted(row)) or 'default'


def freeze(row):
  return tuple(sorted(row.items(), key=lambda kv: kv[0]))


# ---------------------------------------------------------------------------
# lowering a row
# ---------------------------------------------------------------------------

NOT_BUILT = 'fused kernel not built'
FALLBACK = 'pipe falls back to one wave'


class Refused(Exception):
  """A row that lower() refuses or answers without its fused kernel."""


def deepest(mod):
  return max((k for k in mod.kernels if k.tune and 'fused' in k.tune),
             key=lambda k: k.tune['fused'])


def _lower(prog, kw, extent, probe=False):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  st = stencil_of(prog)
  opts = runtime.resolve_options(st, lower.LowerOptions(**kw), extent,
                                 probe=probe)
  return lower.lower(st, opts)


@functools.lru_cache(maxsize=None)
def _lowered(prog, frozen, extent=None, probe=False):
  """The module of a row, or Refused with the reason: the SemanticError's
  text, or `fused kernel not built` where the ladder dropped the depth."""
  from soda_amd import util
  try:
    mod = _lower(prog, keywords(prog, dict(frozen)), extent, probe)
  except util.SemanticError as e:
    raise Refused(str(e))
  if deepest(mod).tune['fused'] != deepest_depth(prog):
    raise Refused(NOT_BUILT)
  return mod


def lowered(prog, row, extent=None, probe=False):
  return _lowered(prog, freeze(row), extent, probe)


def _grid(k):
  """2 S + 9 V cells along x; 9 rows in 3-D; the marched dimension comes from
  the launch geometry (extent_of)."""
  s, v = k.tile[0], k.tune['vec']
  return 2 * s + 9 * v


def _rows_for(k, dim):
  """Seven chunks and a ragged one of the deepest kernel's blocks: with three
  tiles along x (and three along y in 3-D) the block count is 24 or 72, a
  multiple of 8, which is when the XCD renumbering of a kernel is live."""
  return 7 * k.tile[dim - 1] + RAGGED[dim]


def settle(dim, lower_for, what, width=None, pick=None):
  """(extent, extent to build the program for or None) of the module
  `lower_for(extent or None)` answers with: the grid of its deepest kernel.
  `width(kernel)`: the cells along x, where they are not 2 S + 9 V;
  `pick(module)`: the kernel the grid is sized from, where `deepest` does not
  find it."""
  pick = pick or deepest
  mod = lower_for(None)
  k = pick(mod)

  def grid(k):
    x = width(k) if width else _grid(k)
    return (x, _rows_for(k, 2)) if dim == 2 else (x, 9, _rows_for(k, 3))

  extent = grid(k)
  widest = max(q.tune.get('vec', 1) for q in mod.kernels if q.tune)
  if extent[0] % widest == 0:
    return extent, None
  # the vector width follows the row length, the row length the width
  for _ in range(4):
    k = pick(lower_for(extent))
    new = grid(k)
    if new == extent:
      return extent, extent
    extent = new
  raise AssertionError('%s: no stable grid' % (what,))


@functools.lru_cache(maxsize=None)
def _setup(prog, frozen, probe=False):
  row = dict(frozen)
  return settle(stencil_of(prog).dim,
                lambda extent: lowered(prog, row, extent, probe),
                '%s %s' % (prog, row_id(row)))


def setup(prog, row, probe=False):
  """(extent, extent to build the program for or None) of a row: the grid of
  the deepest kernel of the module the row builds."""
  return _setup(prog, freeze(row), probe)


def module_for(prog, row, probe=False):
  extent, build_for = setup(prog, row, probe)
  return lowered(prog, row, build_for, probe), extent


# ---------------------------------------------------------------------------
# is a value in force?
# ---------------------------------------------------------------------------

# why a value may leave a kernel as it would be without it
NO_EFFECT = {
    'pipe_rows': 'no stage-pipelined block to count row steps for',
    'peel': 'a stage-pipelined block has no peeled warm-up, a short warm-up '
            'no trip to peel',
    'edge_loads': 'edge loads are there only where they save a halo lane',
    'align_lanes': 'no spare lane to give up: the strip is a multiple already, '
                   'a 32-lane half strip, or its halo is 16 lanes or more',
    'reg_budget': 'the caller fixed the shape the ladder would change',
    'vec': 'the shape ladder retreats to fewer cells per lane',
}


def _one(mod):
  return [k for k in mod.kernels if k.tune and k.tune.get('fused') == 1
          and 'axis' in k.tune][-1]


def _prefetch_of(k):
  return int(k.name.split('_P')[1].split('_')[0])


def _pass_of(mod, k):
  return [p for p in mod.passes if mod.kernels[p.kernels[0]] is k][0]


def in_force(prog, row, option, mod=None):
  """True if `option`'s value of `row` shapes the deepest kernel of the row's
  module (for `reg_budget`: the one-iteration kernel): the kernel's name
  carries the value's tag and its descriptor agrees.  A key of NO_EFFECT
  where the generator legitimately answers without the value.  Anything else
  -- a tag without the descriptor, a descriptor without the tag -- is an
  AssertionError."""
  st = stencil_of(prog)
  mod = mod or lowered(prog, row)
  k = deepest(mod)
  name, tune = k.name, k.tune
  v = row[option]
  without = {o: w for o, w in row.items() if o != option}

  def agree(tagged, described, what):
    assert bool(tagged) == bool(described), \
        '%s %s: %s: name %s, descriptor %s' % (prog, row_id(row), what, name,
                                               tune)
    return bool(tagged)

  if option == 'lane_shift':
    assert agree('_mixh' in name, tune['lane_shift'] == 'mixh', 'mixh') == \
        (v == 'mixh'), (name, v)
    return True
  if option == 'pipe':
    on = agree('_pipe%dx' % v in name,
               tune['pipe'] == v and tune['waves_per_block'] == v, 'pipe')
    assert on or (tune['pipe'] == 1 and '_pipe' not in name), name
    return on or FALLBACK
  if option == 'pipe_rows':
    if tune['pipe'] == 1:
      assert '_pipe' not in name, name
      return 'pipe_rows'
    assert '_pipe%dx%d_' % (tune['pipe'], v) in name + '_', name
    assert tune['lds_rings'] % (2 * v) == 0 and tune['unroll'] % v == 0, tune
    return True
  if option == 'peel':
    if v is None:
      return True
    trips = 1 if v == 'deepest' else v
    assert '_k%d' % trips in name, name
    assert tune['peel_trips'] == min(trips, tune['peel_trips_max']), tune
    return True if tune['peel_trips'] == trips else 'peel'
  if option == 'prefetch':
    assert _prefetch_of(k) == v, name
    return True
  if option in ('waves_x', 'waves_y'):
    wx, wy = row.get('waves_x', 1), row.get('waves_y', 1)
    assert st.dim == 2 and '_W%dx%d_' % (wx, wy) in name, name
    assert tune['waves_per_block'] == wx * wy or tune['pipe'] > 1, tune
    assert tune['waves_along'] == wy, tune
    assert k.tile[1] == wy * PROGRAMS[prog][2]['chunk_rows'], k.tile
    return True
  if option in ('nt_store', 'nt_load', 'xcd_swizzle'):
    tag = {'nt_store': '_nts', 'nt_load': '_ntl', 'xcd_swizzle': '_xcd'}[option]
    assert (tag in name) == bool(v), name
    return True
  if option == 'edge_loads':
    assert '_edge' not in name, name
    assert tuple(_pass_of(mod, k).traffic_model['edge']) == (0, 0)
    other = lowered(prog, without)
    edge = _pass_of(other, deepest(other)).traffic_model['edge']
    return True if tuple(edge) != (0, 0) else 'edge_loads'
  if option == 'align_lanes':
    assert '_al%d' % v in name, name
    plain = deepest(lowered(prog, dict(without, align_lanes=1)))
    if k.tile[0] == plain.tile[0]:
      return 'align_lanes'
    per_wave = k.tile[0] // tune['vec']
    if tune['pipe'] == 1:
      per_wave //= row.get('waves_x', 1)
    assert per_wave % v == 0 and plain.tile[0] - k.tile[0] < v * tune['vec'] \
        * row.get('waves_x', 1), (k.tile, plain.tile)
    return True
  if option == 'occupancy':
    assert '_occ%d' % v in name and tune['occupancy'] == v, name
    assert k.lds_bytes == tune['lds_pad'], tune
    assert 1024 <= k.lds_bytes + tune['lds_rings'] <= \
        max(81 * 1024, tune['lds_rings']) and k.lds_bytes <= 65536, tune
    return True
  if option == 'min_waves':
    assert '_mw%d' % v in name, name
    assert 'amdgpu_waves_per_eu(%d, 8))) %s(' % (v, name) in mod.source
    return True
  if option == 'tile_rows':
    assert st.dim == 3 and '_R%d_' % v in name, name
    assert tune['tile_rows'] == v == k.tile[1], tune
    return True
  if option == 'vec':
    assert '_V%d_' % tune['vec'] in name and tune['vec'] <= v, name
    return True if tune['vec'] == v else 'vec'
  if option == 'reg_budget':
    a, b = _one(mod), _one(lowered(prog, without))
    moved = (a.tune['vec'], _prefetch_of(a)) != (b.tune['vec'],
                                                 _prefetch_of(b))
    return True if moved else 'reg_budget'
  if option in ('windows', 'inline'):
    assert mod.source != lowered(prog, without).source
    return True
  raise KeyError(option)


def marks(prog, row, mod=None):
  """{option: True or the NO_EFFECT key} of a row that lowers."""
  mod = mod or lowered(prog, row)
  return {o: in_force(prog, row, o, mod) for o in sorted(row)}


def status(prog, row):
  """None if the row lowers with every value in force; the refusal (the
  SemanticError's text, NOT_BUILT, FALLBACK); or `ignored: <options>`."""
  try:
    m = marks(prog, row)
  except Refused as e:
    return str(e)
  if FALLBACK in m.values():
    return FALLBACK
  idle = [o for o in sorted(m) if m[o] is not True]
  return 'ignored: ' + ', '.join(idle) if idle else None


def refused(status_):
  return status_ is not None and not status_.startswith('ignored: ')


# ---------------------------------------------------------------------------
# pairs that cannot be: (programs or ANY, option, values, option or ANY,
# values, reason).  The reason is the start of the SemanticError's text,
# NOT_BUILT where the ladder of lower() drops the fused depth, or FALLBACK
# where `pipe` quietly becomes one wave (documented: lower.pipe_for).  A rule
# whose second option is ANY refuses the value alone, hence with everything.
# tests/test_knobs.py holds the table exact both ways.
# ---------------------------------------------------------------------------

ANY = None
ALONE = 'alone'        # the value with every other option at its default
INADMISSIBLE = [
    # stage-pipelined blocks are one strip and one chunk per block
    (ANY, 'pipe', (2, 4), 'waves_x', (2,), FALLBACK),
    (ANY, 'pipe', (2, 4), 'waves_y', (2, 4), FALLBACK),
    (ANY, 'pipe_rows', (1, 4, 8), 'waves_x', (2,), FALLBACK),
    (ANY, 'pipe_rows', (1, 4, 8), 'waves_y', (2, 4), FALLBACK),
    # four waves do not divide two fused iterations
    (('coupled2d', 'heat3d'), 'pipe', (4,), ANY, (), FALLBACK),
]
# twelve iterations at one cell per lane are a halo of 12 + 12 lanes: too wide
# for the 32-lane half strips of `mixh`, the default at that depth.  Whatever
# brings DPP shifts and whole strips with it builds the kernel
_DPP = ('lane_shift', 'pipe', 'pipe_rows', 'waves_x', 'waves_y')
INADMISSIBLE += [(('jacobi2d_T12',), 'vec', (1,), ALONE, (), NOT_BUILT),
                 (('jacobi2d_T12',), 'vec', (1,), 'lane_shift', ('mixh',),
                  NOT_BUILT)]
INADMISSIBLE += [(('jacobi2d_T12',), 'vec', (1,), o, SWEPT[o][1:], NOT_BUILT)
                 for o in _2D if o != 'vec' and o not in _DPP]


def inadmissible(prog, a, av, b=None, bv=None):
  """The reason the table gives for a value (alone) or a pair, or None."""
  for progs, o1, v1, o2, v2, reason in INADMISSIBLE:
    if progs is not ANY and prog not in progs:
      continue
    if o2 is ANY:
      if (o1 == a and av in v1) or (o1 == b and bv in v1):
        return reason
    elif o2 == ALONE:
      if b is None and o1 == a and av in v1:
        return reason
    elif (o1 == a and av in v1 and o2 == b and bv in v2) or \
        (o1 == b and bv in v1 and o2 == a and av in v2):
      return reason
  return None


def alone(prog):
  """[(option, value)] beside the defaults, in ledger order."""
  return [(o, v) for o in options_of(prog) for v in SWEPT[o][1:]]


def pairs(prog):
  """Every pair of non-default values of two different options."""
  if not PROGRAMS[prog][4]:
    return
  for a, b in itertools.combinations(options_of(prog), 2):
    for av in SWEPT[a][1:]:
      for bv in SWEPT[b][1:]:
        yield a, av, b, bv


def context(a, av, b, bv):
  """The smallest row that can hold the pair: `pipe_rows` counts the row
  steps of a stage-pipelined block, so it comes with one."""
  row = {a: av, b: bv}
  if 'pipe_rows' in row and 'pipe' not in row:
    row['pipe'] = 2
  return row


# ---------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------

def single_rows(prog):
  """The default row, then every value alone (those the table refuses alone
  left out)."""
  return [{}] + [{o: v} for o, v in alone(prog)
                 if inadmissible(prog, o, v) is None]


def held_rows(prog):
  """A value that cannot show alone, with the one companion that lets it:
  `pipe_rows` with `pipe=2`, the UNSCHEDULED values with theirs.  Never scaled
  by the budget."""
  out = []
  for o, v in alone(prog):
    if inadmissible(prog, o, v) is not None:
      continue
    if o == 'pipe_rows':
      out.append({'pipe': 2, 'pipe_rows': v})
    elif (prog, ((o, v),)) in UNSCHEDULED:
      out.append(dict(UNSCHEDULED_COMPANION, **{o: v}))
  return out


def runs_alone(prog, row):
  """Is a single row worth a GPU case of its own?"""
  (o, v), = row.items() or [(None, None)]
  return (o, v) not in NO_EFFECT_ALONE.get(prog, ()) and \
      (prog, freeze(row)) not in UNSCHEDULED


@functools.lru_cache(maxsize=None)
def _pair_rows(prog):
  """A covering array, greedy and seeded: every pair of non-default values
  that can be in force together (its `context` row lowers with both in force)
  stands, both in force, in some row.  A row grows from the first uncovered
  pair by the values that cover most of what is left -- ties by a seeded draw,
  the table consulted, nothing lowered -- and is then lowered once: whatever is
  refused or without effect there is taken out again, last added first."""
  rng = np.random.default_rng(SEED + sum(map(ord, prog)))
  todo = [p for p in pairs(prog) if inadmissible(prog, *p) is None]
  left = set(todo)
  rows = []
  opts = options_of(prog)

  def gain(row, o, v):
    return sum(1 for q, w in row.items()
               if (q, w, o, v) in left or (o, v, q, w) in left)

  def fits(row, o, v):
    if o == 'pipe_rows' and 'pipe' not in row:
      return False
    return all(inadmissible(prog, q, w, o, v) is None for q, w in row.items())

  for first in todo:
    if first not in left:
      continue
    left.discard(first)
    row = context(*first)
    if status(prog, row) is not None:
      continue          # cannot be in force together: nothing to cover
    added = []
    order = [o for o in opts if o not in row]
    rng.shuffle(order)
    for o in order:
      cands = [(gain(row, o, v), float(rng.random()), v) for v in SWEPT[o][1:]
               if inadmissible(prog, o, v) is None and fits(row, o, v)]
      cands = sorted((c for c in cands if c[0] > 0), key=lambda c: c[:2])
      if cands:
        row[o] = cands[-1][2]
        added.append(o)
    while added and status(prog, row) is not None:
      s = status(prog, row)
      idle = s[len('ignored: '):].split(', ') if not refused(s) else []
      drop = [o for o in added if o in idle] or added
      del row[drop[-1]]
      added.remove(drop[-1])
    assert status(prog, row) is None, (prog, row, status(prog, row))
    for (o1, v1), (o2, v2) in itertools.combinations(sorted(row.items()), 2):
      left.discard((o1, v1, o2, v2))
      left.discard((o2, v2, o1, v1))
    rows.append(row)
  return tuple(freeze(r) for r in rows)


def pair_rows(prog):
  return [dict(r) for r in _pair_rows(prog)]


# pair rows of every program (tests/test_knobs.py asserts the numbers): what
# lets the GPU cases be listed without lowering anything
PAIR_ROWS = {'jacobi2d_T12': 49, 'jacobi2d_T4': 41, 'blur': 54, 'coupled2d': 36,
             'ints2d': 22, 'heat3d': 38}
# share of the pair rows a run takes at --fuzz-budget 1
PAIR_SHARE = 0.25


def pair_picks(prog, budget):
  """Indices into pair_rows(prog) a run at `budget` takes: evenly spread,
  PAIR_SHARE of them at 1, all from 1 / PAIR_SHARE on, none at 0.  The single
  rows are never scaled."""
  total = PAIR_ROWS.get(prog, 0)
  n = min(total, int(round(total * PAIR_SHARE * max(0.0, budget))))
  return [int(i * total / float(n)) for i in range(n)]
