"""The marching kernels under every lowering option, alone and in pairs.

LowerOptions has some twenty options that change the text of `march2d` /
`march3d`; the rest of the suite pins the defaults.  Here (tests/knobs.py holds
the tables and the rows):

* a ledger names every field of LowerOptions: swept here, owned by another
  test file, or diagnostic;
* for six programs every value of every swept option runs alone -- or, where
  it cannot show alone, with its one companion (knobs.held_rows) -- and a
  seeded covering array holds every pair of values that can be in force
  together, all of it checked and compiled on the CPU at any budget;
  the pairs that cannot be stand in a table that is exact both ways;
* every row must take effect: the deepest kernel's name carries the row's tags
  and its descriptor agrees, or the row says why the generator ignores it;
* every row compiles for gfx950 without a GPU;
* on the GPU every row runs the device entry between guard bands
  (tests/guarded.py) on signed / full-range cells against the single-threaded C
  oracle: no byte outside the outputs, the valid box bit for bit.

Grids, as in tests/test_device_entry.py, from the deepest kernel of the module
a row builds: 2 S + 9 V cells along x, seven chunks of 16 rows (4 planes) and
a ragged one, 9 rows in 3-D.  Three tiles along x times eight chunks: the
block count is a multiple of 8, the one situation in which a kernel's XCD
renumbering is live.

What the rows are sized to catch (reasoned from the shapes, never run): the
mirrors of a stage-pipelined block read a ring slot R = `pipe_rows` ticks
after it was written, of a ring of 2 R slots indexed by t mod 2 R.  With R
slots where 2 R are meant, tick t + R of the writer lands on the very slot
the reader takes at that tick, within one barrier period -- for EVERY R, the
default 2 included, since R mod R = 0 whatever R is.  So every row with a
pipelined block is exposed: the single rows `pipe=2` and `pipe=4` (R = 2),
the held rows `pipe=2+pipe_rows=1|4|8` of every fused program, and the pair
rows with `pipe`; on 117 rows in chunks of 16 each of them runs dozens of
barrier periods per block.  An off-by-one in the spare lanes of `align_lanes`
moves the strip seam by V cells while the host tiles by the descriptor's
strip: the rows `align_lanes=4`, `align_lanes=8` (jacobi2d T4: 62 -> 60 / 56
lanes; blur: 63 -> 62 / 60 / 56 with `align_lanes=2` as well) and `nt_store=
True`, whose derived value takes the same path, then leave a column of V
cells per strip seam unwritten (0xA5 fill) or written twice from a halo lane
-- both strips are on the grid, 2 S + 9 V."""
import dataclasses
import functools
import os

import numpy as np
import pytest

import fuzz
import knobs
import test_device_entry as tde

PROGS = sorted(knobs.PROGRAMS)
PAIRED = [p for p in PROGS if knobs.PROGRAMS[p][4]]

# every row there is, for the CPU: the single rows, the held rows (a value
# with the one companion that lets it show) and the WHOLE covering array,
# whatever the budget
RUN_CPU = [(p, 'alone', i) for p in PROGS
           for i in range(len(knobs.single_rows(p)))] + \
          [(p, 'held', i) for p in PROGS
           for i in range(len(knobs.held_rows(p)))] + \
          [(p, 'pair', j) for p in PAIRED for j in range(knobs.PAIR_ROWS[p])]
# the GPU runs: the single rows that take effect and are scheduled, the held
# rows, then the pair rows the budget takes -- the first failure names one
# option
RUN_GPU = [r for r in RUN_CPU if r[1] == 'held' or
           (r[1] == 'alone' and
            knobs.runs_alone(r[0], knobs.single_rows(r[0])[r[2]]))] + \
          [(p, 'pair', j) for p in PAIRED
           for j in knobs.pair_picks(p, fuzz.budget())]


def _row(p, kind, i):
  return {'alone': knobs.single_rows, 'held': knobs.held_rows,
          'pair': knobs.pair_rows}[kind](p)[i]


def _run_id(run):
  p, kind, i = run
  if kind == 'pair':
    return '%s-pair%d' % (p, i)
  return '%s-%s' % (p, knobs.row_id(_row(p, kind, i)))


# ---------------------------------------------------------------------------
# CPU: the ledger
# ---------------------------------------------------------------------------

# the values asked for, spelled out once more: a value deleted from the ledger
# (tests/knobs.py SWEPT) fails here
ASKED = {
    'lane_shift': {None, 'dpp', 'mixh'}, 'pipe': {None, 2, 4},
    'pipe_rows': {1, 2, 4, 8}, 'peel': {None, 0, 1, 'deepest'},
    'prefetch': {None, 1, 2, 4, 8}, 'waves_x': {1, 2}, 'waves_y': {1, 2, 4},
    'nt_store': {None, True, False}, 'nt_load': {None, True, False},
    'xcd_swizzle': {True, False}, 'edge_loads': {True, False},
    'align_lanes': {None, 2, 4, 8}, 'occupancy': {0, 1, 2},
    'min_waves': {0, 2, 3}, 'tile_rows': {None, 1, 2, 4}, 'vec': {None, 2, 1},
    'reg_budget': {None, 'lean'}, 'windows': {None, False},
    'inline': {None, False},
}


def _fields():
  from soda_amd.codegen.hip import lower
  return {f.name: f for f in dataclasses.fields(lower.LowerOptions)}


def test_the_ledger_names_every_option():
  """A new field of LowerOptions cannot arrive without a decision."""
  assert set(knobs.LEDGER) == set(_fields())
  assert len(knobs.LEDGER) == len(knobs.SWEPT) + len(knobs.ELSEWHERE) + \
      len(knobs.DIAGNOSTIC)
  assert set(knobs.ELSEWHERE) == {
      'strategy', 'fuse', 'chunk_rows', 'xshare', 'row_cells', 'xshare_block',
      'tile3d_w', 'tile3d_h', 'tile3d_waves', 'banks', 'bank_lead', 'batch',
      'residual'}
  assert set(knobs.DIAGNOSTIC) == {'stamps'}
  assert all(why.strip() for why in knobs.DIAGNOSTIC.values())


def test_the_swept_values_are_those_asked_for():
  assert set(knobs.SWEPT) == set(ASKED)
  fields = _fields()
  for o, values in knobs.SWEPT.items():
    assert len(values) == len(set(values)) and set(values) == ASKED[o], o
    # the default comes first, and is the dataclass's
    assert values[0] == fields[o].default and \
        type(values[0]) is type(fields[o].default), o
  # ... and every one is swept on some program
  swept = {o for p in PROGS for o in knobs.options_of(p)}
  assert swept == set(knobs.SWEPT)
  assert knobs.SCAN_VALUES == {o: knobs.SWEPT[o] for o in (
      'pipe_rows', 'align_lanes', 'occupancy', 'min_waves', 'waves_x')}


@pytest.mark.parametrize('option', sorted(knobs.ELSEWHERE))
def test_options_covered_elsewhere_are(option):
  name, word = knobs.ELSEWHERE[option]
  path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
  assert os.path.isfile(path), path
  with open(path) as f:
    text = f.read()
  import re
  assert re.search(r'\b%s\b' % re.escape(word), text), (name, word)
  assert '@pytest.mark.gpu' in text


# ---------------------------------------------------------------------------
# CPU: the rows
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('prog', PROGS)
def test_every_value_stands_alone(built, prog):
  """Each value in a row that differs from the default in that option only,
  or refused alone by the table -- which a lowering confirms either way."""
  rows = knobs.single_rows(prog)
  assert rows[0] == {} and knobs.status(prog, {}) is None
  for o, v in knobs.alone(prog):
    s = knobs.status(prog, {o: v})
    why = knobs.inadmissible(prog, o, v)
    if why is None:
      assert {o: v} in rows and not knobs.refused(s), (o, v, s)
    else:
      assert {o: v} not in rows and s is not None and s.startswith(why), \
          (o, v, s, why)
  assert len(rows) == len({knobs.freeze(r) for r in rows})


@pytest.mark.parametrize('prog', PAIRED)
def test_the_table_of_inadmissible_pairs_is_exact(built, prog):
  """A pair the table lists is refused, with the text it names; a pair it
  does not list lowers, fused kernel and all."""
  n = 0
  for pair in knobs.pairs(prog):
    n += 1
    s = knobs.status(prog, knobs.context(*pair))
    why = knobs.inadmissible(prog, *pair)
    if why is None:
      assert not knobs.refused(s), 'unlisted, refused: %s: %s' % (pair, s)
    else:
      assert knobs.refused(s) and s.startswith(why), \
          'listed as `%s`: %s: %s' % (why, pair, s)
  assert n > 200
  # every rule is about this suite's options and values
  for progs, a, av, b, bv, why in knobs.INADMISSIBLE:
    assert progs is knobs.ANY or set(progs) <= set(PAIRED)
    assert set(av) <= set(knobs.SWEPT[a][1:])
    assert b in (knobs.ANY, knobs.ALONE) or set(bv) <= set(knobs.SWEPT[b][1:])
    assert why in (knobs.NOT_BUILT, knobs.FALLBACK) or why.startswith('march')


@pytest.mark.parametrize('prog', PAIRED)
def test_every_admissible_pair_is_in_a_row(built, prog):
  """Both values in force in one row, for every pair that can be: whose
  smallest row lowers with both in force."""
  rows = knobs.pair_rows(prog)
  assert len(rows) == knobs.PAIR_ROWS[prog]
  assert rows == knobs.pair_rows(prog) and \
      [knobs.freeze(r) for r in rows] == list(knobs._pair_rows.__wrapped__(prog))
  held = set()
  for row in rows:
    assert knobs.status(prog, row) is None, (row, knobs.status(prog, row))
    items = sorted(row.items())
    held |= {(a, b) for a in items for b in items if a[0] != b[0]}
  missing = [p for p in knobs.pairs(prog)
             if knobs.status(prog, knobs.context(*p)) is None and
             ((p[0], p[1]), (p[2], p[3])) not in held]
  assert not missing, missing[:8]
  # the budget never scales below the single rows, and reaches every pair row
  assert knobs.pair_picks(prog, 0) == []
  assert knobs.pair_picks(prog, 1 / knobs.PAIR_SHARE) == list(range(len(rows)))
  picks = knobs.pair_picks(prog, 1)
  assert len(set(picks)) == len(picks) == round(len(rows) * knobs.PAIR_SHARE)


@pytest.mark.parametrize('prog', PROGS)
def test_every_row_takes_effect_or_says_why_not(built, prog):
  """knobs.in_force asserts tag and descriptor of every value; what is left
  without effect is one of the generator's documented reasons."""
  deepest = knobs.deepest_depth(prog)
  idle = []
  for row in knobs.single_rows(prog) + knobs.held_rows(prog) + \
      knobs.pair_rows(prog):
    mod = knobs.lowered(prog, row)
    k = knobs.deepest(mod)
    assert k.tune['fused'] == deepest and '_T%d_' % deepest in k.name
    for o, mark in knobs.marks(prog, row, mod).items():
      assert mark is True or (len(row) == 1 and mark in knobs.NO_EFFECT), \
          (row, o, mark)
      if mark is not True:
        idle.append((o, row[o]))
  # the single rows left out of the GPU run are those without effect, exactly
  assert sorted(idle, key=str) == \
      sorted(knobs.NO_EFFECT_ALONE.get(prog, []), key=str)
  for row in knobs.held_rows(prog):
    assert len(row) == 2 and knobs.status(prog, row) is None, row
  held = {o for row in knobs.held_rows(prog) for o in row}
  assert all((o, v) in [(q, w) for r in knobs.held_rows(prog)
                        for q, w in r.items()]
             for o, v in knobs.NO_EFFECT_ALONE.get(prog, [])
             if o == 'pipe_rows'), held


def test_every_value_is_in_force_somewhere(built):
  seen = set()
  for prog in PROGS:
    for row in knobs.single_rows(prog) + knobs.held_rows(prog) + \
        knobs.pair_rows(prog):
      seen |= {(o, row[o]) for o, mark in knobs.marks(prog, row).items()
               if mark is True}
  want = {(o, v) for o, values in knobs.SWEPT.items() for v in values[1:]}
  assert want <= seen, sorted(want - seen, key=str)
  # the defaults: in force in every default row, by definition of the default


@pytest.mark.parametrize('prog', sorted(knobs.REG_BUDGET_LEAN))
def test_a_lean_register_budget_moves_the_ladder(built, prog):
  plain = knobs._one(knobs.lowered(prog, {}))
  lean = knobs._one(knobs.lowered(prog, {'reg_budget': 'lean'}))
  assert (lean.tune['vec'], knobs._prefetch_of(lean)) != \
      (plain.tune['vec'], knobs._prefetch_of(plain)), (plain.name, lean.name)
  assert lean.tune['vec'] <= plain.tune['vec'] and \
      knobs._prefetch_of(lean) <= knobs._prefetch_of(plain)


# ---------------------------------------------------------------------------
# CPU: the two refusals
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('strategy', ['auto', 'march', 'direct', 'tile3d'])
def test_pipe_rows_must_be_a_power_of_two(built, strategy):
  """Refused by name where the module is built, whatever the strategy -- not
  answered with the one-iteration kernel alone."""
  from soda_amd import util
  from soda_amd.codegen.hip import lower
  prog = 'heat3d' if strategy == 'tile3d' else 'jacobi2d_T4'
  st = knobs.stencil_of(prog)
  for rows in (3, 6, 0, -2):
    with pytest.raises(util.SemanticError) as err:
      lower.lower(st, lower.LowerOptions(strategy=strategy, fuse=(4,), pipe=4,
                                         pipe_rows=rows))
    assert 'pipe_rows' in str(err.value) and 'power of two' in str(err.value)
  # without pipelined blocks the option is not looked at
  mod = lower.lower(st, lower.LowerOptions(strategy=strategy, fuse=(2,),
                                           pipe_rows=3))
  assert mod.kernels


def test_a_pipe_that_does_not_divide_the_depth_is_one_wave(built):
  """The documented fallback: the fused kernel is built, by one wave."""
  from soda_amd.codegen.hip import lower
  st = knobs.stencil_of('jacobi2d_T4')
  for fuse, pipe, want in (((4,), 4, 4), ((4,), 2, 2), ((3,), 2, 1),
                           ((6,), 4, 1), ((6,), 2, 2)):
    mod = lower.lower(st, lower.LowerOptions(fuse=fuse, pipe=pipe))
    k = knobs.deepest(mod)
    assert k.tune['fused'] == fuse[0] and k.tune['pipe'] == want, k.name
    assert ('_pipe' in k.name) == (want > 1)


def test_the_occupancy_pad_counts_the_rings(built):
  """The dynamic LDS of `occupancy` is what is missing beside the rings a
  stage-pipelined block declares itself, up to the allocation of which one
  block more no longer fits a CU (81 KiB for one block): never a 64 KiB pad on
  top of the rings.  (An MI355X accepted 64 KiB dynamic beside 24 KiB static
  and computed the right bits; 160 KiB a block is the limit.)"""
  seen = 0
  for prog in PAIRED:
    for row in knobs.single_rows(prog) + knobs.pair_rows(prog):
      if not row.get('occupancy'):
        continue
      for k in knobs.lowered(prog, row).kernels:
        static, pad = k.tune['lds_rings'], k.tune['lds_pad']
        assert k.lds_bytes == pad >= 0
        assert static + pad <= max(81 * 1024, static) <= 160 * 1024 and \
            pad <= 65536, (k.name, k.tune)
        if k.tune['pipe'] > 1:
          assert static > 0
          seen += 1
        else:
          assert static == 0 and 1024 <= pad <= 65536
  assert seen >= 8
  # the case of the report: T = 12, pipe 4 x 4, occupancy 1
  k = knobs.deepest(knobs.lowered('jacobi2d_T12', dict(
      pipe=4, pipe_rows=4, occupancy=1)))
  assert (k.tune['lds_rings'], k.tune['lds_pad']) == (24576, 81 * 1024 - 24576)
  # ... and without rings the pad is what it was
  k = knobs.deepest(knobs.lowered('jacobi2d_T12', dict(occupancy=1)))
  assert (k.tune['lds_rings'], k.tune['lds_pad']) == (0, 33792)


# ---------------------------------------------------------------------------
# CPU: grids, oracles, compilation
# ---------------------------------------------------------------------------

def _check_grid(prog, row, mod, tiles, extent):
  """`tiles`: {kernel name: tile} of the launch geometry for `extent`."""
  st = knobs.stencil_of(prog)
  k = knobs.deepest(mod)
  tile, ax = tiles[k.name], st.dim - 1
  fixed = knobs.PROGRAMS[prog][2]['chunk_rows']
  assert tile[ax] == fixed * row.get('waves_y', 1), (tile, k.name)
  assert extent[0] == 2 * k.tile[0] + 9 * k.tune['vec'] and tile[0] == k.tile[0]
  assert extent[ax] == 7 * tile[ax] + knobs.RAGGED[st.dim]
  blocks = -(-extent[0] // tile[0]) * -(-extent[ax] // tile[ax])
  if st.dim == 3:
    assert extent[1] == 9 and tile[1] == k.tune['tile_rows']
    assert extent[1] > tile[1] and (extent[1] % tile[1] or tile[1] == 1)
    blocks *= -(-extent[1] // tile[1])
  if '_xcd' in k.name:
    # the renumbering of the kernel is live on such a grid only
    assert blocks % 8 == 0 and 'nblk % 8u == 0u' in mod.source, blocks
  # a tensor of the widest row the rules allow -- two blocks of two strips of
  # 64 lanes and nine lanes, 16 bytes a lane -- on the tallest grid, seven
  # tiles of four chunks of 16 rows and five rows: (4 x 64 + 9) x 16 x 453
  # bytes, under 2 MiB (most rows: a quarter of a MiB)
  nbytes = int(np.prod(extent)) * max(
      t.size_in_bytes for t in tuple(st.input_types) + tuple(st.output_types))
  assert nbytes <= (4 * 64 + 9) * 16 * 453 < (2 << 20), (extent, nbytes)


@functools.lru_cache(maxsize=None)
def _extents(prog):
  return sorted({knobs.setup(prog, _row(p, kind, i))[0]
                 for p, kind, i in RUN_CPU if p == prog})


@pytest.mark.parametrize('prog', PROGS)
def test_the_oracle_is_finite_on_every_grid(built, prog):
  """A NaN in a GPU result can only be a read of a guard."""
  st = knobs.stencil_of(prog)
  assert len(_extents(prog)) >= 1
  for extent in _extents(prog):
    lo, hi = st.valid_box(extent)
    assert all(h > l for l, h in zip(lo, hi)), (extent, lo, hi)
    ins, want = tde._reference(st, extent, knobs.SEED)
    assert tde._kind(st) == ('signed' if prog not in (
        'blur', 'ints2d', 'erosion', 'xcorr') else 'full')
    assert all(np.isfinite(a).all() for a in ins.values()
               if a.dtype.kind == 'f')
    assert tde._finite(st, extent, want), extent


@pytest.mark.parametrize('prog,kind,idx', RUN_CPU,
                         ids=[_run_id(r) for r in RUN_CPU])
def test_every_row_compiles_for_gfx950(built, prog, kind, idx):
  """The module the GPU case builds, compiled here: every kernel of the plan
  has its resources reported, and the launch geometry is the grid's."""
  from soda_amd import runtime
  row = _row(prog, kind, idx)
  st = knobs.stencil_of(prog)
  mod, extent = knobs.module_for(prog, row, probe=True)
  code = runtime.compile_source(mod.source, '%s.hip' % st.app_name)
  res = runtime.kernel_resources(code)
  plan = runtime.make_plan(mod, res)
  for k in mod.kernels:
    r = res.get(k.name)
    assert r and r['vgpr'] > 0, (k.name, sorted(res))
    if k.tune and 'lds_rings' in k.tune:
      assert r['lds'] == k.tune['lds_rings'], (k.name, r)
      assert r['lds'] + k.lds_bytes <= 160 * 1024
    if r['scratch']:
      # not an error under `min_waves` or `occupancy`: slower, not wrong
      print('%s: %d bytes of scratch, %d VGPRs' % (k.name, r['scratch'],
                                                   r['vgpr']))
  tiles, _ = runtime.plan_geometry(plan, extent)
  _check_grid(prog, row, mod,
              {k.name: t[:st.dim] for k, t in zip(mod.kernels, tiles)}, extent)
  # the deepest pass is scheduled by the launch-time model, the same in every
  # session: the GPU case does not depend on the clock
  count = runtime.plan_schedule(plan, extent, st.iterate)
  deepest = max(zip(mod.sorted_passes(), count),
                key=lambda pc: pc[0].fused_iters)
  assert deepest[0].fused_iters == knobs.deepest_depth(prog)
  assert (deepest[1] == 0) == ((prog, knobs.freeze(row)) in knobs.UNSCHEDULED), \
      (count, row)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('prog,kind,idx', RUN_GPU,
                         ids=[_run_id(r) for r in RUN_GPU])
def test_gpu_every_row_between_guards(built, prog, kind, idx):
  """The device entry on signed / full-range cells: the valid box is the C
  oracle's bit for bit, no byte of the arena outside the outputs changed, the
  deepest kernel carries the row's tags and its pass ran."""
  row = _row(prog, kind, idx)
  st = knobs.stencil_of(prog)
  extent, build_for = knobs.setup(prog, row, probe=True)
  ins, want = tde._reference(st, extent, knobs.SEED)
  with tde._program(st, build_for, **knobs.keywords(prog, row)) as p:
    mod = p.module
    k = knobs.deepest(mod)
    names = [q.name for q in mod.kernels]
    assert k.tune['fused'] == knobs.deepest_depth(prog), names
    for o, mark in knobs.marks(prog, row, mod).items():
      assert mark is True or (len(row) == 1 and mark in knobs.NO_EFFECT), \
          (row, o, mark, names)
    _check_grid(prog, row, mod, p.geometry(extent)[0], extent)
    tde._deepest_is_scheduled(p, extent, st.iterate)
    tde._guarded_case(p, st, extent, ins, want,
                      '%s %s (%s)' % (prog, knobs.row_id(row), names))
    assert k.tune['fused'] == 1 or p.last_launches()[1] > 0, p.last_launches()
