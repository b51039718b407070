"""Every native cell type through every form of the kernels, bit for bit.

lower() takes ten cell types, and nearly everything that moves a cell is
written once per cell size, in places once per signedness: the lane shifts and
half-strip rotations of soda_rt.h, the fragment loads and stores, the one-byte
paths, the LDS halos of shared rows, the rings of stage-pipelined blocks, the
item offsets of batched kernels, |cur - prev| of the residual twins, the copy
kernels and bank maps of the wire format.  The rest of the suite pins these
for float and has about one case each for the other types.  Here
(tests/celltypes.py holds the tables):

* the type list is what ir.Type.is_native accepts: a new native type cannot
  arrive untested;
* each type has a program per dimension -- integers: promotion and truncation,
  signed against unsigned division and remainder by a constant, wrap-around; a
  second one with comparison, min and abs -- whose C oracle, numpy oracle and a
  templated C++ loop nest of its own agree bit for bit on full-range cells;
* one row per form (default fused, mixh, pipe 2 / 4, waves_x / waves_y,
  xshare, xshare_block, vec 1 / 2, direct, batch, residual in 2-D; six of them
  in 3-D): every (type, row) lowers with its tag in force, compiles for gfx950
  and has its deepest pass scheduled by the model; `ldswin` and `tile3d` refuse
  by cell type, in a table that is exact both ways;
* on the GPU every (type, row) runs the device entry between guard bands
  against the C oracle: the valid box bit for bit, no byte outside the outputs;
  batch rows three items between guard items, residual rows the 32 bytes of the
  struct as well, and every type the wire format on 2 and on 4 banks.

uint32 / uint64 move the same bits as int32 / int64: their rows on the movement
forms scale with --fuzz-budget, and so do the mixh / pipe=4 / waves rows of
uint8 / uint16 ("Cell types": the file's cold run against the rest
of the suite's); the base rows (default fused, direct, batch, residual) and all
CPU halves never do."""
import functools

import numpy as np
import pytest

import celltypes as ct
import fuzz
import guarded
import test_batch as tb
import test_device_entry as tde
import test_residual as tr
import test_values as tv
import test_wire_banked as twb
import values

ALL = [(t, row) for row in ct.ROWS for t in ct.TYPES]
# the GPU runs: what always runs, then the budget's share of the rest
_REST = [(t, row) for t, row in ALL if not ct.always(t, row)]
RUN_GPU = [(t, row) for t, row in ALL if ct.always(t, row)] + \
    ct.picks(_REST, fuzz.budget())
CMP = [(t, ct.ROW['fused', dim]) for dim in (2, 3) for t in ct.INTS]
TINY = [(t, ct.ROW['fused', dim]) for dim in (2, 3) for t in ct.FLOATS]
_WIRE_REST = [(t, nb) for t in ct.SAME_BITS_AS for nb in ct.BANKS]
WIRE_ALL = [(t, nb) for t in ct.TYPES for nb in ct.BANKS]
WIRE_GPU = [c for c in WIRE_ALL if c not in _WIRE_REST] + \
    ct.picks(_WIRE_REST, fuzz.budget())


def _ids(cases, kind='main'):
  return [ct.row_id(t, row, kind) for t, row in cases]


def _wire_ids(cases):
  return ['%s-wire-%dbanks' % c for c in cases]


def _box(st, extent, iterate=None):
  (_, idx), = tv._boxes(st, extent, iterate)
  return idx


@functools.lru_cache(maxsize=None)
def _reference(t, row, kind='main', inputs='full', seed=ct.SEED):
  """(inputs, C oracle outputs) on the row's grid: computed once, read-only."""
  st = ct.stencil_of(t, row.dim, kind)
  extent = ct.setup(t, row, kind, probe=True)[0]
  ins = tv._readonly(values.edge_inputs(st, extent, seed, inputs))
  return ins, tv._readonly(tv._oracle(st).run(ins))


# ---------------------------------------------------------------------------
# CPU: types, programs, references
# ---------------------------------------------------------------------------

def test_the_types_are_the_native_ones():
  """... among {u,}int{8,16,32,64}, float and double, which is what
  module._check_native names."""
  from soda_amd import ir
  named = ['%sint%d' % (u, w) for w in (8, 16, 32, 64) for u in ('', 'u')] + \
      ['float', 'double']
  native = [n for n in named if ir.Type(n).is_native]
  assert sorted(ct.TYPES) == sorted(native) and len(set(ct.TYPES)) == 10
  for t in ct.TYPES:
    ty = ir.Type(t)
    assert ty.size_in_bytes == ct.SIZE[t] == np.dtype(ty.np_name).itemsize
    assert ty.is_float == (t in ct.FLOATS)
    assert ty.c_type == ct.C_TYPE[t]
  assert set(ct.SAME_BITS_AS) == {'uint32', 'uint64'}
  assert not ir.Type('half').is_native and not ir.Type('int24').is_native


def test_every_type_has_its_programs(built):
  assert len(ct.programs()) == 2 * (10 + 8)
  for t, dim, kind in ct.programs():
    st = ct.stencil_of(t, dim, kind)
    assert [str(x) for x in st.input_types + st.output_types] == [t, t]
    assert st.dim == dim and st.iterate == ct.ITERATE[dim]
    assert tuple(st.tile_size[:-1]) == (32,) * (dim - 1)
    assert not st.local_names and not st.param_stmts
  assert ct.BASE[2]['fuse'] == (4,) and ct.ITERATE[2] == 9     # 4 + 4 + 1
  assert ct.BASE[3]['fuse'] == (2,) and ct.ITERATE[3] == 3     # 2 + 1
  assert (ct.BASE[2]['chunk_rows'], ct.BASE[3]['chunk_rows']) == (16, 4)


def test_the_nest_knows_nothing_of_the_product():
  source = ct.nest_source()
  for word in ('soda', 'oracle', 'SODA'):
    assert word not in source, word
  assert ct.NEST_FLAGS[:3] == ['-O2', '-ffp-contract=off', '-fwrapv']
  assert source.count('template <class T>') == len(ct.NEST) == 6
  assert source.count('extern "C"') == 2 * (8 + 8 + 2)


def _grids(t, dim, kind):
  """The distinct extents of the GPU cases of a program, each with a row that
  runs on it: every row of the dimension for `main`, the default fused row for
  `cmp`."""
  rows = [r for r in ct.ROWS if r.dim == dim] if kind == 'main' else \
      [ct.ROW['fused', dim]]
  seen = {}
  for row in rows:
    seen.setdefault(ct.setup(t, row, kind, probe=True)[0], row)
  return sorted(seen.items())


@pytest.mark.parametrize('t,dim,kind', ct.programs(),
                         ids=['%s-%dd-%s' % p for p in ct.programs()])
def test_three_references_agree_and_do_not_collapse(built, t, dim, kind):
  """On every grid a GPU case of the program runs on, with that case's inputs
  (the reference of a row is the one its GPU case compares with): (a) the
  nest, the C oracle and the numpy oracle, bit for bit on the whole valid box;
  (b) at least 64 distinct values there, all finite."""
  from oracle import numpy_oracle
  st = ct.stencil_of(t, dim, kind)
  grids = _grids(t, dim, kind)
  assert len(grids) >= (4 if kind == 'main' else 1), grids
  for extent, row in grids:
    fused = row.name == 'fused'
    for inputs in ('full', 'tiny') if t in ct.FLOATS and fused else ('full',):
      ins, want = _reference(t, row, kind, inputs)
      a = ins['a']
      assert a.shape == tuple(extent[::-1])
      if t in ct.INTS:
        info = np.iinfo(a.dtype)
        assert a.min() == info.min and a.max() == info.max
      else:
        assert np.isfinite(a).all() and (a < 0).any() and (a > 0).any()
        tiny = (np.abs(a) > 0) & \
            (np.abs(a) < np.finfo(a.dtype).smallest_normal)
        assert tiny.any() == (inputs == 'tiny')
      nest, box = ct.nest_run(t, dim, kind, a)
      lo, hi = st.valid_box(extent)
      assert box == (tuple(lo), tuple(hi)), (box, lo, hi)
      idx = _box(st, extent)
      other = numpy_oracle.run(st, ins)['b']
      for what, got in (('nest', nest), ('numpy oracle', other)):
        same = values.same_bits(got[idx], want['b'][idx])
        assert same.all(), '%s on %s: %d cells differ from the C oracle' % (
            what, extent, int((~same).sum()))
      assert len(np.unique(want['b'][idx])) >= 64, extent
      assert tde._finite(st, extent, want), extent


def test_the_comparison_is_unsigned_where_it_should_be():
  """On uint32 / uint64 cells above the signed maximum the `cmp` program's
  reference differs from the same bits run as int32 / int64."""
  for u, s in ct.SAME_BITS_AS.items():
    a = values._full(np.random.default_rng(3), (12, 40), np.dtype(u))
    assert (a > np.iinfo(s).max).any()
    got, _ = ct.nest_run(u, 2, 'cmp', a, 1)
    as_signed, _ = ct.nest_run(s, 2, 'cmp', a.view(s), 1)
    assert (got[1:-1, 1:-1] != as_signed.view(u)[1:-1, 1:-1]).mean() > 0.2
    # ... and so does the division of the `main` program
    got, _ = ct.nest_run(u, 2, 'main', a, 1)
    as_signed, _ = ct.nest_run(s, 2, 'main', a.view(s), 1)
    assert (got[1:-1, 1:-1] != as_signed.view(u)[1:-1, 1:-1]).mean() > 0.2


# ---------------------------------------------------------------------------
# CPU: forms and refusals
# ---------------------------------------------------------------------------

ASKED = {2: ['fused', 'mixh', 'pipe2', 'pipe4', 'waves_x2', 'waves_y2',
             'xshare', 'xshare_block4', 'vec1', 'vec2', 'direct', 'batch',
             'residual'],
         3: ['fused', 'xshare', 'xshare_block2', 'direct', 'batch', 'residual']}


def test_the_rows_are_those_asked_for():
  for dim in (2, 3):
    assert [r.name for r in ct.ROWS if r.dim == dim] == ASKED[dim]
  assert {r.name for r in ct.ROWS if r.base} == \
      {'fused', 'direct', 'batch', 'residual'}
  assert len(ct.ROW) == len(ct.ROWS) == 19
  # what always runs, by id; the rest is uint32 / uint64 on movement forms
  ids = set(_ids(RUN_GPU))
  moved = ct.NARROW_UNDER_BUDGET
  for t, row in ALL:
    if row.base or not (t in ('uint32', 'uint64') or (
        moved and t in ('uint8', 'uint16') and
        row.name in ('mixh', 'pipe4', 'waves_x2', 'waves_y2'))):
      assert ct.row_id(t, row) in ids
  assert len(_REST) == 2 * (9 + 2) + (8 if moved else 0)
  assert ct.picks(_REST, 0) == [] and ct.picks(_REST, 1 / ct.SHARE) == _REST
  assert len(set(map(_REST.index, ct.picks(_REST, 1)))) == \
      round(len(_REST) * ct.SHARE)
  wire = set(_wire_ids(WIRE_GPU))
  assert all('%s-wire-%dbanks' % (t, nb) in wire for t, nb in WIRE_ALL
             if t not in ('uint32', 'uint64'))


@pytest.mark.parametrize('row', ct.ROWS,
                         ids=['%dd-%s' % (r.dim, r.name) for r in ct.ROWS])
def test_every_type_lowers_with_the_row_in_force(built, row):
  """No refusal, and the shape ladder has not dropped the fused depth: tag,
  depth and descriptor of the deepest kernel, for the module built without an
  extent and for the one the GPU case builds."""
  for t in ct.TYPES:
    for kind in ct.KINDS if (row.name == 'fused' and t in ct.INTS) else \
        ('main',):
      ct.in_force(t, row, ct.lowered(t, row, kind), kind)
      ct.in_force(t, row, ct.module_for(t, row, kind, probe=True)[0], kind)


@pytest.mark.parametrize('family', sorted(ct.REFUSING))
def test_the_table_of_refusals_is_exact(built, family):
  """A type the table lists is refused with the text it names; a type it does
  not list lowers, with the family's kernel in the module."""
  from soda_amd import util
  from soda_amd.codegen.hip import lower
  kw, dim, takes, why = ct.REFUSING[family]
  assert set(takes) <= set(ct.TYPES)
  for t in ct.TYPES:
    st = ct.stencil_of(t, dim)
    if ct.refusal(family, t) is None:
      mod = lower.lower(st, lower.LowerOptions(**kw))
      assert any(family in k.name for k in mod.kernels), \
          [k.name for k in mod.kernels]
    else:
      with pytest.raises(util.SemanticError) as err:
        lower.lower(st, lower.LowerOptions(**kw))
      assert why in str(err.value), (t, str(err.value))
  assert {t for t in ct.TYPES if ct.SIZE[t] == 4} == \
      set(ct.REFUSING['ldswin'][2]) == set(ct.REFUSING['tile3d'][2])


def _check_grid(t, row, mod, tiles, extent):
  """`tiles`: {kernel name: tile} of the launch geometry for `extent`: the
  seams the grid is meant to have."""
  st = ct.stencil_of(t, row.dim)
  k = ct.deepest(mod)
  tile, ax = tiles[k.name], row.dim - 1
  s, v = k.tile[0], k.tune['vec']
  nbytes = int(np.prod(extent)) * ct.SIZE[t]
  if row.name == 'xshare':
    # one block covers the row: at most four waves, the last one ragged
    assert extent[0] == ct.keywords_of(t, row)['row_cells'] <= tile[0] == s
    assert extent[0] % (64 * v) and s <= 4 * 64 * v
  else:
    # two strips (blocks of `xshare_block`) and a ragged third
    assert extent[0] == 2 * s + 9 * v and tile[0] == s, (extent, tile)
  assert extent[0] % v == 0
  if row.name == 'direct':
    assert tuple(extent[1:]) == ct.DIRECT_ROWS[row.dim]
  else:
    chunk = ct.BASE[row.dim]['chunk_rows'] * row.kw.get('waves_y', 1)
    assert tile[ax] == chunk, (tile, k.name)
    assert extent[ax] == 7 * chunk + {2: 5, 3: 2}[row.dim]
    if row.dim == 3:
      assert extent[1] == 9 and tile[1] == k.tune['tile_rows'] == 4
  lo, hi = st.valid_box(extent)
  assert all(h - l >= 2 for l, h in zip(lo, hi)), (extent, lo, hi)
  assert nbytes < (5 << 18)
  assert guarded.layout(st, extent).nbytes < ARENA_LIMIT.get(
      (t, row.name, row.dim), 2 << 20), guarded.layout(st, extent).nbytes


# arenas of 2 MiB or more.  Two blocks of two waves and a ragged third by 9
# rows by 30 planes are 1.1 MiB a tensor from four bytes a cell on, whatever
# the guards: these six rows take 2 380 464 bytes
ARENA_LIMIT = {(t, 'xshare_block2', 3): 2380464 + 1 for t in ct.TYPES
               if ct.SIZE[t] >= 4}


def _compiled_schedule(t, row, kind, alone=False):
  """(module, extent, {depth: launches by the model}) of a row, compiled."""
  from soda_amd import runtime
  st = ct.stencil_of(t, row.dim, kind)
  mod, extent = ct.module_for(t, row, kind, probe=True, alone=alone)
  code = runtime.compile_source(mod.source, '%s.hip' % st.app_name)
  res = runtime.kernel_resources(code)
  plan = runtime.make_plan(mod, res)
  for k in mod.kernels:
    r = res.get(k.name)
    assert r and r['vgpr'] > 0, (k.name, sorted(res))
    if k.tune and 'lds_rings' in k.tune:
      # the rings of a stage-pipelined block, the halos of shared rows
      shares = '_xs' in k.name or '_xb' in k.name
      assert (r['lds'] == k.tune['lds_rings']) != shares and \
          (r['lds'] > 0) == (k.tune['pipe'] > 1 or shares), (k.name, r)
      assert r['lds'] + k.lds_bytes <= 160 * 1024, (k.name, r)
      if k.tune['pipe'] > 1:
        assert r['lds'] % ct.SIZE[t] == 0, (k.name, r)
    # a residual twin that spills is not launched, the run then ends in the
    # one-iteration twin (tests/test_residual.py test_3d_seams): which ones
    # do is a table, and nothing else spills
    spills = ct.SPILLING_TWIN.get((t, row.dim), 0) if (
        kind == 'main' and row.name == 'residual' and
        k.name.endswith('_rs') and k.tune['fused'] > 1) else 0
    assert r['scratch'] == spills, (k.name, r, spills)
  if (row.name, row.dim) in ct.SHARED_LDS and kind == 'main':
    assert res[ct.deepest(mod).name]['lds'] == \
        ct.SHARED_LDS[row.name, row.dim][ct.SIZE[t]], res[ct.deepest(mod).name]
  tiles, _ = runtime.plan_geometry(plan, extent)
  if kind == 'main' and not alone:
    _check_grid(t, row, mod,
                {k.name: tl[:row.dim] for k, tl in zip(mod.kernels, tiles)},
                extent)
  if row.name == 'batch':
    count = runtime.plan_schedule_batch(plan, extent, ct.BATCH, st.iterate)
  else:
    count = runtime.plan_schedule(plan, extent, st.iterate)
  sched = {p.fused_iters: c for p, c in zip(mod.sorted_passes(), count)}
  assert sum(d * c for d, c in sched.items()) == st.iterate
  return mod, extent, sched


COMPILED = [(t, row, 'main') for t, row in ALL] + [(t, row, 'cmp')
                                                   for t, row in CMP]


@pytest.mark.parametrize('t,row,kind', COMPILED,
                         ids=_ids(ALL) + _ids(CMP, 'cmp'))
def test_every_row_compiles_for_gfx950(built, t, row, kind):
  """The module the GPU case builds, compiled here: every kernel has its
  resources reported and none spills but the deep residual twins of
  celltypes.SPILLING_TWIN, the launch geometry is the grid's, and
  the model -- the same in every session -- schedules the deepest pass.  Where
  it would not (celltypes.UNSCHEDULED: one-byte cells at sixteen a lane, whose
  four-iteration kernel it prices at 42.9 us against 4 x 10.3 us) the row has
  eight cells a lane beside it, and the list is exact both ways."""
  st = ct.stencil_of(t, row.dim, kind)
  mod, extent, sched = _compiled_schedule(t, row, kind)
  if row.name == 'direct':
    assert sched == {1: st.iterate}
    return
  d = ct.depth(row)
  assert sched == {d: st.iterate // d, 1: st.iterate % d}, sched
  if ct.unscheduled(t, row, kind):
    alone, _, sched = _compiled_schedule(t, row, kind, alone=True)
    ct.in_force(t, row, alone, kind)
    assert sched == {d: 0, 1: st.iterate}, sched
    assert ct.deepest(mod).tune['vec'] == 8 < ct.deepest(alone).tune['vec']
  else:
    assert mod.source == ct.module_for(t, row, kind, probe=True,
                                       alone=True)[0].source


def _per_cycle(t, nb):
  """Elements a cycle of the wire format moves: soda_hip_stream_desc_t
  elems_per_cycle."""
  from soda_amd import stream
  st = twb._program(ct.text(t, 2), nb, nb, None, 2)
  return stream.stream_specs(st, dense=True)[0].elems_per_cycle[0]


@pytest.mark.parametrize('t', ct.TYPES)
def test_which_wire_programs_have_a_banked_form(built, t):
  """Every (cell size, banks) but 8-byte cells on 4 banks; where it is
  offered, inputs and outputs alike are in the kernel.  The dense arm compiles
  its per-size copy kernels either way."""
  from soda_amd import stream
  for nb in ct.BANKS:
    tile = ct.wire_tile(t, nb)
    extent = ct.wire_extent(t, nb)
    assert 2 * tile < extent[0] < 3 * tile and extent[1] == 20
    # whole cycles, whole bank groups: there is a dense view
    assert tile % _per_cycle(t, nb) == 0 and tile % nb == 0
    st = twb._program(ct.text(t, 2), nb, nb, (tile,), 2)
    assert st.iterate == 2 and tuple(st.tile_size[:-1]) == (tile,)
    sp = stream.stream_specs(st, dense=True, banked=True)[1]
    offered = 'dense_banked' in sp and sp['dense_banked'].in_kernel
    if (ct.SIZE[t], nb) in ct.NOT_BANKED:
      assert not offered, (t, nb)
    else:
      assert offered == {'a': nb, 'b': nb}, (t, nb, offered)
      twb._banked_kernel_text(st, sp['dense_banked'])
    assert 'dense' in sp and 'unwire_a' in sp
  assert ct.NOT_BANKED == {(8, 4)}


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _run_between_guards(t, row, kind='main', inputs='full'):
  """The device entry of a row's program on its grid: the valid box is the C
  oracle's bit for bit, no byte of the arena outside the output changed, the
  row is in force and its deepest pass ran."""
  st = ct.stencil_of(t, row.dim, kind)
  extent, build_for = ct.setup(t, row, kind, probe=True)
  ins, want = _reference(t, row, kind, inputs)
  with tde._program(st, build_for, **ct.keywords(t, row, kind)) as p:
    mod = p.module
    names = [q.name for q in mod.kernels]
    ct.in_force(t, row, mod, kind)
    if kind == 'main':
      _check_grid(t, row, mod, p.geometry(extent)[0], extent)
    what = '%s %s (%s)' % (ct.row_id(t, row, kind), inputs, names)
    if row.name == 'batch':
      _batch_case(p, st, extent, what)
      return
    tde._deepest_is_scheduled(p, extent, st.iterate)
    tde._guarded_case(p, st, extent, ins, want, what)
    assert row.name == 'direct' or p.last_launches()[1] > 0, p.last_launches()
    if row.name == 'residual':
      # ... and the 32 bytes of the struct, against |cur - prev| formed
      # exactly (through uint64 for 8-byte cells); the maximum is near the
      # type's range on full-range cells
      # -- a residual run launches its deepest pass last, as its twin: the
      # row's depth, but for the twins of celltypes.SPILLING_TWIN, which the
      # library does not launch (then the one-iteration twin)
      kept = {q.tune['fused'] for i, q in enumerate(mod.kernels)
              if q.twin >= 0 and p.plan.kernels[i].twin >= 0}
      spills = kind == 'main' and (t, row.dim) in ct.SPILLING_TWIN
      assert kept == ({1} if spills else {1, ct.depth(row)}), (kept, names)
      got, mode = tr._check(p, st, extent, ins, st.iterate)
      assert mode == ('twin', 1 if spills else ct.depth(row)), (mode, kept)
      assert got.changed > 0, got
      if t in ct.INTS:
        info = np.iinfo(t)
        # (the 2-D program ends in a division by 4: its cells, and so their
        # deltas, span a quarter of the range; the maximum of tens of
        # thousands of deltas lies in the upper half of that span)
        assert got.max_int > (int(info.max) - int(info.min)) // 8, got
      else:
        assert got.max_float > 0 and got.max_int == 0, got


def _batch_case(p, st, extent, what):
  """Three items of one extent through run_device(batch=3): a guard item each
  side of the outputs, every item against its own oracle run."""
  items = [values.edge_inputs(st, extent, ct.SEED + i, 'full')
           for i in range(ct.BATCH)]
  ins = {'a': np.stack([item['a'] for item in items])}
  want = [tv._oracle(st).run(item) for item in items]
  assert p.plan.batched == 1
  sched = p.schedule(extent, st.iterate, ct.BATCH)
  deepest = max(q.fused_iters for q in p.module.passes)
  assert sched.get(deepest), sched
  got = tb._guarded_run(st, p, extent, ct.BATCH, st.iterate, ins)
  tb._compare(st, p, extent, st.iterate, got, want, False, what)
  assert p.last_launches()[1] > 0, p.last_launches()


@pytest.mark.gpu
@pytest.mark.parametrize('t,row', RUN_GPU, ids=_ids(RUN_GPU))
def test_gpu_every_type_on_every_row(built, t, row):
  """Full-range integers -- every product wraps, the type's extremes are
  planted -- and signed floats."""
  _run_between_guards(t, row)


@pytest.mark.gpu
@pytest.mark.parametrize('t,row', CMP, ids=_ids(CMP, 'cmp'))
def test_gpu_comparisons_on_every_integer_type(built, t, row):
  """select over a comparison of two taps, min and abs, fused."""
  _run_between_guards(t, row, 'cmp')


@pytest.mark.gpu
@pytest.mark.parametrize('t,row', TINY, ids=_ids(TINY, 'tiny'))
def test_gpu_subnormals_on_the_default_rows(built, t, row):
  _run_between_guards(t, row, inputs='tiny')


@pytest.fixture
def model_schedules(monkeypatch):
  """As tests/test_wire_banked.py: both arms of a wire case take the launches
  the model names."""
  monkeypatch.setenv('SODA_HIP_NO_CALIBRATE', '1')


@pytest.mark.gpu
@pytest.mark.parametrize('t,nb', WIRE_GPU, ids=_wire_ids(WIRE_GPU))
def test_gpu_every_type_on_the_wire(built, model_schedules, t, nb):
  """The 2-D program at two iterations, inputs and outputs on `nb` banks, two
  tiles and a ragged third by 20 rows: agreement with the reference's kernel
  contract, the copy path's banks over the dense view, guards and tail
  untouched, and the path taken -- `banked` wherever the form is offered,
  else `dense`, whose per-size copy kernels run on both sides either way."""
  st = twb._program(ct.text(t, 2), nb, nb, (ct.wire_tile(t, nb),), 2)
  banked = (ct.SIZE[t], nb) not in ct.NOT_BANKED
  picked = twb._check_case(st, ct.wire_extent(t, nb),
                           expect='banked' if banked else 'dense')
  assert picked == ({'a': nb, 'b': nb} if banked else {})
