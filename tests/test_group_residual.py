"""Residual of the last iteration on slab and group runs; a group run until
converged (soda_hip_plan_residual_slab_box, soda_hip_run_device_slab_residual,
soda_hip_group_run_residual / _residual / _run_until).

The yardstick is always the oracle on the WHOLE grid -- `_expected` of
tests/test_residual.py, which knows nothing of slabs -- and every comparison is
`==` on all four fields: sums and maxima of exact per-cell values combine over
N slabs without a tolerance.

CPU: the slab boxes partition the global box; the launches of a residual slab
run end in the pass that takes the residual, and the cone of the passes before
it is that of the order launched; refusals; the ABI is what it was.  GPU: N
virtual slabs on one device against the oracle, at the seams of strips, chunks
and slabs."""
import ctypes

import numpy as np
import pytest

from conftest import soda_path
import guarded
import values
import test_residual as tr
from test_residual import (BOXES, _delta, _expected, _fields, _inputs, _opts,
                           _stencil)

# soda_hip_sizeof(0..13) before this change: no struct may change layout
SIZEOF = [256, 188, 76, 9088, 32, 312, 48, 296, 304, 40, 40, 32, 256, 0]


def _slabs(rows, n, ghost_lo, ghost_hi):
  """[(begin, own_begin, own_end, end)]: the group's cut of `rows` rows
  (soda_group.cpp slab_rows), ghost rows clipped to the grid."""
  base, extra = rows // n, rows % n
  out = []
  for s in range(n):
    own0 = s * base + min(s, extra)
    own1 = own0 + base + (1 if s < extra else 0)
    out.append((max(0, own0 - (ghost_lo if s else 0)), own0, own1,
                min(rows, own1 + (ghost_hi if s < n - 1 else 0))))
  return out


_WANT = {}


def _want(key, stencil, ins, extent, iterate):
  """`_expected`, once per (key, iterate): shared, never written."""
  k = (key, tuple(extent), iterate)
  if k not in _WANT:
    _WANT[k] = _expected(stencil, ins, extent, iterate)
  return _WANT[k]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_abi_is_what_it_was(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert runtime.ABI_VERSION == 9 and lib.soda_hip_abi_version() == 9
  assert [lib.soda_hip_sizeof(i) for i in range(len(SIZEOF))] == SIZEOF
  for name in ('soda_hip_plan_residual_slab_box',
               'soda_hip_run_device_slab_residual',
               'soda_hip_plan_launches_residual', 'soda_hip_group_run_residual',
               'soda_hip_group_residual', 'soda_hip_group_last_residual',
               'soda_hip_group_run_until'):
    assert name in runtime.API and hasattr(lib, name), name


@pytest.mark.parametrize('name,border,extent', BOXES)
def test_slab_boxes_partition_the_global_box(built, name, border, extent):
  """N = 1..5 slabs of `extent` (and of 121 rows: ragged), iterate 1, 4, 13:
  per output the slabs' boxes are disjoint along the last dimension, their
  cells add up to the global box's, and each is Stencil.valid_box cut to the
  slab's kept rows, in the slab's coordinates.  Slabs whose kept rows miss the
  global box count nothing."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=2, border=border)
  plan = runtime.make_plan(lower.lower(stencil, _opts(peel=0)))
  dim = stencil.dim
  reach = stencil.reach_along(dim - 1)
  empty_slabs = 0
  for rows in (extent[-1], 121):
    ext = tuple(extent[:-1]) + (rows,)
    for iterate in (1, 4, 13):
      whole = runtime.plan_residual_box(plan, ext, iterate)
      for n in range(1, 6):
        cells = [0] * len(stencil.output_names)
        last_end = [0] * len(stencil.output_names)
        for begin, own0, own1, end in _slabs(rows, n, 2 * reach[0],
                                             2 * reach[1]):
          origin = (0,) * (dim - 1) + (begin,)
          local = ext[:-1] + (end - begin,)
          keep = (own0 - begin, own1 - begin)
          got = runtime.plan_residual_box(plan, local, iterate, origin=origin,
                                          global_extent=ext, keep=keep)
          for o, out in enumerate(stencil.output_names):
            lo, hi = got[o]
            assert all(0 <= l <= h <= e for l, h, e in zip(lo, hi, local))
            assert keep[0] <= lo[-1] <= hi[-1] <= keep[1], (out, lo, hi, keep)
            want = runtime.clipped_box(stencil.valid_box(ext, out, iterate),
                                       ext)
            assert (list(whole[o][0]), list(whole[o][1])) == want
            w_lo = max(want[0][-1], own0)
            w_hi = max(w_lo, min(want[1][-1], own1))
            count = int(np.prod([h - l for l, h in zip(lo, hi)]))
            assert count == (w_hi - w_lo) * int(np.prod(
                [h - l for l, h in zip(want[0][:-1], want[1][:-1])])), \
                (out, n, iterate, lo, hi)
            if count:
              assert (list(lo[:-1]), list(hi[:-1])) == (want[0][:-1],
                                                        want[1][:-1])
              assert (lo[-1] + begin, hi[-1] + begin) == (w_lo, w_hi)
              assert lo[-1] + begin >= last_end[o], 'slab boxes overlap'
              last_end[o] = hi[-1] + begin
            else:
              assert lo[-1] == hi[-1] or any(l == h for l, h in zip(lo, hi))
              empty_slabs += 1
            cells[o] += count
        for o in range(len(cells)):
          lo, hi = whole[o]
          assert cells[o] == int(np.prod([h - l for l, h in zip(lo, hi)])), \
              (stencil.output_names[o], n, iterate)
  if border is None:
    assert empty_slabs, 'no slab lay wholly outside the global box'
  else:     # `border: preserve`: a slab counts its kept rows, all of them
    assert not empty_slabs


def _slab_plan(border=None, fuse=(4,)):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=13, border=border)
  opts = runtime.resolve_options(stencil, _opts(fuse=fuse, peel=0), (520, 48),
                                 probe=False)
  mod = lower.lower(stencil, opts)
  code = runtime.compile_source(mod.source, 'jacobi2d.hip')
  return stencil, runtime.make_plan(mod, runtime.kernel_resources(code))


@pytest.mark.parametrize('fuse', [(4,), (8, 4)])
def test_planned_launches_of_a_residual_slab_run(built, fuse, monkeypatch):
  """A middle slab of 48 rows, 4 ghost rows per side: the pass that takes the
  residual is launched last (split: its two parts are one entry), the multiset
  of depths is the plain run's, and walking backwards every pass covers
  exactly what the passes behind it read -- the cone of the order LAUNCHED:
  for 5 = 4 + 1 iterations the one-iteration pass now goes first and must
  cover keep +- 5 rows, not keep +- 1."""
  from soda_amd import runtime
  stencil, plan = _slab_plan(fuse=fuse)
  extent, keep = (520, 48), (4, 44)
  rlo, rhi = stencil.reach_along(1)
  seen_split = seen_moved = 0
  for generic in (False, True):
    if generic:
      monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
    for iterate in (1, 4, 5, 9, 12, 13):
      for exchanged in (False, True):
        run = runtime.SlabRun(keep[0], keep[1], rlo, rhi,
                              4 if exchanged else 0, 4 if exchanged else 0, 4,
                              4, 1 if exchanged else None, 1)
        plain = runtime.plan_launches(plan, extent, iterate, run)
        got, mode = runtime.plan_launches(plan, extent, iterate, run,
                                          residual=True)
        assert mode == ('generic' if generic else 'twin')
        if generic:
          # ends in the one-iteration pass; a schedule that had none is re-cut
          assert got[-1]['fused_iters'] == 1
          assert sum(l['fused_iters'] for l in got) == iterate
        else:
          assert sorted(l['fused_iters'] for l in got) == \
              sorted(l['fused_iters'] for l in plain)
          assert got[-1]['fused_iters'] == max(l['fused_iters'] for l in got)
          seen_moved += [l['fused_iters'] for l in got] != \
              [l['fused_iters'] for l in plain]
        assert [l['record'] for l in got] == [0] * (len(got) - 1) + [1]
        assert [l['wait'] for l in got] == \
            [1 if exchanged else 0] + [0] * (len(got) - 1)
        need = keep
        for l in reversed(got):
          t = l['fused_iters']
          need = (max(0, need[0] - t * rlo), min(extent[1], need[1] + t * rhi))
          assert (l['lo'], l['hi']) == need, (iterate, got)
        last = got[-1]
        if last['split']:
          seen_split += 1
          n = last['hi'] - last['lo']
          assert last['chunks'] == -(-n // last['chunk'])
          for c in range(last['bnd_lo'], last['bnd_hi']):   # the interior
            first = last['lo'] + c * last['chunk']
            end = last['lo'] + min((c + 1) * last['chunk'], n)
            assert first >= keep[0] + run.send_lo
            assert end <= keep[1] - run.send_hi
  assert seen_split, 'no last pass was split'
  assert seen_moved, 'no schedule had its deepest pass moved to the end'


def test_refusals(built):
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=4)
  # a plan without residual: the pure entries say UNSUPPORTED
  bare = runtime.make_plan(lower.lower(
      stencil, lower.LowerOptions(fuse=(4,), peel=0)))
  with pytest.raises(util.BackendError, match='no residual'):
    runtime.plan_residual_box(bare, (64, 20), 4, origin=(0, 4),
                              global_extent=(64, 40), keep=(2, 18))
  with pytest.raises(util.BackendError, match='no residual'):
    runtime.plan_launches(bare, (64, 20), 4, residual=True)
  # a slab that does not lie in the grid, kept rows that are not the slab's
  plan = runtime.make_plan(lower.lower(stencil, _opts(fuse=(4,), peel=0)))
  with pytest.raises(util.BackendError, match='global grid'):
    runtime.plan_residual_box(plan, (64, 20), 4, origin=(0, 30),
                              global_extent=(64, 40))
  with pytest.raises(util.BackendError, match='keep'):
    runtime.plan_residual_box(plan, (64, 20), 4, origin=(0, 4),
                              global_extent=(64, 40), keep=(2, 21))
  # `batch` with `residual`: still refused where the module is made
  with pytest.raises(util.SemanticError, match='residual.*batch'):
    lower.lower(stencil, _opts(batch=True, peel=0))


# ---------------------------------------------------------------------------
# GPU: N virtual slabs on one device
# ---------------------------------------------------------------------------

def _same_on_box(stencil, extent, got, cur, iterate):
  for o in stencil.output_names:
    lo, hi = stencil.valid_box(extent, o, iterate)
    box = tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]
    assert values.same_bits(got[o][box], cur[o][box]).all(), \
        'output %s differs from the oracle (iterate %d)' % (o, iterate)


def _group_run(group, stencil, extent, ins, iterate, key, ahead=0):
  """load, (run `ahead`,) run with a residual, fetch, store: every figure
  against the oracle on the whole grid after ahead + iterate iterations.
  Returns ([how each slab took its share], stats)."""
  total = ahead + iterate
  want, cur = _want(key, stencil, ins, extent, total)
  group.load(ins)
  if ahead:
    group.run(ahead)
  group.run(iterate, residual=True)
  got, each = group.residual(per_slab=True)
  stats = group.stats()
  how = [group.last_residual(s) for s in range(len(each))]
  assert _fields(got) == want, (total, how, got, want)
  assert sum(r.changed for r in each) == got.changed
  assert sum(r.unordered for r in each) == got.unordered
  assert max(r.max_float for r in each) == got.max_float
  assert max(r.max_int for r in each) == got.max_int
  _same_on_box(stencil, extent, group.store(total), cur, total)
  return how, stats


@pytest.mark.gpu
@pytest.mark.parametrize('every', [1, 4])
@pytest.mark.parametrize('slabs', [1, 2, 3])
@pytest.mark.parametrize('border', ['ignore', 'preserve'])
@pytest.mark.parametrize('extent', [(520, 120), (516, 121)])
def test_jacobi2d_slabs(built, extent, border, slabs, every):
  """Rows of 520 / 516 cells (two strips and a ragged third), 120 / 121 rows
  over 1..3 slabs, chunks of 8 rows.  12 iterations end in an interval of 4 (a
  fused twin takes the residual), 13 in an interval of 1, 1 is a fresh state
  without an exchange; `fuse=(4,)` and the default set."""
  from soda_amd import runtime
  stencil = _stencil('jacobi2d.soda', iterate=13, border=border)
  ins = _inputs(stencil, extent)
  for kw in (dict(fuse=(4,)), dict()):
    with runtime.Group(stencil, extent, [0] * slabs, _opts(**kw),
                       exchange_every=every) as group:
      for iterate in (1, 12, 13):
        how, stats = _group_run(group, stencil, extent, ins, iterate,
                                ('jacobi2d', border))
        if kw:     # (the default set may hold a depth whose twin did not fit)
          assert all(h[0] == 'twin' for h in how), how
        k = stats['exchange_every']
        assert k == every and stats['intervals'] == -(-iterate // k)
        last = iterate - (stats['intervals'] - 1) * k
        assert all(h[1] <= last for h in how), (how, last)
        if every == 4 and iterate == 12 and kw:
          assert all(h[1] == 4 for h in how), how


@pytest.mark.gpu
@pytest.mark.parametrize('threads,overlap', [(True, True), (False, False),
                                             (True, False)])
def test_threaded_and_without_overlap(built, threads, overlap):
  """One enqueueing thread per slab, and exchange-then-compute: the same
  figures.  With overlap the last pass of a middle slab is split around the
  exchange and its twin runs twice on one struct."""
  from soda_amd import runtime
  extent = (520, 120)
  stencil = _stencil('jacobi2d.soda', iterate=13, border='preserve')
  ins = _inputs(stencil, extent)
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(4,)),
                     exchange_every=4, overlap=overlap,
                     threads=threads) as group:
    for iterate in (12, 13):
      how, stats = _group_run(group, stencil, extent, ins, iterate,
                              ('jacobi2d', 'preserve'))
      assert all(h[0] == 'twin' for h in how), how
      assert (stats['split_passes'] > 0) == overlap, stats


@pytest.mark.gpu
def test_twin_generic_and_split_all_occur(built, monkeypatch):
  """Through soda_hip_group_last_residual and the group's stats: a split last
  pass taken by a fused twin; the same run with the twins switched off ends in
  `<app>_residual` behind both parts."""
  from soda_amd import runtime
  extent = (520, 120)
  stencil = _stencil('jacobi2d.soda', iterate=13)
  ins = _inputs(stencil, extent)
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(4,)),
                     exchange_every=4) as group:
    how, stats = _group_run(group, stencil, extent, ins, 12,
                            ('jacobi2d', 'ignore'))
    assert how == [('twin', 4)] * 3, how
    # every slab's last pass of the last interval is split, and more
    assert stats['split_passes'] >= 3, stats
    monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
    how, stats = _group_run(group, stencil, extent, ins, 12,
                            ('jacobi2d', 'ignore'))
    assert how == [('generic', 1)] * 3, how
    assert stats['split_passes'] >= 3, stats


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['strips', 'rows'])
def test_heat3d_slabs(built, form, monkeypatch):
  """heat3d 72 x 24 x 36 over 3 slabs of 12 planes, exchange every 2, with
  overlapping strips and with blocks that cover whole rows.  A fused kernel
  that has a twin takes the residual of 2 iterations itself; where it has none
  (the whole-row twin is kept only where it compiles without spilling), and
  with the twins switched off, the interval ends in a one-iteration pass and
  `<app>_residual` over the slab's arrays: the generic path on a slab."""
  from soda_amd import runtime
  extent = (72, 24, 36)
  stencil = _stencil('heat3d.soda', iterate=3)
  ins = _inputs(stencil, extent)
  kw = dict(xshare=False) if form == 'strips' else {}
  with runtime.Group(stencil, extent, [0] * 3,
                     _opts(fuse=(2,), chunk_rows=8, **kw),
                     exchange_every=2) as group:
    march = [k for k in tr._march(group.module)
             if not k.name.endswith(tr.SUFFIX)]
    fused, = [k for k in march if k.tune['fused'] == 2]
    assert ('_xs' in fused.name) == (form == 'rows'), fused.name
    # (the plan keeps a twin only if it compiled without spilling)
    has_twin = group.plan.kernels[[k.name for k in group.module.kernels]
                                  .index(fused.name)].twin >= 0
    if form == 'strips':
      assert has_twin
    for iterate in (1, 2, 3):
      how, _ = _group_run(group, stencil, extent, ins, iterate, 'heat3d')
      if iterate == 2:
        want = ('twin', 2) if has_twin else ('generic', 1)
        assert how == [want] * 3, how
      else:
        assert how == [('twin', 1)] * 3, how
    monkeypatch.setenv('SODA_HIP_RESIDUAL_GENERIC', '1')
    for iterate in (2, 3):
      how, _ = _group_run(group, stencil, extent, ins, iterate, 'heat3d')
      assert how == [('generic', 1)] * 3, how


UPWIND = '''kernel: upwind
burst width: 64
unroll factor: 2
iterate: 4
input float: u(64, *)
output float: v(0, 0) = (u(0, 0) + u(0, 1) + u(-1, 0) + u(1, 1)) * 0.25f
'''


@pytest.mark.parametrize('name,extent,every,iterate', [
    ('coupled2d.soda', (264, 60), 3, 5),
    ('skew2d.soda', (264, 60), 2, 5),
    (UPWIND, (264, 60), 2, 5),
], ids=['coupled2d', 'skew2d', 'upwind'])
@pytest.mark.gpu
def test_two_pairs_and_a_one_sided_reach(built, name, extent, every, iterate):
  """coupled2d: two pairs, each on its own box.  skew2d: windows that lean
  (its reach along the rows is (2, 2): two-sided).  upwind: a reach of (0, 1)
  -- ghosts on one side, sends on the other."""
  from soda_amd import runtime
  stencil = _stencil(name, iterate=iterate)
  ins = _inputs(stencil, extent)
  if name == UPWIND:
    assert stencil.reach_along(1) == (0, 1)
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(every,)),
                     exchange_every=every) as group:
    assert sum(group.slab(s).ghost_lo + group.slab(s).ghost_hi
               for s in range(3)) > 0
    for n in (1, every, iterate):
      _group_run(group, stencil, extent, ins, n, name)


@pytest.mark.gpu
@pytest.mark.parametrize('iterate', [1, 2, 5])
def test_a_cell_on_a_slab_seam_counts_once(built, iterate):
  """NaN and +-inf on the first and the last kept row of the middle slab and on
  the rows next to them -- the neighbours' last and first kept rows, which the
  middle slab holds as ghost rows and writes too: `unordered` and `changed`
  are the oracle's, the slabs' structs add up."""
  from soda_amd import runtime
  extent = (520, 120)
  stencil = _stencil('jacobi2d.soda', iterate=5)
  at = [(7, 39), (8, 40), (300, 79), (301, 80), (519, 40), (0, 79)]
  ins = values.edge_inputs(stencil, extent, 11, 'nonfinite', at=at)
  assert sorted(values.nonfinite_cells(ins['t1'])) == sorted(at)
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(4,)),
                     exchange_every=4) as group:
    info = group.slab(1)
    assert (info.own_begin, info.own_end) == (40, 80)
    _group_run(group, stencil, extent, ins, iterate, 'seam')
    got = group.residual()
    assert got.unordered > 0 and got.changed >= got.unordered


@pytest.mark.gpu
def test_all_zero_input_gives_four_zeros(built):
  from soda_amd import runtime
  extent = (520, 120)
  stencil = _stencil('jacobi2d.soda', iterate=5)
  ins = {'t1': np.zeros(extent[::-1], np.float32)}
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(4,)),
                     exchange_every=4) as group:
    for iterate in (1, 5):
      group.load(ins)
      group.run(iterate, residual=True)
      got, each = group.residual(per_slab=True)
      assert _fields(got) == (0, 0, 0.0, 0)
      assert [_fields(r) for r in each] == [(0, 0, 0.0, 0)] * 3


@pytest.mark.gpu
def test_repeated_runs_on_one_loaded_group(built):
  """run(5), then run(7, residual=True): the box is that of 12 iterations; a
  second load starts the count again.  Without a residual run the group has
  none to give, and a plain group refuses."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  extent = (520, 120)
  stencil = _stencil('jacobi2d.soda', iterate=13)
  ins = _inputs(stencil, extent)
  with runtime.Group(stencil, extent, [0] * 3, _opts(fuse=(4,)),
                     exchange_every=4) as group:
    with pytest.raises(util.BackendError, match='no state'):
      group.run(3, residual=True)
    _group_run(group, stencil, extent, ins, 7, ('jacobi2d', 'ignore'),
               ahead=5)
    group.run(2)
    with pytest.raises(util.BackendError, match='took no residual'):
      group.residual()
    _group_run(group, stencil, extent, ins, 1, ('jacobi2d', 'ignore'))
  with runtime.Group(stencil, extent, [0] * 2, lower.LowerOptions(fuse=(4,)),
                     exchange_every=4) as plain:
    plain.load(ins)
    with pytest.raises(util.BackendError, match='(?i)unsupported|cannot serve'):
      plain.run(4, residual=True)
    assert plain.stats()['launches'] == 0
    with pytest.raises(util.BackendError, match='(?i)unsupported|cannot serve'):
      plain.run_until(0.0, 4)


@pytest.mark.gpu
def test_group_run_until(built):
  """The table of test_the_definition_on_the_issue_table: jacobi2d `preserve`,
  shape (40, 64), default_rng(7), two slabs, a check every 16 iterations.
  Tolerances between the tabulated maxima stop at 16, 32 and 64."""
  from soda_amd import runtime
  extent = (64, 40)
  stencil = _stencil('jacobi2d.soda', iterate=64, border='preserve')
  ins = {'t1': np.random.default_rng(7).random((40, 64), dtype=np.float32)}
  table = {16: (2356, 0.005204678), 32: (2356, 0.002126694),
           64: (2355, 0.000624001)}
  with runtime.Group(stencil, extent, [0, 0], _opts(), iterate=16) as group:
    # (after 48 iterations the oracle's maximum is 0.00106: above 0.0008)
    for tol, stop in ((0.006, 16), (0.003, 32), (0.0008, 64)):
      group.load(ins)
      done, res = group.run_until(tol, 200, check_every=16)
      assert done == stop, (tol, done, res)
      want, cur = _want('until', stencil, ins, extent, stop)
      assert _fields(res) == want
      assert res.changed == table[stop][0]
      assert abs(res.max_float - table[stop][1]) < 1e-6 * table[stop][1]
      _same_on_box(stencil, extent, group.store(stop), cur, stop)
    # too few iterations allowed: OK, with the count done
    group.load(ins)
    done, res = group.run_until(1e-9, 40, check_every=16)
    assert done == 40 and res.max_float > 1e-9
    assert _fields(res) == _want('until', stencil, ins, extent, 40)[0]


@pytest.mark.gpu
def test_the_slab_entry_between_guard_bands(built):
  """One middle slab by itself: rows [36, 84) of a 520 x 120 grid, of which it
  keeps [40, 80).  Its share is the oracle's delta on those rows of the global
  box; no byte outside the outputs and the 32 bytes changes; `box_iterate`
  below `iterate` is refused with nothing launched."""
  from soda_amd import runtime, util
  extent, rows = (520, 120), (36, 84)
  local, keep = (520, rows[1] - rows[0]), (4, 44)
  for border in ('ignore', 'preserve'):
    stencil = _stencil('jacobi2d.soda', iterate=4, border=border)
    ins = _inputs(stencil, extent)
    with runtime.Program(stencil, _opts(fuse=(4,), chunk_rows=8, peel=1),
                         calibrate=False) as prog, tr._Device() as dev:
      event = runtime.Event()
      for ahead in (0, 5):
        total = ahead + 4
        _, cur = _want(('jacobi2d', border), stencil, ins, extent, total)
        _, before = _want(('jacobi2d', border), stencil, ins, extent,
                          total - 1)
        state = ins['t1'] if not ahead else _want(
            ('jacobi2d', border), stencil, ins, extent, ahead)[1]['t0']
        lo, hi = runtime.clipped_box(stencil.valid_box(extent, 't0', total),
                                     extent)
        box = (slice(max(lo[1], 40), min(hi[1], 80)), slice(lo[0], hi[0]))
        want = _delta(cur['t0'][box], before['t0'][box])
        res = dev.alloc(32, fill=0xFF)
        kw = dict(origin=(0, rows[0]), global_extent=extent, keep=keep,
                  sends=(4, 4), sendable=event.handle(), residual=res,
                  box_iterate=total)
        slab_ins = {'t1': np.ascontiguousarray(state[rows[0]:rows[1]])}
        got, violation, _ = guarded.run(prog, stencil, local, slab_ins, 4, **kw)
        assert violation is None, violation
        assert _fields(prog.residual(res)) == want, (border, ahead)
        assert prog.last_residual() == ('twin', 4)
        assert prog.last_split() == 1
        assert values.same_bits(got['t0'][keep[0]:keep[1], lo[0]:hi[0]],
                                cur['t0'][40:80, lo[0]:hi[0]]).all()
        assert prog.residual_box(local, total, origin=(0, rows[0]),
                                 global_extent=extent, keep=keep) == \
            [((lo[0], 4), (hi[0], 44))]
      # refused: the state cannot have seen fewer iterations than this call
      res = dev.alloc(32, fill=0xA5)
      kw.update(residual=res, box_iterate=3)
      with pytest.raises(util.BackendError, match='box_iterate'):
        guarded.run(prog, stencil, local, slab_ins, 4, **kw)
      assert (dev.download(res, (32,), np.uint8) == 0xA5).all()
      assert prog.last_launches()[0] == 0
      with pytest.raises(util.InputError, match='batch'):
        prog.run_device([res], [res], local, 4, batch=2, residual=res)


@pytest.mark.gpu
def test_sodac_until_on_two_virtual_gpus(built):
  """`sodac --hip-backend --hip-gpus 2 --hip-virtual --hip-until TOL` prints
  the iteration count and the struct of the one-GPU form, for the same program
  and input; `--hip-residual` with `--hip-gpus` prints the combined struct of
  the whole run."""
  import json
  import subprocess
  import sys
  from conftest import ROOT

  def run(*flags):
    r = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', *flags],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])

  base = [soda_path('jacobi2d.soda'), '--iterate', '64', '--border', 'preserve',
          '--hip-backend', '--hip-extent', '64', '40']
  until = ['--hip-until', '0.003', '--hip-check-every', '16']
  one = run(*base, *until)
  two = run(*base, *until, '--hip-gpus', '2', '--hip-virtual')
  assert one['iterations'] == two['iterations']
  assert one['iterations'] in (16, 32, 48), 'the tolerance never stopped it'
  assert two['residual'] == one['residual'] and one['residual']['changed'] > 0
  assert two['checksum'] == one['checksum']
  assert two['gpus'] == 2
  whole = run(*base, '--hip-residual', '--hip-gpus', '2', '--hip-virtual')
  stencil = _stencil('jacobi2d.soda', iterate=64, border='preserve')
  rng = np.random.default_rng(0)
  ins = {'t1': rng.random((40, 64), dtype=np.float64).astype(np.float32)}
  want, _ = _want('sodac', stencil, ins, (64, 40), 64)
  assert (whole['residual']['changed'], whole['residual']['unordered'],
          whole['residual']['max_float'], whole['residual']['max_int']) == want
