"""The steps a marching kernel's schedule is built in, one at a time
(soda_amd/codegen/hip/march_schedule.py), and the boundary between the
schedule and its text (march.py).  Nothing here needs a GPU, the library or a
compiler; that the generated text itself is what it was is the business of
tools/codegen_snapshot.py."""
import functools

import pytest

import knobs
from conftest import soda_path
from soda_amd import core, util


def _state(mod):
  return (mod.kernels, list(mod.kernels), mod.passes, list(mod.passes),
          mod.chunks, list(mod.chunks), mod.source)


def _same_state(mod, before):
  kernels, ks, passes, ps, chunks, cs, source = before
  return (mod.kernels is kernels and mod.passes is passes and
          mod.chunks is chunks and mod.kernels == ks and mod.passes == ps and
          mod.chunks == cs and mod.source == source)


def _schedule(st, slots=None, **ckw):
  from soda_amd.codegen.hip import lower, march_schedule
  mod = lower.Module(st, slots)
  return march_schedule.Schedule(st, lower.MarchConfig(**ckw), mod.banks,
                                 mod.slot)


@functools.lru_cache(maxsize=None)
def _deepest(prog):
  """(module of the default row, its deepest kernel, the program as lowered,
  the MarchConfig of that kernel)."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  st = knobs.stencil_of(prog)
  mod = knobs.lowered(prog, {})
  k = knobs.deepest(mod)
  opts = runtime.resolve_options(
      st, lower.LowerOptions(**knobs.keywords(prog, {})), None,
      probe=False).resolved(st.dim, iterated=st.iterate > 1)
  derived = lower._derive(st, opts)
  cfg = lower.march_config(
      opts, derived, k.tune['fused'], k.tune['vec'], knobs._prefetch_of(k),
      k.tune['tile_rows'] if st.dim == 3 else None)
  return mod, k, derived, cfg


# ---------------------------------------------------------------------------
# schedule and text
# ---------------------------------------------------------------------------

def test_a_schedule_writes_nothing_and_the_text_decides_nothing():
  from soda_amd.codegen.hip import lower, march, march_schedule
  # (the schedule's module knows neither the Module nor its descriptors)
  assert not any(hasattr(march_schedule, n)
                 for n in ('Module', 'KernelDesc', 'PassDesc'))
  _, built, derived, cfg = _deepest('jacobi2d_T4')
  mod = lower.Module(derived)
  before = _state(mod)
  s = march_schedule.Schedule(derived, cfg, mod.banks, mod.slot)
  assert _same_state(mod, before) and mod.source == before[-1]
  assert s.name == built.name
  assert not any(isinstance(v, str) and '\n' in v for v in vars(s).values())
  # the kernel object builds the same schedule and no text yet ...
  k = march._MarchKernel(mod, cfg)
  assert _same_state(mod, before) and k.L == [] and k.shift_temps == 0
  names, names_s = set(vars(k)), set(vars(k.s))
  values = {a: v for a, v in vars(k.s).items()
            if isinstance(v, (int, float, str, tuple))}
  p = k.emit()
  # ... and emission assigns no attribute first, and changes no value of the
  # schedule: only the line list and the counter of shifted operands move
  assert set(vars(k)) == names and set(vars(k.s)) == names_s
  assert {a: getattr(k.s, a) for a in values} == values
  assert k.L and k.shift_temps > 0
  assert mod.passes == [p] and mod.kernels[0].name == built.name
  assert mod.chunks == ['\n'.join(k.L) + '\n']


# (strip lanes, halo lanes, warm, unroll, peeled, peel_trips_max, estimated
# window registers without the shifted operands, and with them as published):
# recorded from the output of the commit BEFORE the schedule became a module of
# its own -- the `strip:` line of the kernel's text, its `tune` and its pass's
# `traffic_model` -- so they hold the steps to what the one constructor gave
PUBLISHED = {
    'jacobi2d_T12': (52, (3, 3), 24, 9, 0, 3, 196),
    'jacobi2d_T4': (62, (1, 1), 8, 9, 0, 1, 84),
    'blur': (63, (0, 1), 8, 9, 0, 1, 192),
    'coupled2d': (62, (1, 1), 4, 12, 0, 1, 146),
    'heat3d': (62, (1, 1), 4, 12, 0, 1, 236),
}


@pytest.mark.parametrize('prog', sorted(PUBLISHED))
def test_schedule_values_are_the_published_ones(prog):
  from soda_amd.codegen.hip import lower, march
  mod, built, derived, cfg = _deepest(prog)
  k = march._MarchKernel(lower.Module(derived), cfg)
  s = k.s
  k.emit()
  tune, model = built.tune, knobs._pass_of(mod, built).traffic_model
  assert s.name == built.name
  got = (s.strip_lanes, (s.lanes_lo, s.lanes_hi), s.warm, s.U, s.peeled,
         s.peel_trips_max, s.est_regs + k.shift_temps)
  assert got == PUBLISHED[prog]
  # ... and what the built kernel publishes
  assert s.strip_lanes * tune['vec'] == model['strip_cells'] == s.strip_cells
  assert tune['lane_redundancy'] == 64.0 / s.strip_lanes
  assert s.strip_lanes == (s.group - s.lanes_lo - s.lanes_hi) * (64 // s.group)
  assert s.warm == tune['warm'] == model['warm_rows']
  assert s.U == tune['unroll'] == model['unroll']
  assert s.peeled == tune['peel_trips'] * s.U
  assert s.peel_trips_max == tune['peel_trips_max']
  assert s.est_regs + k.shift_temps == model['est_window_regs']
  assert 0 < s.est_regs <= model['est_window_regs']
  assert (s.rows_in, s.tile_rows) == (model['rows_in'], model['tile_rows'])
  assert s.edge == tuple(model['edge'])


# ---------------------------------------------------------------------------
# the steps
# ---------------------------------------------------------------------------

def _shape(nodes):
  return [(n.var, n.delay, n.window, n.margin, n.omargin, n.rmargin)
          for n in nodes]


def test_edge_cells_are_taken_only_where_they_save_a_halo_lane():
  from soda_amd.codegen.hip import march_schedule
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  # one iteration reaches one cell: fetched by the edge lanes, every lane of
  # the strip stores
  one = _schedule(st, fused_iters=1, vec=4, prefetch=8)
  assert one.edge == (1, 1) and one.n_edge == 1
  assert (one.lanes_lo, one.lanes_hi, one.strip_lanes) == (0, 0, 64)
  assert [n.margin for n in one.inputs.values()] == [[-1, -1]]
  assert _schedule(st, fused_iters=1, vec=4, prefetch=8,
                   edge_loads=False).strip_lanes == 62
  # four iterations reach four cells, three with edge cells: one lane of four
  # cells a side either way, so the kernel is the plain chain's
  four = _schedule(st, fused_iters=4, vec=4, prefetch=4)
  assert four.edge == (0, 0) and four.n_edge == 0
  assert (four.lanes_lo, four.lanes_hi) == (1, 1)
  plain = march_schedule._build_chain(st, 4, 4, (0, 0))
  assert _shape(four.nodes) == _shape(plain[0])
  assert [n.margin for n in four.out_nodes] == [[4, 4]]
  # (the cells the header names stay those of the chain tried first)
  assert (four.margin_lo, four.margin_hi) == (3, 3)
  # the step alone answers the same
  edge, chain, halo = four._edge_cells()
  assert edge == (0, 0) and halo == (3, 3)
  assert _shape(chain[0]) == _shape(plain[0])


class _Stage:
  """As much of a core.Stage as a _Node asks for."""

  def __init__(self, name, taps):
    self.name, self.taps, self.st_idx = name, taps, (0, 0, 0)

  def tap_bounds(self, pname):
    offs = self.taps[pname]
    return (tuple(min(o[d] for o in offs) for d in range(3)),
            tuple(max(o[d] for o in offs) for d in range(3)))


def test_the_backward_walk_on_a_chain_with_a_mirror():
  from soda_amd.codegen.hip.march_schedule import _Node, _walk_back
  a = _Node(('in', 'a'), 'float', None, -1)
  b = _Node(('b', 0), 'float', _Stage('b', {
      'a': [(0, -1, -1), (0, 1, 0), (1, 0, 2)]}), 0)
  b.parents = {'a': a}
  d = _Node(('d', 0), 'float', _Stage('d', {'a': [(0, 0, 0)]}), 0)
  d.parents = {'a': a}                 # read by nobody
  m = _Node(('mirror', b.key, 1), 'float', None, 1)
  m.mirror_of, m.owner = b, 1
  c = _Node(('c', 1), 'float', _Stage('c', {
      'm': [(0, 0, -2), (0, 2, 0)], 'a': [(0, -3, -5), (0, 0, 0)]}), 1)
  c.parents = {'m': m, 'a': a}
  nodes = [a, b, d, m, c]
  # rows [1, 5) of the output: c reads rows +0 .. +2 of m -> [1, 7), the same
  # of b behind the mirror; b reads rows -1 .. +1 of a -> [0, 8); c itself
  # reads rows -3 .. 0 of a -> [-2, 5); together [-2, 8)
  rows = _walk_back(
      nodes, {id(c): (1, 5)},
      lambda v, lo, hi: (v[0] + lo[1], v[1] + hi[1]),
      lambda old, new: (min(old[0], new[0]), max(old[1], new[1])))
  assert [rows[id(n)] for n in nodes] == \
      [(-2, 8), (1, 7), None, (1, 7), (1, 5)]
  # plane 0 of the output: plane -2 of m and b, through b plane -3 of a,
  # straight from c plane -5 of a
  planes = _walk_back(nodes, {id(c): 0}, lambda v, lo, hi: v + lo[2], min)
  assert [planes[id(n)] for n in nodes] == [-5, -2, None, -2, 0]


@pytest.mark.parametrize('prog', sorted(knobs.PROGRAMS))
def test_a_stage_that_entered_the_warm_up_is_never_dropped_again(prog):
  """What the sliding sums rest on: stage_needed(n, step) is monotone in
  `step`, for every stage at the program's deepest fusion depth."""
  from soda_amd.codegen.hip import lower, march_schedule
  _, built, derived, cfg = _deepest(prog)
  mod = lower.Module(derived)
  s = march_schedule.Schedule(derived, cfg, mod.banks, mod.slot)
  assert s.name == built.name and s.T == knobs.deepest_depth(prog)
  stages = [n for n in s.nodes if n.stage is not None]
  assert stages
  steps = s.warm + 3 * s.U
  for n in stages:
    needed = [s.stage_needed(n, i) for i in range(steps)]
    assert needed == sorted(needed), (n.var, needed)
  # every output's stage is needed once the warm-up is over
  assert all(s.stage_needed(n, steps - 1) for n in s.out_nodes)


REFUSALS = [
    ('heat4d.soda', {}, dict(fused_iters=1), None, '2- or 3-dimensional'),
    ('denoise2d.soda', {}, dict(fused_iters=2), None,
     'march: cannot fuse iterations of a program whose inputs and outputs '
     'differ in number'),
    ('jacobi2d.soda', dict(iterate=8), dict(fused_iters=3, pipe=2), None,
     'march: 2 pipelined waves need a fusion depth that is a multiple of it '
     'and one strip per block'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, pipe=2, waves_y=2), None,
     'march: 2 pipelined waves need'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, pipe=2, banks={'t1': 2}), {'t1': 2},
     'march: stage-pipelined blocks read and write dense arrays'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, vec=2, banks={'t1': 4}), {'t1': 4},
     'banks: 2 cells per lane are no whole number of groups of 4 banks'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, banks={'t1': 2}, bank_lead={'t1': 3}), {'t1': 2},
     'march: bank_lead of `t1`: a banked input, a multiple of its bank count'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, vec=4, prefetch=4, pipe=2, pipe_rows=3, tile_rows=4),
     None, 'march: rows per barrier must be a power of two'),
    ('jacobi2d.soda', dict(iterate=8), dict(fused_iters=4, xshare_block=17),
     None, 'march: xshare_block = 17: 2 to 16 waves share a segment of a row'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=2, lane_shift='mixh'), None,
     'march: x-halo sharing needs DPP shifts and one wave per strip'),
    ('jacobi2d.soda', dict(iterate=8), dict(fused_iters=4, xshare=17), None,
     'march: 1 to 16 waves can share a row'),
    ('heat3d.soda', dict(iterate=3),
     dict(fused_iters=2, prefetch=1, xshare=2, tile_rows=25), None,
     'march: x-halo sharing holds a row per lane'),
    ('jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, waves_y=2, residual=True), None,
     'march: no residual twin of stage-pipelined blocks, segmented x-halo '
     'sharing, several waves per block or banked tensors'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=lambda c: c[4][:40])
def test_the_config_check_refuses_what_it_refused(case):
  soda, skw, ckw, slots, text = case
  st = core.from_file(soda_path(soda), **skw)
  s = _schedule(core.from_file(soda_path('jacobi2d.soda'), iterate=8),
                fused_iters=4)
  for build in (lambda: _schedule(st, slots, **ckw),
                # ... and by the step alone, before any chain exists
                lambda: type(s)._check_config(_blank(st, ckw), slots or {})):
    with pytest.raises(util.SemanticError) as err:
      build()
    assert str(err.value).startswith(text) or text in str(err.value)


def _blank(st, ckw):
  from soda_amd.codegen.hip import lower, march_schedule
  s = march_schedule.Schedule.__new__(march_schedule.Schedule)
  s.st, s.cfg = st, lower.MarchConfig(**ckw)
  return s


def test_the_config_check_and_the_modules_slots():
  """Bank counts that differ from the module's are the caller's mistake, not
  the program's: an InternalError, and the first thing said about a tensor."""
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  with pytest.raises(util.InternalError, match='slots differ'):
    _schedule(st, {'t1': 4}, fused_iters=4, pipe=2, banks={'t1': 2})
  # a config that passes sets what the config alone decides
  s = _blank(st, dict(fused_iters=4, pipe=2, pipe_rows=4, lane_shift='mixh'))
  assert s._check_config({}) is None
  assert (s.T, s.W, s.R, s.group, s.one_wave, s.xs, s.seg) == \
      (4, 2, 4, 32, True, 0, False)
  assert not hasattr(s, 'nodes')
