"""The steps lower() is made of, one at a time (soda_amd/codegen/hip/lower.py),
and the memo helper of the probing code in soda_amd/runtime.py.  Nothing here
needs a GPU, the library or a compiler."""
import json
import os

import pytest

import knobs
from conftest import soda_path
from soda_amd import core, util


def _resolved(stencil, **kw):
  from soda_amd.codegen.hip import lower
  return lower.LowerOptions(**kw).resolved(stencil.dim,
                                           iterated=stencil.iterate > 1)


def _state(mod):
  return (mod.kernels, list(mod.kernels), mod.passes, list(mod.passes),
          mod.chunks, list(mod.chunks), mod.source)


def _same_state(mod, before):
  kernels, ks, passes, ps, chunks, cs, source = before
  return (mod.kernels is kernels and mod.passes is passes and
          mod.chunks is chunks and len(mod.kernels) == len(ks) and
          all(a is b for a, b in zip(mod.kernels, ks)) and
          len(mod.passes) == len(ps) and
          all(a is b for a, b in zip(mod.passes, ps)) and
          mod.chunks == cs and mod.source == source)


# ---------------------------------------------------------------------------
# _add_march: a pass and its twin, or nothing
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('residual', [False, True])
def test_add_march_rolls_back_what_the_generator_refuses(residual):
  from soda_amd.codegen.hip import lower
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  opts = _resolved(st, fuse=(4,), peel=0)
  mod = lower.Module(st, None, False, residual)
  # a config that fits: one pass, and the twin the plain kernel names
  assert lower._add_march(mod, lower.march_config(opts, st, 1, 4, 8), residual)
  assert [p.fused_iters for p in mod.passes] == [1]
  plain = mod.kernels[mod.passes[0].kernels[0]]
  if residual:
    assert len(mod.kernels) == 2 and plain.twin == 1
    assert mod.kernels[1].name == plain.name + '_rs'
    assert mod.kernels[1].tune['twin_of'] == plain.name
  else:
    assert len(mod.kernels) == 1 and plain.twin == -1
  # one the generator refuses: three row steps per barrier
  bad = lower.MarchConfig(fused_iters=4, vec=4, prefetch=4, pipe=2,
                          pipe_rows=3, tile_rows=4)
  with pytest.raises(util.SemanticError, match='power of two'):
    lower.add_march_pass(lower.Module(st), bad)
  before = _state(mod)
  assert lower._add_march(mod, bad, residual) is False
  assert _same_state(mod, before)
  # ... and the module still takes the next one
  assert lower._add_march(mod, lower.march_config(opts, st, 4, 4, None),
                          residual)
  assert [p.fused_iters for p in mod.passes] == [1, 4]
  assert len(mod.kernels) == (4 if residual else 2)
  fused = mod.kernels[mod.passes[1].kernels[0]]
  assert fused.twin == (3 if residual else -1)


def test_add_march_rolls_back_a_refusal_after_kernels_were_added():
  """A wide halo is refused late, by the kernel's own geometry: whatever the
  generator appended before it raised is taken out again."""
  from soda_amd.codegen.hip import lower
  st = knobs.stencil_of('jacobi2d_T12')
  opts = _resolved(st, fuse=(12,), peel=0)
  mod = lower.Module(st)
  assert lower._add_march(mod, lower.march_config(opts, st, 1, 4, 8), False)
  before = _state(mod)
  # twelve iterations at one cell per lane: 12 + 12 halo lanes of a 32-lane
  # half strip (knobs.INADMISSIBLE)
  cfg = lower.march_config(opts, st, 12, 1, None)
  assert cfg.lane_shift == 'mixh'
  assert lower._add_march(mod, cfg, False) is False
  assert _same_state(mod, before)


# ---------------------------------------------------------------------------
# _one_iteration_shape
# ---------------------------------------------------------------------------

def _estimate(stencil, opts, vec, pf):
  from soda_amd.codegen.hip import lower
  trial = lower.Module(stencil)
  return lower.add_march_pass(
      trial, lower.march_config(opts, stencil, 1, vec, pf)).traffic_model[
          'est_window_regs']


# the candidates in the order they are tried: 16 bytes per lane halved down to
# one cell; 2-D below 128 operations per cell 8, 2, 1 rows in flight, 3-D the
# one plane LowerOptions.resolved fixes
CANDIDATES = {
    'jacobi2d_T4': [(v, pf) for v in (4, 2, 1) for pf in (8, 2, 1)],
    'heat3d': [(4, 1), (2, 1), (1, 1)],
}


@pytest.mark.parametrize('prog', sorted(CANDIDATES))
def test_one_iteration_shape(prog):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  st = knobs.stencil_of(prog)
  lean = knobs.REG_BUDGET_LEAN[prog]
  opts = runtime.resolve_options(
      st, lower.LowerOptions(**knobs.keywords(prog, {'reg_budget': 'lean'})),
      None, probe=False)
  built = knobs._one(lower.lower(st, opts))
  opts = opts.resolved(st.dim, iterated=True)
  opts.vec = None        # the candidates start at 16 bytes per lane
  work = lower.ops_per_cell(st)
  derived = lower._derive(st, opts)
  ests = [_estimate(derived, opts, v, pf) for v, pf in CANDIDATES[prog]]
  # the lean budget: the first candidate within it, which lower() builds
  shape, refusal = lower._one_iteration_shape(derived, opts, work, lean)
  assert refusal is None
  first = [c for c, e in zip(CANDIDATES[prog], ests) if e <= lean][0]
  assert shape == first + (opts.tile_rows,)
  assert shape[:2] == (built.tune['vec'], knobs._prefetch_of(built))
  assert shape[:2] != CANDIDATES[prog][0]          # (the budget is lean)
  # the default budget: the preferred shape
  shape, _ = lower._one_iteration_shape(derived, opts, work, lower.REG_BUDGET)
  assert shape[:2] == CANDIDATES[prog][0]
  # no budget at all: the leanest estimate, the earlier of two alike
  shape, refusal = lower._one_iteration_shape(derived, opts, work, 0)
  assert refusal is None
  assert shape[:2] == CANDIDATES[prog][ests.index(min(ests))]
  assert min(ests) > 0


def test_one_iteration_shape_answers_none_with_the_last_refusal():
  from soda_amd.codegen.hip import lower
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  # two cells per lane, then one, are no whole groups of four banks
  opts = _resolved(st, strategy='march', fuse=(), vec=2, banks={'t1': 4})
  shape, refusal = lower._one_iteration_shape(st, opts, lower.ops_per_cell(st),
                                              lower.REG_BUDGET)
  assert shape is None
  assert isinstance(refusal, util.SemanticError)
  assert '1 cells per lane' in str(refusal) and '4 banks' in str(refusal)
  # ... which `march` raises and `auto` answers with its own refusal of banks
  with pytest.raises(util.SemanticError, match='1 cells per lane'):
    lower.lower(st, opts)
  opts.strategy = 'auto'
  with pytest.raises(util.SemanticError, match='`direct` kernels'):
    lower.lower(st, opts)


# ---------------------------------------------------------------------------
# peel_for, pipe_for, shift_for: functions of the options alone
# ---------------------------------------------------------------------------

def test_peel_for():
  from soda_amd.codegen.hip.lower import LowerOptions, peel_for
  assert peel_for(LowerOptions(), 12) == -1           # None: all the warm-up
  assert peel_for(LowerOptions(peel=2), 12) == 2
  assert peel_for(LowerOptions(peel=0), 1) == 0
  by_depth = LowerOptions(peel={12: 3, 4: 1})
  assert [peel_for(by_depth, t) for t in (12, 4, 8, 1)] == [3, 1, -1, -1]


def test_pipe_for():
  from soda_amd.codegen.hip.lower import LowerOptions, default_pipe, pipe_for
  assert [pipe_for(LowerOptions(), t) for t in (1, 4, 12)] == \
      [default_pipe(t) for t in (1, 4, 12)] == [1, 1, 1]
  assert pipe_for(LowerOptions(pipe=4), 12) == 4
  assert pipe_for(LowerOptions(pipe=2), 4) == 2
  # the waves do not divide the iterations; one iteration has none to share
  assert pipe_for(LowerOptions(pipe=4), 2) == 1
  assert pipe_for(LowerOptions(pipe=4), 13) == 1
  assert pipe_for(LowerOptions(pipe=2), 1) == 1
  # a block of several waves already
  assert pipe_for(LowerOptions(pipe=4, waves_x=2), 12) == 1
  assert pipe_for(LowerOptions(pipe=4, waves_y=2), 12) == 1
  assert pipe_for(LowerOptions(pipe=1), 12) == 1


def test_shift_for():
  from soda_amd.codegen.hip.lower import (LowerOptions, default_lane_shift,
                                          shift_for)
  plain = LowerOptions()
  # the default: `mixh` from eight fused iterations on, in 2-D only
  assert [shift_for(plain, 2, t) for t in (1, 4, 7, 8, 12, 13)] == \
      ['dpp', 'dpp', 'dpp', 'mixh', 'mixh', 'mixh']
  assert [shift_for(plain, 3, t) for t in (2, 8)] == ['dpp', 'dpp']
  assert all(shift_for(plain, d, t) == default_lane_shift(t, d)
             for d in (2, 3) for t in (1, 2, 8, 12))
  # blocks of several waves shift by DPP: shared x-halos, stage pipelines,
  # waves_x / waves_y
  assert shift_for(plain, 2, 12, 3) == 'dpp'
  assert shift_for(LowerOptions(pipe=4), 2, 12) == 'dpp'
  assert shift_for(LowerOptions(pipe=4), 2, 13) == 'mixh'   # (13 % 4: none)
  assert shift_for(LowerOptions(waves_x=2), 2, 12) == 'dpp'
  assert shift_for(LowerOptions(waves_y=4), 2, 12) == 'dpp'
  # what the caller asks for wins over all of it
  asked = LowerOptions(lane_shift='mixh', pipe=4, waves_x=2)
  assert shift_for(asked, 2, 12, 3) == 'mixh'
  assert shift_for(asked, 3, 1) == 'mixh'
  assert shift_for(LowerOptions(lane_shift='dpp'), 2, 12) == 'dpp'


def test_march_config_carries_the_options():
  from soda_amd.codegen.hip import lower
  st = knobs.stencil_of('jacobi2d_T12')
  opts = _resolved(st, fuse=(12,), peel={12: 2}, chunk_rows=16)
  cfg = lower.march_config(opts, st, 12, 4, None)
  assert (cfg.fused_iters, cfg.vec, cfg.lane_shift, cfg.peel, cfg.pipe) == \
      (12, 4, 'mixh', 2, 1)
  assert cfg.prefetch == lower.default_prefetch(12, 'mixh') == 4
  assert cfg.chunk_rows == 16 and cfg.chunk_fixed is True
  assert cfg.align_lanes == 1           # plain stores: nothing to align
  one = lower.march_config(_resolved(st, nt_store=True), st, 1, 4, 8)
  assert one.align_lanes == 64 // (4 * 4) and one.chunk_fixed is False
  assert one.chunk_rows == 64 and one.peel == -1 and one.prefetch == 8
  assert lower.march_config(_resolved(st, nt_store=True, align_lanes=2), st, 1,
                            4, 8).align_lanes == 2
  shared = lower.march_config(opts, st, 12, 4, None, xshare_block=2)
  assert shared.lane_shift == 'dpp' and shared.xshare_block == 2
  assert shared.prefetch == lower.default_prefetch(12, 'dpp') == 2


# ---------------------------------------------------------------------------
# ops_per_cell, same_boxes, check_options
# ---------------------------------------------------------------------------

def test_ops_per_cell_and_the_narrow_strips():
  from soda_amd.codegen.hip import lower
  denoise = core.from_file(soda_path('denoise2d.soda'))
  jacobi = core.from_file(soda_path('jacobi2d.soda'))
  assert lower.ops_per_cell(denoise) == 55
  assert lower.NARROW_STRIP_OPS[0] <= lower.ops_per_cell(denoise) < \
      lower.NARROW_STRIP_OPS[1]
  assert lower.ops_per_cell(jacobi) < lower.NARROW_STRIP_OPS[0]
  assert lower.prefers_narrow_strips(denoise) is True
  assert lower.prefers_narrow_strips(jacobi) is False


OFF_CENTRE = '''kernel: offc
burst width: 64
unroll factor: 2
iterate: 1
input float: in(32, *)
local float: loc(0, -1) = in(1, 0)
output float: out(0, 0) = loc(0, -1)
'''


def test_same_boxes_refuses_a_fold_that_moves_an_outputs_window():
  from soda_amd.codegen.hip import lower
  from soda_amd.optimization import pointwise
  jacobi = core.from_file(soda_path('jacobi2d.soda'))
  assert lower.same_boxes(jacobi, jacobi)
  st = core.from_text(OFF_CENTRE)
  folded = pointwise.inline_pointwise(st)
  assert len(folded.local_names) < len(st.local_names)
  assert not lower.same_boxes(st, folded)
  # ... so the derived program keeps the local
  derived = lower._derive(st, _resolved(st))
  assert list(derived.local_names) == list(st.local_names)


def test_check_options_names_the_first_rule_broken():
  from soda_amd.codegen.hip import lower
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  cases = [
      (dict(strategy='x', lane_shift='up'), "strategy 'x'"),
      (dict(lane_shift='up', xshare_block=1), "lane_shift 'up'"),
      (dict(xshare_block=17, pipe=2, pipe_rows=3), 'xshare_block 17'),
      (dict(pipe=2, pipe_rows=3, batch=True, banks={'t1': 2}), 'pipe_rows 3'),
      (dict(batch=True, banks={'t1': 2}, residual=True), 'batch: the wire'),
      (dict(batch=True, residual=True), 'residual: not together'),
      (dict(strategy='tile3d', banks={'t1': 2}), 'banks: `tile3d` kernels'),
      (dict(strategy='tile3d'), 'tile3d: tile3d needs a 3-dimensional'),
  ]
  for kw, start in cases:
    for call in (lambda o: lower.check_options(st, o),
                 lambda o: lower.lower(st, o)):
      with pytest.raises(util.SemanticError) as err:
        call(_resolved(st, **kw))
      assert str(err.value).startswith(start), (kw, str(err.value))
  assert lower.check_options(st, _resolved(st, pipe_rows=3)) is None


# ---------------------------------------------------------------------------
# runtime._memo, _fused_kernel
# ---------------------------------------------------------------------------

def test_memo_round_trip_garbage_and_an_unwritable_cache(tmp_path, monkeypatch):
  from soda_amd import runtime
  monkeypatch.setattr(runtime, 'CACHE_DIR', str(tmp_path / 'cache'))
  calls = []

  def compute():
    calls.append(1)
    return {12: 3, 4: 1}

  decode = lambda got: {int(t): int(v) for t, v in got.items()}
  # a miss computes, creates the directory and writes; a hit only reads
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  path = tmp_path / 'cache' / 'peel_x.json'
  assert json.loads(path.read_text()) == {'12': 3, '4': 1}
  assert os.listdir(str(tmp_path / 'cache')) == ['peel_x.json']   # no .tmp left
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  assert len(calls) == 1
  # `None` and a tuple go through encode / decode (select_shape's)
  enc = lambda found: list(found) if found else []
  dec = lambda got: tuple(got) if got else None
  assert runtime._memo('shape_a.json', lambda: (8, 2), enc, dec) == (8, 2)
  assert runtime._memo('shape_a.json', lambda: 1 / 0, enc, dec) == (8, 2)
  assert runtime._memo('shape_b.json', lambda: None, enc, dec) is None
  assert (tmp_path / 'cache' / 'shape_b.json').read_text() == '[]'
  assert runtime._memo('shape_b.json', lambda: 1 / 0, enc, dec) is None
  # garbage is a miss, and is overwritten
  path.write_text('{"12": 3, "4"')
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  assert len(calls) == 2
  assert json.loads(path.read_text()) == {'12': 3, '4': 1}
  path.write_text('')
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  assert len(calls) == 3 and json.loads(path.read_text()) == {'12': 3, '4': 1}
  # a cache that cannot be written (its directory is a file): computed, no error
  blocked = tmp_path / 'blocked'
  blocked.write_text('not a directory')
  monkeypatch.setattr(runtime, 'CACHE_DIR', str(blocked))
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  assert runtime._memo('peel_x.json', compute, decode=decode) == {12: 3, 4: 1}
  assert len(calls) == 5 and blocked.read_text() == 'not a directory'


def test_fused_kernel_finds_the_first_of_a_depth():
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  st = core.from_file(soda_path('jacobi2d.soda'), iterate=8)
  mod = lower.lower(st, lower.LowerOptions(fuse=(4,), peel=0, residual=True))
  four, one = runtime._fused_kernel(mod, 4), runtime._fused_kernel(mod, 1)
  assert four is mod.kernels[0] and '_T4_' in four.name
  assert one.tune['fused'] == 1
  assert not one.name.endswith('_rs')            # the kernel, not its twin
  assert runtime._fused_kernel(mod, 1, marching_only=True) is one
  assert runtime._fused_kernel(mod, 2) is None
  direct = lower.lower(st, lower.LowerOptions(strategy='direct'))
  assert runtime._fused_kernel(direct, 1, marching_only=True) is None


def test_extent_array_pads_to_four_dimensions():
  from soda_amd import runtime
  assert list(runtime._extent_array((7, 5))) == [7, 5, 1, 1]
  assert list(runtime._extent_array([3, 4, 5], fill=0)) == [3, 4, 5, 0]
  assert list(runtime._extent_array((2, 3, 4, 5))) == [2, 3, 4, 5]
