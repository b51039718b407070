"""Random programs on tori and bordered domains against nests that share
nothing with the product (tests/fuzz_nest.py: `run_torus`, `run_bordered`,
`reach`).

Every other domain test takes its expected value from tests/periodic.py and
tests/borders.py, which pad by Stencil.window_bounds, run the oracle that reads
the program through the product's front-end, and cut by Stencil.valid_box --
the derivation the product's own frames come from.  Here the expected value is
a loop nest emitted from the program's tree: on a torus every index modulo N,
between walls every input extended by the closed forms over a margin counted
from the tree.  Comparison is on bits, NaN == NaN.

CPU: the two helpers pinned on seeds 0-23 of three families; the product's
frames against the tree's reach; the fused scheme (tests/rims.py,
tests/domains.py) on random programs; a ledger of what the seeds cover.
GPU: A torus, B walls at depth 1, C walls fused, D batches, E residual and
norms."""
import numpy as np
import pytest

import borders
import domains
import fuzz_nest
import norms
import periodic
import rims

FAMILIES = ('plain', 'rich', 'window')
CPU_SEEDS = range(0, 24)
GPU_SEEDS = range(0, 12)
BATCH_SEEDS = range(0, 4)
PER_FAMILY_RESIDUAL = 4         # iterable seeds per family in part E
DEPTHS = (2, 3)
WALLS = ('clamp', 'constant', 'mirror', 'mirror101')
ROW_LENGTHS = (1, 3, 7, 12, 33, 70)
# cells of a domain whose every wall dimension is L + H wide; a dimension
# that would pass it wraps instead (window programs reach 20 cells and more)
CPU_CELLS, GPU_CELLS = 20000, 400000

_TREES = {}


def _tree(seed, family):
  """(tree, text, the product's stencil of that text)."""
  key = (seed, family)
  if key not in _TREES:
    from soda_amd import core
    prog, _ = fuzz_nest.program(seed, family)
    text = prog.soda_text()
    _TREES[key] = (prog, text, core.from_text(text))
  return _TREES[key]


def _iterates(seed, family):
  """The generator keeps what is undefined beyond int32 (float -> int) out of
  programs it iterates: only those run more iterations than their own."""
  prog, _ = fuzz_nest.program(seed, family)
  return prog.iterable() and prog.iterate >= 2


ITERABLE = [(s, f) for f in FAMILIES for s in CPU_SEEDS if _iterates(s, f)]
GPU_ITERABLE = [(s, f) for s, f in ITERABLE if s in GPU_SEEDS]
# part E: four per family -- 1-D, 2-D and 3-D, mixed cell types (rich 1), and
# programs whose lowering keeps two iterations in a launch
RESIDUAL = [(2, 'plain'), (3, 'plain'), (7, 'plain'), (11, 'plain'),
            (1, 'rich'), (5, 'rich'), (7, 'rich'), (11, 'rich'),
            (1, 'window'), (3, 'window'), (5, 'window'), (9, 'window')]
# part C at L + H - 1: programs that run two deep at L + H, 2-D and 3-D
ONE_BELOW = [(2, 'plain'), (7, 'rich'), (5, 'window'), (9, 'window')]
# part C on fuse=(3,): the programs whose lowering keeps three in a launch
FUSE3 = [(8, 'plain'), (5, 'rich'), (7, 'rich'), (8, 'rich')]


def _same(a, b):
  """Bit for bit; a NaN on both sides counts as equal."""
  if a.dtype != b.dtype or a.shape != b.shape:
    return False
  if a.dtype.kind != 'f':
    return bool((a == b).all())
  bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
  eq = np.ascontiguousarray(a).view(bits) == np.ascontiguousarray(b).view(bits)
  return bool((eq | (np.isnan(a) & np.isnan(b))).all())


def _assert_same(got, want, what, text=''):
  assert sorted(got) == sorted(want)
  for o in want:
    assert _same(got[o], want[o]), '%s, output %s: %d of %d cells differ\n%s' % (
        what, o, periodic.differing(got[o], want[o]), want[o].size, text)


def _modes(seed, family, dim, shift=0):
  fi = FAMILIES.index(family)
  return tuple(fuzz_nest.MODES[(seed + fi + d + shift) % 5] for d in range(dim))


def _mixed(seed, family, dim):
  """`wrap` in one dimension, one wall mode in the others."""
  fi = FAMILIES.index(family)
  wall = WALLS[(seed + fi) % len(WALLS)]
  return tuple('wrap' if d == seed % dim else wall for d in range(dim))


def _constants(prog):
  """Small, distinct, nonzero, exact in every cell type."""
  return {n: 3 + 2 * i for i, (n, _) in enumerate(prog.inputs)}


def _cpu_extent(seed, family, dim):
  """8-28 x 5-13 (x 5-13) cells; every sixth seed 1-3 cells a side, narrower
  than most programs reach."""
  rng = np.random.default_rng(seed * 3 + FAMILIES.index(family) + 70000)
  if seed % 6 == 5:
    return tuple(int(rng.integers(1, 4)) for _ in range(dim))
  return (int(rng.integers(8, 29)),) + tuple(
      int(rng.integers(5, 14)) for _ in range(dim - 1))


def _gpu_extent(seed, family, dim):
  """Rows of 1, 3, 7, 12, 33 or 70 cells -- odd, shorter than a 16-byte
  fragment, a ghost_hi[0] rounded past the domain --, 2-9 cells elsewhere."""
  fi = FAMILIES.index(family)
  return (ROW_LENGTHS[(seed + fi) % len(ROW_LENGTHS)],) + tuple(
      2 + (3 * seed + 5 * d + fi) % 8 for d in range(1, dim))


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('peel', 0)
  return lower.LowerOptions(**kw)


def _plan(stencil, **kw):
  """The launch plan of a program, lowered without trial compilations."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, _opts(**kw), None, probe=False)
  return runtime.make_plan(lower.lower(stencil, opts))


def _fused_ghosts(st, modes, depth):
  """border_fused_ghosts, or None where it refuses -- with its own message."""
  from soda_amd import runtime, util
  try:
    return runtime.border_fused_ghosts(st, modes, depth)
  except util.InputError as e:
    assert 'reach more than' in str(e) and 'times what one' in str(e), str(e)
    return None


def _fused_geometry(st, plan, seed, family, depth, cells, below=False):
  """(modes, extent, ghosts) of a fused run whose every wall dimension is
  exactly L + H wide, L and H read from border_fused_plan on a roomy domain;
  None where border_fused_ghosts refuses the program.  Wall dimensions are
  kept, dimension 0 first, while the domain stays under `cells`; the others
  wrap.  `below`: the first wall dimension one cell narrower."""
  from soda_amd import runtime
  dim = st.dim
  modes = list(_modes(seed, family, dim))
  small = [5 + (seed + d) % 3 for d in range(dim)]
  for _ in range(dim + 1):
    ghosts = _fused_ghosts(st, modes, depth)
    if ghosts is None:
      return None
    rlo, rhi, lo, hi = ghosts
    roomy = tuple(8 * depth * (a + b) + 9 for a, b in zip(rlo, rhi))
    info, _ = runtime.border_fused_plan(plan, roomy, modes, depth, rlo, rhi,
                                        lo, hi)
    assert info['depth'] == depth, (info['depth'], depth)
    extent = list(small)
    for s in info['strips']:
      extent[s['dim']] = s['lo'] + s['hi']
    if int(np.prod(extent)) <= cells or not info['strips']:
      break
    widest = max(info['strips'], key=lambda s: s['lo'] + s['hi'])['dim']
    modes[widest] = 'wrap'
  if below and info['strips']:
    extent[info['strips'][0]['dim']] -= 1
  return tuple(modes), tuple(extent), ghosts


# ---------------------------------------------------------------------------
# CPU: the helpers every other domain test rests on
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('seed', CPU_SEEDS)
def test_the_helpers_are_the_independent_nests(seed, family):
  """periodic.expected is the torus nest, borders.expected the bordered nest
  under a mode per dimension, on every output, whole arrays."""
  prog, text, st = _tree(seed, family)
  extent = _cpu_extent(seed, family, prog.dim)
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  _assert_same(periodic.expected(st, ins, prog.iterate),
               prog.run_torus(ins, extent), 'torus %s' % (extent,), text)
  modes, cst = _modes(seed, family, prog.dim), _constants(prog)
  _assert_same(borders.expected(st, ins, prog.iterate, modes, cst),
               prog.run_bordered(ins, extent, modes, cst),
               'walls %s %s' % (extent, modes), text)


def test_the_closed_forms_restated():
  """fuzz_nest.extend against np.pad, the third statement of the table."""
  rng = np.random.default_rng(5)
  for shape, lo, hi in (((7,), (3,), (9,)), ((1, 4), (2, 5), (0, 3)),
                        ((3, 2, 5), (4, 0, 7), (1, 6, 2))):
    arr = rng.integers(0, 250, size=shape).astype(np.int16)
    for shift in range(5):
      modes = tuple(fuzz_nest.MODES[(d + shift) % 5] for d in range(arr.ndim))
      want = arr
      for d, m in enumerate(modes):
        width = [(0, 0)] * arr.ndim
        width[arr.ndim - 1 - d] = (lo[d], hi[d])
        kw = dict(constant_values=-7) if m == 'constant' else {}
        want = np.pad(want, width, mode=borders.NUMPY[m], **kw)
      got = fuzz_nest.extend(arr, lo, hi, modes, -7)
      assert got.dtype == arr.dtype and (got == want).all(), (shape, modes)


def test_the_frames_are_the_trees_reach(capsys):
  """periodic_ghosts(stencil, k) is Program.reach(k) in every dimension but
  the last and at least that in the last (where the plan's reach counts too);
  border_fused_ghosts accepts a program or refuses it in its own words."""
  from soda_amd import runtime
  accepted = refused = 0
  for family in FAMILIES:
    for seed in CPU_SEEDS:
      prog, text, st = _tree(seed, family)
      for k in (1, 2, 3):
        if k > 1 and not prog.iterable():
          continue
        lo, hi = runtime.periodic_ghosts(st, k)
        rlo, rhi = prog.reach(k)
        assert lo[:-1] == rlo[:-1] and hi[:-1] == rhi[:-1], (k, text)
        assert lo[-1] >= rlo[-1] and hi[-1] >= rhi[-1], (k, text)
        if k == 1:
          assert (lo, hi) == runtime.border_ghosts(st, 'clamp')
          continue
        ghosts = _fused_ghosts(st, _modes(seed, family, prog.dim), k)
        if ghosts is None:
          refused += 1
        else:
          accepted += 1
          assert ghosts[:2] == runtime.periodic_ghosts(st, 1)
  with capsys.disabled():
    print('\nborder_fused_ghosts on random programs: %d accepted, %d refused'
          % (accepted, refused))
  assert accepted >= 20


# ---------------------------------------------------------------------------
# CPU: the fused scheme on random programs, from the plan's numbers alone
# ---------------------------------------------------------------------------

def _nest_numbers(prog, cur, prev):
  """(residual tuple, norms dict or None) of the nest's two last states; the
  norms only where all cells are of one type (one accumulator holds one kind
  of units: the product serves no other)."""
  res = domains.fold(domains.delta(cur[s.name], prev[s.name])
                     for s in prog.outputs)
  if len({t for _, t in prog.inputs} | {s.typ for s in prog.outputs}) > 1:
    return res, None
  acc = None
  for s in prog.outputs:
    acc = norms.oracle(cur[s.name], prev[s.name], acc)
  return res, acc


@pytest.mark.parametrize('depth', DEPTHS)
@pytest.mark.parametrize('seed,family', ITERABLE,
                         ids=['%s%d' % (f, s) for s, f in ITERABLE])
def test_the_fused_scheme_on_random_programs(built, seed, family, depth):
  """rims.emulate (interior spoiled outside its valid box, strips scattered by
  the plan's widths) gives the bordered nest's bits, domains.emulate (deltas
  over the trusted box and the rims) the residual and the norms of the nest's
  two last states -- every wall dimension L + H wide, with 1, T - 1 and T
  iterations in the last chunk."""
  from soda_amd import runtime
  prog, text, st = _tree(seed, family)
  plan = _plan(st, fuse=(depth,))
  found = _fused_geometry(st, plan, seed, family, depth, CPU_CELLS)
  if found is None:
    return              # refused in its own words: counted by the ledger
  modes, extent, (rlo, rhi, lo, hi) = found
  cst = _constants(prog)
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  args = (plan, extent, modes, depth, rlo, rhi, lo, hi)
  boxes = runtime.border_fused_residual_boxes(*args)
  for last in sorted({1, depth - 1, depth}):
    iterate = last if last == depth else depth + last
    info, chunks = runtime.border_fused_plan(*args, iterate)
    assert info['depth'] == boxes['depth'] == depth and chunks[-1] == last
    for s in info['strips']:
      assert extent[s['dim']] == s['lo'] + s['hi']
    what = '%s%d depth %d, %s %s, %d iterations' % (family, seed, depth,
                                                    extent, modes, iterate)
    cur, prev = prog.run_bordered(ins, extent, modes, cst, iterate=iterate,
                                  with_previous=True)
    _assert_same(rims.emulate(st, ins, modes, cst, info, chunks), cur, what,
                 text)
    got_res, got_norms = None, None
    want_res, want_norms = _nest_numbers(prog, cur, prev)
    if want_norms is not None:
      got_res, got_norms = domains.emulate(st, ins, modes, cst, info, boxes,
                                           chunks)
      assert got_res == want_res and got_norms == want_norms, what


# ---------------------------------------------------------------------------
# CPU: what the chosen seeds cover
# ---------------------------------------------------------------------------

def test_coverage_ledger(built, capsys):
  """A change of the generator cannot hollow this file out."""
  from soda_amd import runtime
  seen = {d: set() for d in range(3)}
  dims, one_sided, lopsided, mixed_sizes, odd_rows = set(), 0, 0, 0, 0
  narrow = {f: 0 for f in FAMILIES}
  for family in FAMILIES:
    for seed in CPU_SEEDS:
      prog, _, _ = _tree(seed, family)
      dims.add(prog.dim)
      for d, m in enumerate(_modes(seed, family, prog.dim)):
        seen[d].add(m)
      a, b = prog.reach(1)
      one_sided += any(x + y > 0 and 0 in (x, y) for x, y in zip(a, b))
      lopsided += any(x != y for x, y in zip(a, b))
      mixed_sizes += len({np.dtype(fuzz_nest.NPTYPES[t]).itemsize
                          for _, t in prog.inputs}) > 1
      extent = _cpu_extent(seed, family, prog.dim)
      odd_rows += extent[0] % 2
      klo, khi = prog.reach(prog.iterate)
      narrow[family] += any(n < max(l, h)
                            for n, l, h in zip(extent, klo, khi))
  for d in range(3):
    assert seen[d] == set(fuzz_nest.MODES), (d, seen[d])
  assert dims == {1, 2, 3}
  assert one_sided >= 8 and lopsided >= 8, (one_sided, lopsided)
  assert mixed_sizes >= 3, mixed_sizes
  # ... and on the GPU's seeds: a fill launch per cell size, blockIdx.y the
  # tensor
  assert sum(len({np.dtype(fuzz_nest.NPTYPES[t]).itemsize
                  for _, t in _tree(s, f)[0].inputs}) > 1
             for f in FAMILIES for s in GPU_SEEDS) >= 3
  assert {_tree(s, f)[0].dim for f in FAMILIES for s in GPU_SEEDS} == {1, 2, 3}
  assert odd_rows >= 12 and all(n >= 1 for n in narrow.values()), (odd_rows,
                                                                   narrow)
  # the fused form: what the plan resolves to when the program is lowered with
  # fuse=(T,) and asked for depth 0, as part C asks
  deep = served = 0
  for seed, family in ITERABLE:
    prog, _, st = _tree(seed, family)
    plan = _plan(st, fuse=(2,))
    deepest = max(p.fused_iters for p in plan.passes[:plan.num_passes])
    found = _fused_geometry(st, plan, seed, family, 2, CPU_CELLS)
    if found is None:
      continue
    served += 1
    modes, extent, (rlo, rhi, lo, hi) = found
    info, _ = runtime.border_fused_plan(plan, extent, modes, 0, rlo, rhi, lo,
                                        hi) if deepest == 2 else ({'depth': 1},
                                                                  None)
    deep += info['depth'] >= 2
  with capsys.disabled():
    print('\n%d iterable programs, %d served by the fused form, %d at depth '
          '>= 2; one-sided %d, a != b %d, mixed cell sizes %d, narrow %s' % (
              len(ITERABLE), served, deep, one_sided, lopsided, mixed_sizes,
              narrow))
  assert deep >= 10, deep
  # nothing above is skipped; what border_fused_ghosts refuses is asserted
  # refused, and must stay under a tenth of the iterable programs
  assert 10 * (len(ITERABLE) - served) < len(ITERABLE)
  assert len(ITERABLE) >= 24 and len(GPU_ITERABLE) >= 12
  assert len(RESIDUAL) == PER_FAMILY_RESIDUAL * len(FAMILIES)
  assert all(sum(f == g for _, g in RESIDUAL) == PER_FAMILY_RESIDUAL
             for f in FAMILIES)
  for chosen in (RESIDUAL, ONE_BELOW, FUSE3):
    assert set(chosen) <= set(GPU_ITERABLE) and len(set(chosen)) == len(chosen)
  assert len(ONE_BELOW) == len(FUSE3) == 4


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_PROGRAMS = {}


@pytest.fixture(scope='module')
def programs(built):
  """One runtime.Program per (seed, family, option set), built without an
  extent on first use and shared: kernels are JIT-built once."""
  from soda_amd import runtime

  def get(seed, family, **okw):
    okw.setdefault('fuse', (2,))
    key = (seed, family, tuple(sorted(okw.items())))
    if key not in _PROGRAMS:
      _PROGRAMS[key] = runtime.Program(_tree(seed, family)[2], _opts(**okw))
    return _PROGRAMS[key]
  yield get
  for prog in _PROGRAMS.values():
    prog.close()
  _PROGRAMS.clear()


def _dense(hip, handle, ins, iterate):
  """The dense entry of a handle on device copies of `ins`."""
  st = hip.stencil
  shape = ins[st.input_names[0]].shape
  with periodic.Device(hip) as dev:
    d_in = [dev.upload(ins[n]) for n in st.input_names]
    d_out = [dev.alloc(int(np.prod(shape)) * np.dtype(t.np_name).itemsize)
             for t in st.output_types]
    handle.run_device(d_out, d_in, iterate)
    return {n: dev.download(p, shape, np.dtype(t.np_name))
            for n, p, t in zip(st.output_names, d_out, st.output_types)}


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('seed', GPU_SEEDS)
def test_a_torus(programs, seed, family):
  """A: run_periodic at the default refill interval and at 1."""
  prog, text, _ = _tree(seed, family)
  extent = _gpu_extent(seed, family, prog.dim)
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  want = prog.run_torus(ins, extent)
  hip = programs(seed, family)
  for k in (None, 1):
    _assert_same(hip.run_periodic(ins, refill_every=k), want,
                 'torus %s, refill every %s' % (extent, k), text)


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('seed', GPU_SEEDS)
def test_b_walls_at_depth_1(programs, seed, family):
  """B: run_bordered under MODES[(seed + family + d) % 5], then with `wrap`
  in one dimension and a wall in the others."""
  prog, text, _ = _tree(seed, family)
  extent = _gpu_extent(seed, family, prog.dim)
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  cst = _constants(prog)
  hip = programs(seed, family)
  for modes in (_modes(seed, family, prog.dim), _mixed(seed, family, prog.dim)):
    _assert_same(hip.run_bordered(ins, modes, cst),
                 prog.run_bordered(ins, extent, modes, cst),
                 'walls %s %s' % (extent, modes), text)


def _fused_on_the_gpu(programs, seed, family, fuse, below):
  """A fused run at depth 0 against the bordered nest; (the program's deepest
  pass, info(), the wall dimensions that have a strip), or None where
  border_fused_ghosts refuses the program."""
  from soda_amd import util
  prog, text, st = _tree(seed, family)
  hip = programs(seed, family, fuse=(fuse,))
  deepest = max(p.fused_iters for p in hip.module.passes)
  cst = _constants(prog)
  found = _fused_geometry(st, hip.plan, seed, family, deepest, GPU_CELLS,
                          below)
  if found is None:                 # the handle refuses in the same words
    with pytest.raises(util.InputError, match='reach more than'):
      hip.bordered(_gpu_extent(seed, family, prog.dim),
                   _modes(seed, family, prog.dim), cst, depth=0)
    return None
  modes, extent, (rlo, rhi, _, _) = found
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  iterate = 2 * deepest - 1 if seed % 2 else deepest + 1
  want = prog.run_bordered(ins, extent, modes, cst, iterate=iterate)
  with hip.bordered(extent, modes, cst, depth=0) as handle:
    info = handle.info()
    got = _dense(hip, handle, ins, iterate)
  _assert_same(got, want, 'fused %d deep, %s %s, %d iterations' % (
      deepest, extent, modes, iterate), text)
  walls = [d for d in range(prog.dim)
           if modes[d] != 'wrap' and rlo[d] + rhi[d]] if deepest > 1 else []
  return deepest, info, walls


@pytest.mark.gpu
@pytest.mark.parametrize('seed,family,fuse',
                         [(s, f, 2) for s, f in GPU_ITERABLE] +
                         [(s, f, 3) for s, f in FUSE3],
                         ids=['%s%d-fuse%d' % (f, s, t) for t, cases in (
                             (2, GPU_ITERABLE), (3, FUSE3)) for s, f in cases])
def test_c_walls_fused(programs, seed, family, fuse):
  """C: depth 0 on a program lowered with fuse=(2,) -- four of them with
  fuse=(3,) --, every wall dimension exactly L + H wide."""
  done = _fused_on_the_gpu(programs, seed, family, fuse, below=False)
  if done is not None:
    deepest, info, walls = done
    assert info['depth'] == deepest
    assert [s['dim'] for s in info['strips']] == walls
    if fuse == 3:
      assert deepest == 3 and walls


@pytest.mark.gpu
@pytest.mark.parametrize('seed,family', ONE_BELOW,
                         ids=['%s%d' % (f, s) for s, f in ONE_BELOW])
def test_c_one_cell_below_the_depth_is_1(programs, seed, family):
  """C: at L + H - 1 along a wall info() reports depth 1, the bits stay."""
  deepest, info, walls = _fused_on_the_gpu(programs, seed, family, 2,
                                           below=True)
  assert deepest == 2 and walls
  assert info['depth'] == 1 and info['strips'] == []


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('seed', BATCH_SEEDS)
def test_d_batches(programs, seed, family):
  """D: three items with different inputs through run_periodic_batch and
  run_bordered_batch, every item against the nest on it alone."""
  prog, text, _ = _tree(seed, family)
  extent = _gpu_extent(seed + 1, family, prog.dim)
  items = [fuzz_nest.inputs_for(prog, extent, seed + 1000 * (i + 1))
           for i in range(3)]
  stacked = {n: np.stack([it[n] for it in items]) for n, _ in prog.inputs}
  modes, cst = _modes(seed, family, prog.dim, shift=1), _constants(prog)
  hip = programs(seed, family, batch=True)
  torus = hip.run_periodic_batch(stacked)
  walls = hip.run_bordered_batch(stacked, modes, cst)
  for i, ins in enumerate(items):
    _assert_same({o: a[i] for o, a in torus.items()},
                 prog.run_torus(ins, extent), 'item %d, torus %s' % (i, extent),
                 text)
    _assert_same({o: a[i] for o, a in walls.items()},
                 prog.run_bordered(ins, extent, modes, cst),
                 'item %d, walls %s %s' % (i, extent, modes), text)


def _structs(hip, handle, prog, ins, modes, cst, iterate, cur, prev, what):
  """The residual and the norms of a handle's run against the nest's."""
  want_res, want_norms = _nest_numbers(prog, cur, prev)
  with domains.Run(hip, handle, ins, modes, cst) as run:
    padded, res = run.residual(iterate)
    print(what, domains.fields(res), want_res)
    _assert_same(run.interior(padded), cur, what)
    assert domains.fields(res) == want_res, what
    if want_norms is not None:
      padded, acc = run.norms(iterate)
      _assert_same(run.interior(padded), cur, what + ', norms')
      assert norms.same(acc, want_norms), what
    else:
      from soda_amd import util
      with pytest.raises(util.InputError, match='one accumulator'):
        run.norms(iterate)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,family', RESIDUAL,
                         ids=['%s%d' % (f, s) for s, f in RESIDUAL])
def test_e_residual_and_norms(programs, seed, family):
  """E: on the torus, between walls at depth 1 and fused, word for word
  against domains.delta / fold and norms.oracle on the nest's two last
  states."""
  prog, text, st = _tree(seed, family)
  hip = programs(seed, family, residual=True)
  cst = _constants(prog)
  extent = _gpu_extent(seed + 2, family, prog.dim)
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  n = prog.iterate
  cur, prev = prog.run_torus(ins, extent, n, with_previous=True)
  with hip.periodic(extent) as handle:
    _structs(hip, handle, prog, ins, None, None, n, cur, prev,
             'torus %s' % (extent,))
  modes = _modes(seed, family, prog.dim, shift=2)
  cur, prev = prog.run_bordered(ins, extent, modes, cst, iterate=n,
                                with_previous=True)
  with hip.bordered(extent, modes, cst) as handle:
    _structs(hip, handle, prog, ins, modes, cst, n, cur, prev,
             'walls %s %s' % (extent, modes))
  deepest = max(p.fused_iters for p in hip.module.passes)
  found = _fused_geometry(st, hip.plan, seed, family, deepest, GPU_CELLS)
  if found is None:
    return
  modes, extent, _ = found
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  n = 2 * deepest - 1
  cur, prev = prog.run_bordered(ins, extent, modes, cst, iterate=n,
                                with_previous=True)
  with hip.bordered(extent, modes, cst, depth=0) as handle:
    assert handle.info().get('depth', 1) == deepest
    _structs(hip, handle, prog, ins, modes, cst, n, cur, prev,
             'fused %d deep, %s %s' % (deepest, extent, modes))
