"""Periodic domains: a program on a torus, its ghost frame refilled on the GPU
(soda_hip_periodic_*, soda_hip_wrap_host).

Every comparison is on bit patterns.  The expected value is that of
tests/periodic.py: the inputs wrapped once on the host by all that `iterate`
iterations reach, the existing oracle on that open box, the torus cut out.

CPU: wrap_host against np.pad(mode='wrap') on all four cell sizes in 1 to 4
dimensions, one-sided ghosts, ghosts wider than the domain; the same closed
forms under a sanitizer in a program of their own; soda_hip_periodic_plan
against Stencil.window_bounds; the wrap modules compiled for gfx950 without
scratch; what the feature leaves untouched; refusals that need no GPU.
GPU: parity of the dense entry on ten programs, independence of the refill
interval, translation, the padded entry across calls, guard bands, a live
stream, a captured graph, refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import asyncrun
import celltypes
import guarded
import periodic

SIZES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _stencil(name, **kw):
  from soda_amd import core
  kw = {k: v for k, v in kw.items() if v is not None}
  return core.from_file(soda_path(name), **kw)


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('peel', 0)
  return lower.LowerOptions(**kw)


def _plan(stencil, extent=None, **kw):
  """The launch plan of a program, lowered without trial compilations."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, _opts(**kw), extent, probe=False)
  return runtime.make_plan(lower.lower(stencil, opts))


# ---------------------------------------------------------------------------
# CPU: the host twin
# ---------------------------------------------------------------------------

WRAP_CASES = [
    # (torus extent, ghost_lo, ghost_hi), dimension 0 first
    ((9,), (2,), (3,)),
    ((1,), (4,), (5,)),                       # N = 1: every cell the same
    ((5,), (0,), (7,)),                       # one-sided, wider than N
    ((12, 3), (4, 4), (4, 4)),                # wider than the domain in y
    ((7, 5), (3, 0), (0, 2)),                 # one-sided, alternating
    ((1, 1), (2, 3), (3, 2)),
    ((6, 4, 3), (1, 2, 0), (2, 0, 4)),
    ((3, 2, 2), (4, 4, 4), (4, 4, 4)),
    ((5, 3, 2, 2), (1, 0, 2, 1), (0, 2, 1, 3)),
    ((1, 2, 1, 3), (3, 3, 3, 3), (3, 3, 3, 3)),
]


@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('case', WRAP_CASES, ids=lambda c: 'x'.join(
    map(str, c[0])) + '+' + '.'.join(map(str, c[1] + c[2])))
def test_wrap_host_is_np_pad_wrap(built, size, case):
  from soda_amd import runtime
  extent, lo, hi = case
  rng = np.random.default_rng(size + len(extent))
  torus = rng.integers(0, 256, size=extent[::-1] + (size,), dtype=np.uint8)
  torus = np.ascontiguousarray(torus).view(SIZES[size]).reshape(extent[::-1])
  want = periodic.wrap_pad(torus, lo, hi)
  got = np.full(want.shape, 0x5A, torus.dtype)         # ghosts: garbage
  periodic.interior(got, dict(ghost_lo=lo, ghost_hi=hi))[...] = torus
  assert runtime.wrap_host(got, lo, hi) is got
  assert periodic.same_bits(got, want), periodic.differing(got, want)
  # float cells are moved like any other bits: a NaN payload survives
  if size in (4, 8):
    f = got.view({4: np.float32, 8: np.float64}[size]).copy()
    runtime.wrap_host(f, lo, hi)
    assert periodic.same_bits(f.view(got.dtype), want)


def test_wrap_host_refusals(built):
  from soda_amd import runtime, util
  a = np.zeros((4, 6), np.float32)
  with pytest.raises(util.InputError):
    runtime.wrap_host(a, (1,), (1,))                   # two dimensions
  with pytest.raises(util.InputError):
    runtime.wrap_host(a, (3, 0), (3, 0))               # no torus left
  with pytest.raises(util.InputError):
    runtime.wrap_host(a, (-1, 0), (1, 0))
  with pytest.raises(util.InputError):
    runtime.wrap_host(a[:, ::2], (1, 1), (1, 1))       # not contiguous
  with pytest.raises(util.InputError):
    runtime.wrap_host(np.zeros((4, 6), np.complex128), (1, 1), (1, 1))
  assert not a.any()


def test_host_twin_under_a_sanitizer(built, tmp_path):
  """tests/host/wrap_main.cpp + soda_wrap.cpp as one program with its own
  main, -fsanitize=address,undefined: nothing loaded into Python."""
  exe = os.path.join(str(tmp_path), 'wrap_main')
  subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
                  '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined',
                  '-I', os.path.join(ROOT, 'include'),
                  os.path.join(ROOT, 'tests', 'host', 'wrap_main.cpp'),
                  os.path.join(ROOT, 'soda_amd', 'csrc', 'soda_wrap.cpp'),
                  '-o', exe], check=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 0 and run.stdout.startswith('OK'), (
      run.stdout + run.stderr)


# ---------------------------------------------------------------------------
# CPU: the plan
# ---------------------------------------------------------------------------

PLANS = [
    # name, stencil keywords, LowerOptions keywords, torus, k, iterate
    ('jacobi2d.soda', dict(iterate=9), dict(fuse=(4,)), (40, 7), 4, 9),
    ('skew2d.soda', {}, {}, (24, 6), 1, 1),
    ('coupled2d.soda', {}, dict(fuse=(2,)), (32, 9), 2, 3),
    ('heat3d.soda', dict(iterate=5), dict(fuse=(2,)), (32, 6, 5), 2, 5),
]


@pytest.mark.parametrize('name,skw,okw,extent,k,iterate', PLANS,
                         ids=[p[0][:-5] for p in PLANS])
def test_plan_against_window_bounds(built, name, skw, okw, extent, k, iterate):
  """Ghosts: the most Stencil.window_bounds(k) reaches over all outputs; the
  padded extent; the chunk list; k = 0 resolves to the deepest pass."""
  from soda_amd import runtime
  stencil = _stencil(name, **skw)
  plan = _plan(stencil, **okw)
  boxes = stencil.window_bounds(k)
  want_lo = [max(0, max(-boxes[o][0][d] for o in stencil.output_names))
             for d in range(stencil.dim)]
  want_hi = [max(0, max(boxes[o][1][d] for o in stencil.output_names))
             for d in range(stencil.dim)]
  lo, hi = runtime.periodic_ghosts(stencil, k)
  assert lo[:-1] == want_lo[:-1] and hi[:-1] == want_hi[:-1]
  # (along the last dimension at least k x the per-iteration reach)
  rl, rh = stencil.reach_along(stencil.dim - 1)
  assert lo[-1] == max(want_lo[-1], k * rl) and \
      hi[-1] == max(want_hi[-1], k * rh)
  info, chunks = runtime.periodic_plan(plan, extent, k, lo, hi, iterate)
  vec = max(1, max(q.vec for q in plan.kernels[:plan.num_kernels]))
  assert info['refill_every'] == k
  assert info['ghost_lo'] == tuple(lo) and info['ghost_hi'][1:] == tuple(hi[1:])
  p0 = lo[0] + extent[0] + hi[0]
  assert info['padded'][0] == -(-p0 // vec) * vec
  assert info['ghost_hi'][0] == hi[0] + info['padded'][0] - p0 < hi[0] + vec
  assert info['padded'][1:] == tuple(
      l + n + h for l, n, h in zip(lo[1:], extent[1:], hi[1:]))
  assert chunks == [k] * (iterate // k) + ([iterate % k] if iterate % k else [])
  assert sum(chunks) == iterate
  cells = int(np.prod(info['padded']))
  per_cell = sum(plan.elem_size[i] for i in range(plan.num_inputs)) + 2 * sum(
      plan.elem_size[plan.num_inputs + o] for o in range(plan.num_outputs))
  assert info['scratch_bytes'] == cells * per_cell
  # k = 0: the largest fused_iters of the plan's passes
  deepest = max(plan.passes[i].fused_iters for i in range(plan.num_passes))
  glo, ghi = runtime.periodic_ghosts(stencil, deepest)
  assert runtime.periodic_plan(plan, extent, 0, glo, ghi)[0][
      'refill_every'] == deepest


def test_plan_shapes_of_the_ghosts(built):
  """jacobi2d: k per side; skew2d: the window of its offset output, local
  stage included; blur: one-sided; coupled2d: the widest of two outputs'
  windows, which differ."""
  from soda_amd import runtime
  assert runtime.periodic_ghosts(_stencil('jacobi2d.soda'), 4) == ([4, 4],
                                                                   [4, 4])
  st = _stencil('skew2d.soda')
  (lo, hi), = [st.window_bounds(1)[o] for o in st.output_names]
  assert (lo, hi) == ((-2, -2), (2, 2))    # b reaches (-1..2, -2..1), c b(1, 1)
  assert runtime.periodic_ghosts(st, 1) == ([2, 2], [2, 2])
  assert runtime.periodic_ghosts(_stencil('blur.soda'), 1) == ([0, 0], [2, 2])
  st = _stencil('coupled2d.soda')
  boxes = st.window_bounds(2)
  a2, b2 = (boxes[o] for o in st.output_names)
  assert a2 == ((-2, -1), (1, 2)) and b2 == ((-2, -2), (1, 2))
  assert runtime.periodic_ghosts(st, 2) == ([2, 2], [1, 2])


def test_plan_rounds_the_row_to_vec(built):
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda')
  for vec in (4, 2, 1):
    plan = _plan(st, fuse=(2,), vec=vec)
    for n0 in (37, 38, 39, 40):
      info, _ = runtime.periodic_plan(plan, (n0, 5), 2, (2, 2), (2, 2))
      p0 = info['padded'][0]
      assert p0 % vec == 0 and 0 <= p0 - (n0 + 4) < vec
      assert info['ghost_lo'] == (2, 2)
      assert info['ghost_hi'] == (2 + p0 - (n0 + 4), 2)


def test_refusals_without_a_gpu(built):
  from soda_amd import runtime, util
  st = _stencil('jacobi2d.soda')
  plan = _plan(st, fuse=(4,))
  ok = lambda **kw: runtime.periodic_plan(
      plan, kw.pop('extent', (40, 7)), kw.pop('k', 4),
      kw.pop('lo', (4, 4)), kw.pop('hi', (4, 4)), **kw)
  assert ok()[0]['padded'] == (48, 15)
  with pytest.raises(util.BackendError, match='unsupported.*preserve'):
    ok(preserve=True)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.periodic_plan(_plan(st, fuse=(4,), batch=True), (40, 7), 4,
                          (4, 4), (4, 4))
  # ghosts too small along the last dimension: k x reach = 4
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(lo=(4, 3))
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(hi=(4, 0))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(extent=(0, 7))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(lo=(-1, 4))
  # iterate > 1 on a program that cannot iterate
  sobel = _stencil('sobel2d.soda')
  splan = _plan(sobel)
  glo, ghi = runtime.periodic_ghosts(sobel, 1)
  assert runtime.periodic_plan(splan, (32, 6), 1, glo, ghi, 1,
                               not_iterable=True)[1] == [1]
  with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
    runtime.periodic_plan(splan, (32, 6), 1, glo, ghi, 2, not_iterable=True)
  # P[0] beyond a kernel's max_extent0: rows a whole block covers
  xs = _plan(st, (256, 8), fuse=(2,), xshare=True, row_cells=256)
  limit = max(q.max_extent0 for q in xs.kernels[:xs.num_kernels])
  assert limit > 0
  with pytest.raises(util.BackendError, match='invalid.*rows of at most'):
    runtime.periodic_plan(xs, (limit, 8), 2, (2, 2), (2, 2))
  # a plane above the 1 GiB window of the 3-D kernels
  heat = _stencil('heat3d.soda')
  hplan = _plan(heat, fuse=(2,))
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.periodic_plan(hplan, (32768, 16384, 4), 2, (2, 2, 2), (2, 2, 2))


@pytest.mark.parametrize('dim', (1, 2, 3, 4))
def test_the_kernels_compile_without_scratch(built, dim):
  """The wrap module of every cell size and dimension count, for gfx950: one
  kernel, no scratch, no LDS."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import wrap as gen
  for elem in sorted(SIZES):
    _, res = runtime.wrap_resources(elem, dim)
    name = gen.kernel_name(elem, dim)
    assert sorted(res) == [name]
    assert res[name]['scratch'] == 0, res[name]
    assert res[name]['lds'] == 0 and 0 < res[name]['vgpr'] <= 64, res[name]
    text = gen.source(elem, dim)
    assert 'asm' not in text.split('soda_rt_wrap.h', 1)[1]   # plain C++
  from soda_amd import util
  with pytest.raises(util.SemanticError):
    gen.source(3, 2)
  with pytest.raises(util.SemanticError):
    gen.source(4, 5)


def test_existing_modules_are_untouched():
  """Every module of the corpus is what it was: its text, kernels and plan
  know nothing of the torus, whether or not the wrap code was ever imported;
  no LowerOptions field was added."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  corpus = [('jacobi2d.soda', dict(iterate=13), dict(fuse=(13, 4))),
            ('jacobi2d.soda', dict(iterate=13), dict(fuse=(4,), residual=True)),
            ('heat3d.soda', dict(iterate=4), dict(fuse=(2,))),
            ('blur.soda', {}, {}), ('skew2d.soda', {}, {}),
            ('coupled2d.soda', {}, dict(fuse=(2,))),
            ('heat4d.soda', {}, dict(strategy='direct'))]
  for name, skw, okw in corpus:
    stencil = _stencil(name, **skw)
    opts = runtime.resolve_options(stencil, _opts(**okw), None, probe=False)
    before = lower.lower(stencil, opts)
    from soda_amd.codegen.hip import wrap as gen
    gen.source(4, stencil.dim)
    runtime.periodic_ghosts(stencil, 2)
    after = lower.lower(stencil, opts)
    assert before.source == after.source
    assert 'soda_wrap' not in after.source and 'periodic' not in after.source
    assert [k.name for k in before.kernels] == [k.name for k in after.kernels]
    assert bytes(runtime.make_plan(before)) == bytes(runtime.make_plan(after))
  assert not any('period' in f or 'wrap' in f or 'torus' in f
                 for f in lower.LowerOptions.__dataclass_fields__)


def test_abi_and_structs(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == 9
  assert lib.soda_hip_sizeof(15) == ctypes.sizeof(runtime.PeriodicDesc) == 60
  assert lib.soda_hip_sizeof(16) == ctypes.sizeof(runtime.PeriodicInfo)
  assert lib.soda_hip_sizeof(3) == ctypes.sizeof(runtime.Plan)
  assert lib.soda_hip_sizeof(14) == ctypes.sizeof(runtime.NormsStruct)
  for name in ('soda_hip_wrap_host', 'soda_hip_periodic_plan',
               'soda_hip_periodic_create', 'soda_hip_periodic_destroy',
               'soda_hip_periodic_info', 'soda_hip_periodic_fill',
               'soda_hip_periodic_run_padded', 'soda_hip_periodic_run_device'):
    assert name in runtime.API and hasattr(lib, name), name


def test_command_line_has_the_torus():
  run = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', '--help'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode == 0
  assert '--hip-periodic' in run.stdout and '--hip-refill-every' in run.stdout


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ct(t):
  return lambda: celltypes.stencil_of(t, 2, 'main', 5)


# name -> (stencil, LowerOptions keywords, torus, iterate, refill_every)
CASES = {
    'jacobi2d': (lambda: _stencil('jacobi2d.soda', iterate=9), dict(fuse=(4,)),
                 (40, 7), 9, 4),                       # chunks 4, 4, 1
    'jacobi2d_narrow': (lambda: _stencil('jacobi2d.soda', iterate=9),
                        dict(fuse=(4,)), (12, 3), 9, 4),   # ghosts wider in y
    'skew2d': (lambda: _stencil('skew2d.soda'), {}, (24, 6), 1, None),
    'coupled2d': (lambda: _stencil('coupled2d.soda'), dict(fuse=(2,)),
                  (32, 9), 3, 2),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=5), dict(fuse=(2,)),
               (32, 6, 5), 5, 2),
    'blur': (lambda: _stencil('blur.soda'), {}, (64, 8), 1, None),
    'ints2d': (lambda: _stencil('ints2d.soda'), {}, (32, 6), 1, None),
    # `direct`, on the smallest torus there is: one cell, wrapped many times
    'heat4d': (lambda: _stencil('heat4d.soda', iterate=2),
               dict(strategy='direct'), (1, 1, 1, 1), 2, None),
    'double': (_ct('double'), dict(fuse=(4,), chunk_rows=16), (24, 5), 5, 4),
    'uint8': (_ct('uint8'), dict(fuse=(4,), chunk_rows=16), (48, 5), 5, 4),
}

_PROGRAMS = {}
_EXPECTED = {}


@pytest.fixture(scope='module')
def programs(built):
  """Programs by (case name, extra keywords), made on first use, shared."""
  from soda_amd import runtime

  def get(name, **extra):
    key = (name, tuple(sorted(extra.items())))
    if key not in _PROGRAMS:
      make, okw = CASES[name][:2]
      _PROGRAMS[key] = runtime.Program(make(), _opts(**dict(okw, **extra)))
    return _PROGRAMS[key]
  yield get
  for prog in _PROGRAMS.values():
    prog.close()
  _PROGRAMS.clear()


def _case(name, seed=0):
  """(stencil, torus, iterate, k, inputs, expected), computed once."""
  key = (name, seed)
  if key not in _EXPECTED:
    make, _, extent, iterate, k = CASES[name]
    stencil = make()
    ins = periodic.inputs(stencil, extent, seed)
    _EXPECTED[key] = (stencil, extent, iterate, k, ins,
                      periodic.expected(stencil, ins, iterate))
  return _EXPECTED[key]


def _dense(prog, per, ins, iterate, stream=0):
  """The dense entry on device copies of `ins`; {output: array}."""
  st = prog.stencil
  shape = ins[st.input_names[0]].shape
  with periodic.Device(prog) as dev:
    d_in = [dev.upload(ins[n]) for n in st.input_names] + \
        [dev.upload(np.ascontiguousarray(ins[p.name]).reshape(-1))
         for p in st.param_stmts]
    d_out = [dev.alloc(int(np.prod(shape)) * np.dtype(t.np_name).itemsize)
             for t in st.output_types]
    per.run_device(d_out, d_in, iterate, stream)
    return {n: dev.download(p, shape, np.dtype(t.np_name))
            for n, p, t in zip(st.output_names, d_out, st.output_types)}


def _assert_same(got, want, what):
  assert sorted(got) == sorted(want)
  for o in want:
    assert periodic.same_bits(got[o], want[o]), \
        '%s: %d cells of %s differ in their bits' % (
            what, periodic.differing(got[o], want[o]), o)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_dense_entry_against_the_padded_oracle(programs, name):
  stencil, extent, iterate, k, ins, want = _case(name)
  assert all(np.isfinite(w).all() for w in want.values() if w.dtype.kind == 'f')
  prog = programs(name)
  with prog.periodic(extent, k) as per:
    info = per.info()
    assert info['refill_every'] == (k or max(
        p.fused_iters for p in prog.module.passes))
    got = _dense(prog, per, ins, iterate)
  _assert_same(got, want, name)
  if name == 'jacobi2d_narrow':
    assert info['ghost_lo'][1] > extent[1] and info['ghost_hi'][1] > extent[1]
  if name == 'jacobi2d':
    # the C oracle agrees with the numpy one on the padded box
    from oracle import c_oracle
    _assert_same(periodic.expected(
        stencil, ins, iterate,
        run=lambda st, p, it: c_oracle.COracle(st).run(p, iterate=it)),
                 want, 'c_oracle')
    # ... and numpy in, numpy out
    _assert_same(prog.run_periodic(ins, iterate, k), want, 'run_periodic')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['jacobi2d', 'heat3d'])
def test_the_refill_interval_does_not_change_a_bit(programs, name):
  stencil, extent, iterate, _, ins, want = _case(name)
  prog = programs(name)
  deepest = max(p.fused_iters for p in prog.module.passes)
  assert deepest == {'jacobi2d': 4, 'heat3d': 2}[name]
  seen = []
  for k in (1, 2, None):
    with prog.periodic(extent, k) as per:
      assert per.info()['refill_every'] == (k or deepest)
      seen.append(_dense(prog, per, ins, iterate))
  for k, got in zip((1, 2, deepest), seen):
    _assert_same(got, want, '%s, refill every %d' % (name, k))
    _assert_same(got, seen[0], '%s, refill every %d against 1' % (name, k))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['jacobi2d', 'coupled2d'])
def test_translation(programs, name):
  """Rolling every input by (3, 2) rolls every output by the same amount."""
  stencil, extent, iterate, k, ins, _ = _case(name)
  prog = programs(name)
  roll = lambda a: np.roll(a, (2, 3), axis=(0, 1))     # x by 3, y by 2
  with prog.periodic(extent, k) as per:
    plain = _dense(prog, per, ins, iterate)
    rolled = _dense(prog, per, {n: roll(a) for n, a in ins.items()}, iterate)
  _assert_same(rolled, {o: roll(a) for o, a in plain.items()}, name)
  assert not all(periodic.same_bits(rolled[o], plain[o]) for o in plain)


@pytest.mark.gpu
def test_padded_entry_across_calls(programs):
  """Two run_padded calls of 3 and 4 iterations equal one dense run of 7; the
  outputs come back wrapped; the inputs are byte-identical afterwards."""
  from soda_amd import runtime
  stencil, extent, _, k, ins, _ = _case('jacobi2d')
  want = periodic.expected(stencil, ins, 7)
  prog = programs('jacobi2d')
  with prog.periodic(extent, k) as per, periodic.Device(prog) as dev:
    info = per.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    start = periodic.wrap_pad(ins['t1'], lo, hi)
    assert start.shape == info['padded'][::-1]
    d0, d1, d2 = dev.upload(start), dev.alloc(start.nbytes), \
        dev.alloc(start.nbytes)
    per.run_padded([d1], [d0], 3)
    per.run_padded([d2], [d1], 4)
    after3 = dev.download(d1, start.shape, start.dtype)
    after7 = dev.download(d2, start.shape, start.dtype)
    assert periodic.same_bits(dev.download(d0, start.shape, start.dtype),
                              start)
    dense = _dense(prog, per, ins, 7)
  _assert_same({'t0': periodic.interior(after7, info)}, want, 'padded 3 + 4')
  _assert_same(dense, want, 'dense 7')
  _assert_same({'t0': periodic.interior(after3, info)},
               periodic.expected(stencil, ins, 3), 'padded 3')
  for arr in (after3, after7):                 # wrapped: ghosts current
    again = np.full_like(arr, -77.0)             # ghosts: garbage
    periodic.interior(again, info)[...] = periodic.interior(arr, info)
    runtime.wrap_host(again, lo, hi)
    assert periodic.same_bits(again, arr), periodic.differing(again, arr)
    assert periodic.same_bits(
        arr, periodic.wrap_pad(periodic.interior(arr, info), lo, hi))


class _DenseEntry:
  """The dense entry with run_device's call shape, for tests/guarded.py."""

  def __init__(self, prog, per):
    self.device, self.per = prog.device, per

  def run_device(self, outputs, inputs, extent, iterate=None, **kw):
    self.per.run_device(outputs, inputs, iterate, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['jacobi2d', 'coupled2d', 'heat3d', 'blur'])
def test_dense_entry_between_guard_bands(programs, name):
  stencil, extent, iterate, k, ins, want = _case(name)
  prog = programs(name)
  with prog.periodic(extent, k) as per:
    got, violation, _ = guarded.run(_DenseEntry(prog, per), stencil, extent,
                                    ins, iterate)
  assert violation is None, violation
  _assert_same(got, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['jacobi2d', 'jacobi2d_narrow', 'heat3d',
                                  'blur', 'heat4d', 'double', 'uint8'])
def test_fill_writes_ghost_cells_only(programs, name):
  """A planted pattern: the interior keeps every byte, every ghost cell takes
  its interior cell -- at an address that is aligned to the cell only."""
  stencil, extent, _, k, _, _ = _case(name)
  prog = programs(name)
  dtype = np.dtype(stencil.output_types[0].np_name)
  with prog.periodic(extent, k) as per, periodic.Device(prog) as dev:
    info = per.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    shape = info['padded'][::-1]
    rng = np.random.default_rng(11)
    for lead in (0, 1, 3):                       # cells behind a 16-byte line
      raw = rng.integers(0, 256, size=(lead + int(np.prod(shape)) + 5) *
                         dtype.itemsize, dtype=np.uint8)
      base = dev.upload(raw)
      per.fill([base + lead * dtype.itemsize])
      back = dev.download(base, raw.shape, np.uint8)
      cells = lambda b: b[lead * dtype.itemsize:
                          (lead + int(np.prod(shape))) * dtype.itemsize].view(
                              dtype).reshape(shape)
      before, after = cells(raw), cells(back)
      assert periodic.same_bits(periodic.interior(after, info),
                                periodic.interior(before, info))
      assert periodic.same_bits(
          after, periodic.wrap_pad(periodic.interior(before, info), lo, hi)), \
          periodic.differing(after, periodic.wrap_pad(
              periodic.interior(before, info), lo, hi))
      # no byte in front of or behind the array
      n = lead * dtype.itemsize
      assert (back[:n] == raw[:n]).all()
      assert (back[-5 * dtype.itemsize:] == raw[-5 * dtype.itemsize:]).all()


@pytest.mark.gpu
def test_dense_entry_on_a_side_stream_ahead_of_its_inputs(programs):
  stencil, extent, iterate, k, ins, want = _case('jacobi2d')
  prog = programs('jacobi2d')
  shape = extent[::-1]
  with prog.periodic(extent, k) as per:
    _dense(prog, per, ins, iterate)       # sizes and times the program on P
    got = asyncrun.late_fill(
        'periodic dense entry', ins, {'t0': (shape, np.float32)},
        lambda run: per.run_device(run.outs(), run.ins(), iterate,
                                   stream=run.ptr))
  _assert_same(got, want, 'late fill')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['jacobi2d', 'heat3d'])
def test_dense_entry_captured_and_replayed(programs, name):
  import torch
  stencil, extent, iterate, k, ins, want = _case(name)
  ins2, want2 = _case(name, seed=5)[4:]
  prog = programs(name)
  i_name, o_name = stencil.input_names[0], stencil.output_names[0]
  S = torch.cuda.Stream()
  with prog.periodic(extent, k) as per:
    t_in = asyncrun._bytes(ins[i_name])
    t_out = asyncrun._bytes(asyncrun.poison_like(want[o_name]))
    read = lambda: t_out.cpu().numpy().view(np.float32).reshape(extent[::-1])
    call = lambda: per.run_device([t_out.data_ptr()], [t_in.data_ptr()],
                                  iterate, stream=S.cuda_stream)
    torch.cuda.synchronize()
    call()                                        # eager: sizes the scratch
    S.synchronize()
    _assert_same({o_name: read()}, want, name + ', eager')
    warm, held = prog.scratch(), per.info()['scratch_bytes']
    t_out.copy_(asyncrun._bytes(asyncrun.poison_like(want[o_name])))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
      call()
    assert np.isnan(read()).all()                 # capture records only
    g.replay()
    torch.cuda.synchronize()
    _assert_same({o_name: read()}, want, name + ', replay')
    t_in.copy_(asyncrun._bytes(ins2[i_name]))     # changed inputs
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_same({o_name: read()}, want2, name + ', replay on new inputs')
    assert prog.scratch() == warm and per.info()['scratch_bytes'] == held
    del g


@pytest.mark.gpu
def test_refusals_launch_nothing_and_allocate_nothing(programs, built):
  from soda_amd import runtime, util
  stencil, extent, iterate, k, ins, want = _case('jacobi2d')
  prog = programs('jacobi2d')
  with prog.periodic(extent, k) as per:
    _dense(prog, per, ins, iterate)
  launches, scratch = prog.last_launches(), prog.scratch()
  # ghosts too small along the last dimension
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    prog.periodic(extent, 4, ghosts=((4, 3), (4, 4)))
  assert prog.last_launches() == launches and prog.scratch() == scratch
  assert prog._periodic == []
  # `border: preserve`
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3, border='preserve'),
                       _opts(fuse=(2,))) as pres:
    before = pres.last_launches(), pres.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*preserve'):
      pres.periodic(extent)
    assert (pres.last_launches(), pres.scratch()) == before
  # a batched plan
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3),
                       _opts(fuse=(2,), batch=True)) as bat:
    before = bat.last_launches(), bat.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      bat.periodic(extent)
    assert (bat.last_launches(), bat.scratch()) == before
  # iterate > 1 on sobel2d: refused by both run entries, no byte written
  sobel = _stencil('sobel2d.soda')
  sext = (32, 6)
  sins = periodic.inputs(sobel, sext)
  with runtime.Program(sobel, _opts()) as sp, \
      sp.periodic(sext) as per, periodic.Device(sp) as dev:
    info = per.info()
    got = _dense(sp, per, sins, 1)                # one iteration is served
    _assert_same(got, periodic.expected(sobel, sins, 1), 'sobel2d')
    before = sp.last_launches(), sp.scratch(), info['scratch_bytes']
    planted = np.full(info['padded'][::-1], 0xA5A5, np.uint16)
    d_out = dev.upload(planted)
    d_in = dev.upload(periodic.wrap_pad(sins['img'], info['ghost_lo'],
                                        info['ghost_hi']))
    d_dense = dev.upload(sins['img'])
    with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
      per.run_padded([d_out], [d_in], 2)
    with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
      per.run_device([d_out], [d_dense], 2)
    with pytest.raises(util.BackendError, match='invalid'):
      per.run_device([d_out], [d_dense], 0)
    # the contract: an output that is an input
    with pytest.raises(util.BackendError, match='overlaps an input'):
      per.run_padded([d_in], [d_in], 1)
    assert periodic.same_bits(dev.download(d_out, planted.shape, np.uint16),
                              planted)
    assert (sp.last_launches(), sp.scratch(),
            per.info()['scratch_bytes']) == before
