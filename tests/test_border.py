"""Bordered domains: a border mode per dimension -- wrap, clamp, mirror,
mirror101, constant -- refilled on the GPU after every iteration
(soda_hip_border_*, soda_hip_extend_host).

Every comparison is on bit patterns.  The expected value is that of
tests/borders.py: for every iteration the inputs padded with np.pad axis by
axis by what one iteration reaches, the existing oracle for one iteration on
that open box, the domain cut out.

CPU: extend_host against np.pad on all four cell sizes in 1 to 4 dimensions,
mixed modes, one-sided frames, frames wider than the domain; the closed forms
under a sanitizer in a program of their own; soda_hip_border_plan; the extend
modules compiled for gfx950 without scratch; what the feature leaves
untouched; refusals that need no GPU.
GPU: parity of the dense entry per mode and program, the padded entry across
calls, guard bands, fills on unaligned arrays, NaN payloads, translation along
a wrapped dimension, the torus, a live stream, a captured graph, refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import asyncrun
import borders
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

EXTEND_CASES = [
    # (extent, ghost_lo, ghost_hi), dimension 0 first
    ((9,), (2,), (3,)),
    ((1,), (4,), (5,)),                       # N = 1
    ((2,), (7,), (6,)),                       # N = 2, several bounces
    ((5,), (0,), (11,)),                      # one-sided, wider than N
    ((12, 3), (4, 4), (4, 4)),                # wider than the domain in y
    ((7, 5), (3, 0), (0, 2)),                 # one-sided, alternating
    ((1, 2), (2, 3), (3, 5)),
    ((6, 4, 3), (1, 2, 0), (2, 0, 4)),
    ((2, 1, 2), (4, 4, 4), (4, 4, 4)),
    ((5, 3, 2, 2), (1, 0, 2, 1), (0, 2, 1, 3)),
    ((1, 2, 1, 3), (3, 3, 3, 3), (3, 3, 3, 3)),
]
# per dimension, cut to the case's dimension count: every mode alone, mixed
MODE_SETS = [('wrap',) * 4, ('clamp',) * 4, ('mirror',) * 4,
             ('mirror101',) * 4, ('constant',) * 4,
             ('wrap', 'clamp', 'mirror', 'mirror101'),
             ('constant', 'mirror', 'constant', 'clamp'),
             ('mirror101', 'constant', 'wrap', 'constant')]


def _cells(rng, extent, size):
  raw = rng.integers(0, 256, size=extent[::-1] + (size,), dtype=np.uint8)
  return np.ascontiguousarray(raw).view(SIZES[size]).reshape(extent[::-1])


@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('case', EXTEND_CASES, ids=lambda c: 'x'.join(
    map(str, c[0])) + '+' + '.'.join(map(str, c[1] + c[2])))
def test_extend_host_is_np_pad(built, size, case):
  from soda_amd import runtime
  extent, lo, hi = case
  dim = len(extent)
  rng = np.random.default_rng(size + dim)
  domain = _cells(rng, extent, size)
  # an 8-byte constant uses all its bytes
  cst = SIZES[size](0xF1E2D3C4B5A69788 & ((1 << (8 * size)) - 1))
  for modes in MODE_SETS:
    modes = modes[:dim]
    want = borders.pad(domain, lo, hi, modes, cst)
    got = np.full(want.shape, 0x5A, domain.dtype)        # ghosts: garbage
    periodic.interior(got, dict(ghost_lo=lo, ghost_hi=hi))[...] = domain
    assert runtime.extend_host(got, lo, hi, modes, cst) is got
    assert periodic.same_bits(got, want), (modes,
                                           periodic.differing(got, want))
    # one name for all dimensions
    if len(set(modes)) == 1:
      again = got.copy()
      periodic.interior(again, dict(ghost_lo=lo, ghost_hi=hi))[...] = domain
      runtime.extend_host(again, lo, hi, modes[0], cst)
      assert periodic.same_bits(again, want)


def test_extend_host_order_of_the_axes_does_not_matter():
  """np.pad axis by axis in either order gives the same array, `constant`
  included: the map is separable."""
  rng = np.random.default_rng(3)
  a = rng.integers(0, 1000, size=(3, 5)).astype(np.int32)
  for m0 in borders.MODES:
    for m1 in borders.MODES:
      kw = lambda m: dict(constant_values=-9) if m == 'constant' else {}
      xy = np.pad(np.pad(a, ((0, 0), (4, 7)), mode=borders.NUMPY[m0], **kw(m0)),
                  ((6, 2), (0, 0)), mode=borders.NUMPY[m1], **kw(m1))
      yx = np.pad(np.pad(a, ((6, 2), (0, 0)), mode=borders.NUMPY[m1], **kw(m1)),
                  ((0, 0), (4, 7)), mode=borders.NUMPY[m0], **kw(m0))
      assert xy.tobytes() == yx.tobytes()
      assert xy.tobytes() == borders.closed_form(a, (4, 6), (7, 2), (m0, m1),
                                                 -9).tobytes()


def test_extend_host_keeps_a_nan_payload(built):
  """Cells are moved, the constant is bits: an fp32 NaN with a payload comes
  out as it went in, in the ghosts of a constant and of a mirrored array."""
  from soda_amd import runtime
  nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
  lo, hi = (2, 1), (3, 2)
  a = np.zeros((3 + 3, 2 + 4 + 3), np.float32)
  periodic.interior(a, dict(ghost_lo=lo, ghost_hi=hi))[...] = 1.0
  runtime.extend_host(a, lo, hi, 'constant', nan)
  bits = a.view(np.uint32)
  assert (periodic.interior(bits, dict(ghost_lo=lo, ghost_hi=hi)) ==
          0x3F800000).all()
  assert (bits == 0x7FC12345).sum() == a.size - 3 * 4
  # the same bits as bytes
  b = np.zeros_like(a)
  runtime.extend_host(b, lo, hi, ('clamp', 'constant'),
                      np.array([0xFFC00001], np.uint32).tobytes())
  assert (b.view(np.uint32)[0] == 0xFFC00001).all()
  assert (b.view(np.uint32)[1:4] == 0).all()
  # a NaN in the interior, mirrored
  c = np.zeros((1, 7), np.float32)
  c.view(np.uint32)[0, 2] = 0x7FC12345
  runtime.extend_host(c, (2, 0), (2, 0), 'mirror')
  assert list(c.view(np.uint32)[0]) == [0, 0x7FC12345, 0x7FC12345, 0, 0, 0, 0]


def test_extend_host_refusals(built):
  from soda_amd import runtime, util
  a = np.zeros((4, 6), np.float32)
  with pytest.raises(util.InputError):
    runtime.extend_host(a, (1,), (1,), 'clamp')              # two dimensions
  with pytest.raises(util.InputError):
    runtime.extend_host(a, (3, 0), (3, 0), 'clamp')          # no domain left
  with pytest.raises(util.InputError):
    runtime.extend_host(a, (-1, 0), (1, 0), 'clamp')
  with pytest.raises(util.InputError):
    runtime.extend_host(a[:, ::2], (1, 1), (1, 1), 'clamp')  # not contiguous
  with pytest.raises(util.InputError, match='unknown mode'):
    runtime.extend_host(a, (1, 1), (1, 1), 'reflect')
  with pytest.raises(util.InputError):
    runtime.extend_host(a, (1, 1), (1, 1), ('clamp',))       # one per dimension
  with pytest.raises(util.InputError):
    runtime.extend_host(a, (1, 1), (1, 1), 'constant', b'\x00' * 8)
  assert not a.any()
  # the library itself refuses a mode it does not know
  lib = runtime.library()
  i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
  assert lib.soda_hip_extend_host(a.ctypes.data, 4, 2, i32(4, 2), i32(1, 1),
                                  i32(1, 1), i32(1, 5), 0) != 0
  assert not a.any()


def test_host_twin_under_a_sanitizer(built, tmp_path):
  """tests/host/extend_main.cpp + soda_extend.cpp as one program with its own
  main, -fsanitize=address,undefined: nothing loaded into Python."""
  exe = os.path.join(str(tmp_path), 'extend_main')
  subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
                  '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined',
                  '-I', os.path.join(ROOT, 'include'),
                  os.path.join(ROOT, 'tests', 'host', 'extend_main.cpp'),
                  os.path.join(ROOT, 'soda_amd', 'csrc', 'soda_extend.cpp'),
                  '-o', exe], check=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 0 and run.stdout.startswith('OK'), (
      run.stdout + run.stderr)


# ---------------------------------------------------------------------------
# CPU: the plan
# ---------------------------------------------------------------------------

PLANS = [
    # name, stencil keywords, LowerOptions keywords, extent, modes, iterate
    ('jacobi2d.soda', dict(iterate=9), dict(fuse=(4,)), (40, 7), 'clamp', 9),
    ('skew2d.soda', {}, {}, (24, 6), ('mirror', 'wrap'), 1),
    ('coupled2d.soda', {}, dict(fuse=(2,)), (32, 9), 'constant', 3),
    ('heat3d.soda', dict(iterate=5), dict(fuse=(2,)), (32, 6, 5),
     ('mirror', 'clamp', 'wrap'), 5),
]


@pytest.mark.parametrize('name,skw,okw,extent,modes,iterate', PLANS,
                         ids=[p[0][:-5] for p in PLANS])
def test_plan_against_window_bounds(built, name, skw, okw, extent, modes,
                                    iterate):
  """Ghosts: the most Stencil.window_bounds(1) reaches over all outputs; the
  padded extent; chunks of one iteration each, whatever the plan fuses."""
  from soda_amd import runtime
  stencil = _stencil(name, **skw)
  plan = _plan(stencil, **okw)
  boxes = stencil.window_bounds(1)
  want_lo = [max(0, max(-boxes[o][0][d] for o in stencil.output_names))
             for d in range(stencil.dim)]
  want_hi = [max(0, max(boxes[o][1][d] for o in stencil.output_names))
             for d in range(stencil.dim)]
  lo, hi = runtime.border_ghosts(stencil, modes)
  assert lo[:-1] == want_lo[:-1] and hi[:-1] == want_hi[:-1]
  rl, rh = stencil.reach_along(stencil.dim - 1)
  assert lo[-1] == max(want_lo[-1], rl) and hi[-1] == max(want_hi[-1], rh)
  assert (lo, hi) == runtime.periodic_ghosts(stencil, 1)
  for k in (0, 1):
    info, chunks = runtime.border_plan(plan, extent, modes, lo, hi, iterate,
                                       refill_every=k)
    vec = max(1, max(q.vec for q in plan.kernels[:plan.num_kernels]))
    assert info['refill_every'] == 1
    assert info['ghost_lo'] == tuple(lo)
    assert info['ghost_hi'][1:] == tuple(hi[1:])
    p0 = lo[0] + extent[0] + hi[0]
    assert info['padded'][0] == -(-p0 // vec) * vec
    assert info['ghost_hi'][0] == hi[0] + info['padded'][0] - p0 < hi[0] + vec
    assert info['padded'][1:] == tuple(
        l + n + h for l, n, h in zip(lo[1:], extent[1:], hi[1:]))
    assert chunks == [1] * iterate
    cells = int(np.prod(info['padded']))
    per_cell = sum(plan.elem_size[i] for i in range(plan.num_inputs)) + \
        2 * sum(plan.elem_size[plan.num_inputs + o]
                for o in range(plan.num_outputs))
    assert info['scratch_bytes'] == cells * per_cell


def test_plan_shapes_of_the_ghosts(built):
  from soda_amd import runtime
  assert runtime.border_ghosts(_stencil('jacobi2d.soda'), 'clamp') == (
      [1, 1], [1, 1])
  assert runtime.border_ghosts(_stencil('skew2d.soda'), 'mirror') == (
      [2, 2], [2, 2])
  assert runtime.border_ghosts(_stencil('blur.soda'), 'mirror101') == (
      [0, 0], [2, 2])                                     # one-sided
  st = _stencil('coupled2d.soda')
  boxes = st.window_bounds(1)
  a1, b1 = (boxes[o] for o in st.output_names)
  assert a1 != b1                                         # the widest of two
  assert runtime.border_ghosts(st, ('clamp', 'wrap')) == (
      [max(-a1[0][d], -b1[0][d]) for d in range(2)],
      [max(a1[1][d], b1[1][d]) for d in range(2)])
  assert runtime.border_ghosts(_stencil('heat3d.soda'), 'constant') == (
      [1, 1, 1], [1, 1, 1])


def test_plan_rounds_the_row_to_vec(built):
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda')
  for vec in (4, 2, 1):
    plan = _plan(st, fuse=(2,), vec=vec)
    for n0 in (1, 2, 37, 38, 39, 40):
      info, _ = runtime.border_plan(plan, (n0, 5), 'mirror101', (1, 1), (1, 1))
      p0 = info['padded'][0]
      assert p0 % vec == 0 and 0 <= p0 - (n0 + 2) < vec
      assert info['ghost_lo'] == (1, 1)
      assert info['ghost_hi'] == (1 + p0 - (n0 + 2), 1)


def test_an_all_wrap_plan_is_the_periodic_plan(built):
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda', iterate=9)
  plan = _plan(st, fuse=(4,))
  for k in (0, 1, 2, 4):
    lo, hi = runtime.periodic_ghosts(st, k or 4)
    assert runtime.border_plan(plan, (40, 7), 'wrap', lo, hi, 9,
                               refill_every=k) == \
        runtime.periodic_plan(plan, (40, 7), k, lo, hi, 9)
  assert runtime.border_plan(plan, (40, 7), 'wrap', (4, 4), (4, 4), 9)[1] == [
      4, 4, 1]


def test_refusals_without_a_gpu(built):
  from soda_amd import runtime, util
  st = _stencil('jacobi2d.soda')
  plan = _plan(st, fuse=(4,))
  ok = lambda **kw: runtime.border_plan(
      plan, kw.pop('extent', (40, 7)), kw.pop('modes', ('clamp', 'mirror')),
      kw.pop('lo', (1, 1)), kw.pop('hi', (1, 1)), **kw)
  assert ok()[0]['padded'] == (44, 9)
  # modes
  with pytest.raises(util.BackendError, match='invalid.*mode'):
    ok(modes=(1, 5))
  with pytest.raises(util.BackendError, match='invalid.*mode'):
    ok(modes=(-1, 0))
  with pytest.raises(util.InputError, match='unknown mode'):
    ok(modes='edge')
  # only a torus fuses between refills
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    ok(refill_every=2)
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    ok(modes=('wrap', 'constant'), lo=(4, 4), hi=(4, 4), refill_every=4)
  assert ok(modes='wrap', lo=(4, 4), hi=(4, 4), refill_every=4)[0][
      'refill_every'] == 4
  # what a torus refuses
  with pytest.raises(util.BackendError, match='unsupported.*preserve'):
    ok(preserve=True)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.border_plan(_plan(st, fuse=(4,), batch=True), (40, 7), 'clamp',
                        (1, 1), (1, 1))
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(lo=(1, 0))
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(hi=(1, 0))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(extent=(0, 7))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(lo=(-1, 1))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(refill_every=-1)
  sobel = _stencil('sobel2d.soda')
  splan = _plan(sobel)
  glo, ghi = runtime.border_ghosts(sobel, 'mirror101')
  assert runtime.border_plan(splan, (32, 6), 'mirror101', glo, ghi, 1,
                             not_iterable=True)[1] == [1]
  with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
    runtime.border_plan(splan, (32, 6), 'mirror101', glo, ghi, 2,
                        not_iterable=True)
  # P[0] beyond a kernel's max_extent0: rows a whole block covers
  xs = _plan(st, (256, 8), fuse=(2,), xshare=True, row_cells=256)
  limit = max(q.max_extent0 for q in xs.kernels[:xs.num_kernels])
  assert limit > 0
  with pytest.raises(util.BackendError, match='invalid.*rows of at most'):
    runtime.border_plan(xs, (limit, 8), 'clamp', (1, 1), (1, 1))
  # a plane above the 1 GiB window of the 3-D kernels
  hplan = _plan(_stencil('heat3d.soda'), fuse=(2,))
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.border_plan(hplan, (32768, 16384, 4), 'clamp', (1, 1, 1),
                        (1, 1, 1))


@pytest.mark.parametrize('dim', (1, 2, 3, 4))
def test_the_kernels_compile_without_scratch(built, dim):
  """The extend module of every cell size and dimension count, for gfx950:
  one kernel, no scratch, no LDS."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import extend as gen
  for elem in sorted(SIZES):
    _, res = runtime.extend_resources(elem, dim)
    name = gen.kernel_name(elem, dim)
    assert sorted(res) == [name]
    assert res[name]['scratch'] == 0, res[name]
    assert res[name]['lds'] == 0 and 0 < res[name]['vgpr'] <= 64, res[name]
    text = gen.source(elem, dim)
    assert 'asm' not in text.split('soda_rt_extend.h', 1)[1]   # plain C++
  with pytest.raises(util.SemanticError):
    gen.source(3, 2)
  with pytest.raises(util.SemanticError):
    gen.source(4, 5)


def test_existing_modules_are_untouched():
  """The wrap modules and the programs' modules are what they were: neither
  mentions the extend module, no LowerOptions field was added."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import extend, lower, wrap
  for elem in sorted(SIZES):
    for dim in (1, 2, 3, 4):
      extend.source(elem, dim)
      text = wrap.source(elem, dim)
      assert 'extend' not in text.lower() and 'border_' not in text
  for name, skw, okw in [('jacobi2d.soda', dict(iterate=13), dict(fuse=(4,))),
                         ('heat3d.soda', dict(iterate=4), dict(fuse=(2,))),
                         ('blur.soda', {}, {})]:
    stencil = _stencil(name, **skw)
    opts = runtime.resolve_options(stencil, _opts(**okw), None, probe=False)
    before = lower.lower(stencil, opts)
    runtime.border_ghosts(stencil, 'clamp')
    after = lower.lower(stencil, opts)
    assert before.source == after.source
    assert 'soda_extend' not in after.source and \
        'SODA_EXTEND' not in after.source
    assert bytes(runtime.make_plan(before)) == bytes(runtime.make_plan(after))
  assert not any('border' in f or 'extend' in f
                 for f in lower.LowerOptions.__dataclass_fields__)


def test_abi_and_structs(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == 9
  assert lib.soda_hip_sizeof(15) == ctypes.sizeof(runtime.PeriodicDesc) == 60
  assert lib.soda_hip_sizeof(17) == ctypes.sizeof(runtime.BorderDesc) == 208
  for name in ('soda_hip_extend_host', 'soda_hip_border_plan',
               'soda_hip_border_create', 'soda_hip_border_destroy',
               'soda_hip_border_info', 'soda_hip_border_fill',
               'soda_hip_border_run_padded', 'soda_hip_border_run_device'):
    assert name in runtime.API and hasattr(lib, name), name
  from soda_amd.codegen.hip import extend
  assert extend.MODES == dict(wrap=0, clamp=1, mirror=2, mirror101=3,
                              constant=4)


def test_command_line_has_the_borders():
  run = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', '--help'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode == 0
  assert '--hip-border' in run.stdout and '--hip-border-value' in run.stdout
  for more in (['--hip-periodic'], ['--hip-until', '1e-3'],
               ['--hip-gpus', '2']):
    run = subprocess.run(
        [sys.executable, '-m', 'soda_amd.sodac', '--hip-backend',
         '--hip-border', 'clamp', '--hip-extent', '64', '8'] + more +
        [soda_path('jacobi2d.soda')],
        capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert run.returncode != 0 and '--hip-border runs on one GPU' in (
        run.stdout + run.stderr), (more, run.stdout, run.stderr)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ct(t):
  return lambda: celltypes.stencil_of(t, 2, 'main', 5)


_J = lambda: _stencil('jacobi2d.soda', iterate=5)
# program name -> (stencil, LowerOptions keywords)
PROGRAMS = {
    'jacobi2d': (_J, dict(fuse=(4,))),
    'skew2d': (lambda: _stencil('skew2d.soda'), {}),
    'coupled2d': (lambda: _stencil('coupled2d.soda'), dict(fuse=(2,))),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=3), dict(fuse=(2,))),
    'blur': (lambda: _stencil('blur.soda'), {}),
    'ints2d': (lambda: _stencil('ints2d.soda'), {}),
    'heat4d': (lambda: _stencil('heat4d.soda', iterate=2),
               dict(strategy='direct')),
    'double': (_ct('double'), dict(fuse=(4,), chunk_rows=16)),
    'uint8': (_ct('uint8'), dict(fuse=(4,), chunk_rows=16)),
}
# case name -> (program, extent, iterate, modes, constants)
CASES = {
    # once per mode, all dimensions alike
    'wrap': ('jacobi2d', (40, 7), 5, 'wrap', None),
    'clamp': ('jacobi2d', (40, 7), 5, 'clamp', None),
    'mirror': ('jacobi2d', (40, 7), 5, 'mirror', None),
    'mirror101': ('jacobi2d', (40, 7), 5, 'mirror101', None),
    'constant': ('jacobi2d', (40, 7), 5, 'constant', -3.5),
    # mixed
    'wrap_clamp': ('jacobi2d', (40, 7), 5, ('wrap', 'clamp'), None),
    'mirror_constant': ('jacobi2d', (40, 7), 5, ('mirror', 'constant'), 2.0),
    # other programs
    'blur': ('blur', (64, 8), 1, ('mirror101', 'mirror'), None),  # one-sided
    'skew2d': ('skew2d', (24, 6), 1, ('constant', 'mirror101'), 2.0),
    'coupled2d': ('coupled2d', (32, 9), 3, 'constant',
                  {'a': 1.5, 'b': -2.0}),       # two pairs, two constants
    'ints2d': ('ints2d', (32, 6), 1, ('clamp', 'constant'), 201),
    'heat3d': ('heat3d', (12, 6, 5), 3, ('mirror', 'clamp', 'wrap'), None),
    'heat4d': ('heat4d', (3, 2, 2, 1), 2, 'mirror101', None),
    'double': ('double', (24, 5), 5, 'mirror', None),
    'uint8': ('uint8', (48, 5), 5, ('constant', 'clamp'), 77),
}
# the rounded ghost_hi[0] is wider than these domains: more than one bounce,
# mirror101 at N = 1
for _m in borders.MODES:
  CASES['2x3_' + _m] = ('jacobi2d', (2, 3), 5, _m, -3.5)
  CASES['1x1_' + _m] = ('jacobi2d', (1, 1), 5, _m, -3.5)

_PROGRAMS = {}
_EXPECTED = {}


@pytest.fixture(scope='module')
def programs(built):
  """Programs by name, made on first use, shared."""
  from soda_amd import runtime

  def get(name):
    if name not in _PROGRAMS:
      make, okw = PROGRAMS[name]
      _PROGRAMS[name] = runtime.Program(make(), _opts(**okw))
    return _PROGRAMS[name]
  yield get
  for prog in _PROGRAMS.values():
    prog.close()
  _PROGRAMS.clear()


def _case(name, seed=0):
  """(program name, stencil, extent, iterate, modes, constants, inputs,
  expected), computed once."""
  key = (name, seed)
  if key not in _EXPECTED:
    pname, extent, iterate, modes, cst = CASES[name]
    stencil = PROGRAMS[pname][0]()
    ins = periodic.inputs(stencil, extent, seed)
    _EXPECTED[key] = (pname, stencil, extent, iterate, modes, cst, ins,
                      borders.expected(stencil, ins, iterate, modes, cst))
  return _EXPECTED[key]


def _dense(prog, bor, ins, iterate, stream=0):
  """The dense entry on device copies of `ins`; {output: array}."""
  st = prog.stencil
  shape = ins[st.input_names[0]].shape
  with periodic.Device(prog) as dev:
    d_in = [dev.upload(ins[n]) for n in st.input_names] + \
        [dev.upload(np.ascontiguousarray(ins[p.name]).reshape(-1))
         for p in st.param_stmts]
    d_out = [dev.alloc(int(np.prod(shape)) * np.dtype(t.np_name).itemsize)
             for t in st.output_types]
    bor.run_device(d_out, d_in, iterate, stream)
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
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  assert all(np.isfinite(w).all() for w in want.values() if w.dtype.kind == 'f')
  prog = programs(pname)
  with prog.bordered(extent, modes, cst) as bor:
    info = bor.info()
    got = _dense(prog, bor, ins, iterate)
  _assert_same(got, want, name)
  all_wrap = set(borders.per_dim(modes, stencil.dim)) == {'wrap'}
  if not all_wrap:
    assert info['refill_every'] == 1
  if name.startswith('1x1_') and not all_wrap:
    assert info['ghost_hi'][0] > extent[0]        # more than one bounce
  if name == 'blur':
    assert info['ghost_lo'] == (0, 0)
  if name == 'clamp':
    # the C oracle agrees with the numpy one on the padded boxes
    from oracle import c_oracle
    _assert_same(borders.expected(
        stencil, ins, iterate, modes, cst,
        run=lambda st, p, it: c_oracle.COracle(st).run(p, iterate=it)),
                 want, 'c_oracle')
  if name in ('constant', 'coupled2d'):
    # numpy in, numpy out
    _assert_same(prog.run_bordered(ins, modes, cst, iterate), want,
                 'run_bordered')


@pytest.mark.gpu
def test_padded_entry_across_calls(programs):
  """Two run_padded calls of 3 and 4 iterations equal one dense run of 7; the
  outputs come back extended; the inputs are byte-identical afterwards."""
  _, stencil, extent, _, _, _, ins, _ = _case('clamp')
  prog = programs('jacobi2d')
  for modes, cst in (('clamp', 0), (('mirror101', 'constant'), -3.5)):
    want = borders.expected(stencil, ins, 7, modes, cst)
    with prog.bordered(extent, modes, cst) as bor, \
        periodic.Device(prog) as dev:
      info = bor.info()
      lo, hi = info['ghost_lo'], info['ghost_hi']
      start = borders.pad(ins['t1'], lo, hi, modes, cst)
      assert start.shape == info['padded'][::-1]
      d0, d1, d2 = dev.upload(start), dev.alloc(start.nbytes), \
          dev.alloc(start.nbytes)
      bor.run_padded([d1], [d0], 3)
      bor.run_padded([d2], [d1], 4)
      after3 = dev.download(d1, start.shape, start.dtype)
      after7 = dev.download(d2, start.shape, start.dtype)
      assert periodic.same_bits(dev.download(d0, start.shape, start.dtype),
                                start)
      dense = _dense(prog, bor, ins, 7)
    _assert_same({'t0': periodic.interior(after7, info)}, want, 'padded 3 + 4')
    _assert_same(dense, want, 'dense 7')
    _assert_same({'t0': periodic.interior(after3, info)},
                 borders.expected(stencil, ins, 3, modes, cst), 'padded 3')
    for arr in (after3, after7):               # extended: ghosts current
      form = borders.closed_form(periodic.interior(arr, info), lo, hi, modes,
                                 cst)
      assert periodic.same_bits(arr, form), periodic.differing(arr, form)


class _DenseEntry:
  """The dense entry with run_device's call shape, for tests/guarded.py."""

  def __init__(self, prog, bor):
    self.device, self.bor = prog.device, bor

  def run_device(self, outputs, inputs, extent, iterate=None, **kw):
    self.bor.run_device(outputs, inputs, iterate, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mirror_constant', 'coupled2d', 'heat3d',
                                  'blur'])
def test_dense_entry_between_guard_bands(programs, name):
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  prog = programs(pname)
  with prog.bordered(extent, modes, cst) as bor:
    got, violation, _ = guarded.run(_DenseEntry(prog, bor), stencil, extent,
                                    ins, iterate)
  assert violation is None, violation
  _assert_same(got, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['clamp', 'mirror_constant', '2x3_mirror101',
                                  '1x1_mirror', 'heat3d', 'blur', 'heat4d',
                                  'double', 'uint8'])
def test_fill_writes_ghost_cells_only(programs, name):
  """A planted pattern: the interior keeps every byte, every ghost cell takes
  what its modes give -- at an address that is aligned to the cell only."""
  pname, stencil, extent, _, modes, cst, _, _ = _case(name)
  prog = programs(pname)
  dtype = np.dtype(stencil.output_types[0].np_name)
  cst = borders.constants_of(stencil, cst)[stencil.input_names[0]]
  with prog.bordered(extent, modes, cst) as bor, periodic.Device(prog) as dev:
    info = bor.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    shape = info['padded'][::-1]
    rng = np.random.default_rng(11)
    for lead in (0, 1, 3):                       # cells behind a 16-byte line
      raw = rng.integers(0, 256, size=(lead + int(np.prod(shape)) + 5) *
                         dtype.itemsize, dtype=np.uint8)
      base = dev.upload(raw)
      bor.fill([base + lead * dtype.itemsize])
      back = dev.download(base, raw.shape, np.uint8)
      cells = lambda b: b[lead * dtype.itemsize:
                          (lead + int(np.prod(shape))) * dtype.itemsize].view(
                              dtype).reshape(shape)
      before, after = cells(raw), cells(back)
      assert periodic.same_bits(periodic.interior(after, info),
                                periodic.interior(before, info))
      form = borders.closed_form(periodic.interior(before, info), lo, hi,
                                 modes, cst)
      assert periodic.same_bits(after, form), periodic.differing(after, form)
      # no byte in front of or behind the array
      n = lead * dtype.itemsize
      assert (back[:n] == raw[:n]).all()
      assert (back[-5 * dtype.itemsize:] == raw[-5 * dtype.itemsize:]).all()


@pytest.mark.gpu
def test_a_constant_fill_keeps_a_nan_payload(programs):
  prog = programs('jacobi2d')
  nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
  extent = (5, 3)
  with prog.bordered(extent, ('constant', 'clamp'), nan) as bor, \
      periodic.Device(prog) as dev:
    info = bor.info()
    arr = np.zeros(info['padded'][::-1], np.float32)
    inner = periodic.interior(arr, info)
    inner[...] = np.arange(inner.size, dtype=np.float32).reshape(inner.shape)
    inner.view(np.uint32)[1, 2] = 0xFFC00077         # and one in the interior
    ptr = dev.upload(arr)
    bor.fill([ptr])
    got = dev.download(ptr, arr.shape, np.float32).view(np.uint32)
  lo, hi = info['ghost_lo'], info['ghost_hi']
  want = borders.closed_form(inner.view(np.uint32), lo, hi,
                             ('constant', 'clamp'), 0x7FC12345)
  assert periodic.same_bits(got, want), periodic.differing(got, want)
  assert (got[:, :lo[0]] == 0x7FC12345).all() and \
      (got[:, lo[0] + extent[0]:] == 0x7FC12345).all()


@pytest.mark.gpu
def test_translation_along_a_wrapped_dimension(programs):
  """(wrap, clamp): rolling the inputs along x rolls the outputs; (mirror,
  wrap): along y."""
  _, stencil, extent, iterate, _, _, ins, _ = _case('clamp')
  prog = programs('jacobi2d')
  for modes, axis, by in ((('wrap', 'clamp'), 1, 3), (('mirror', 'wrap'), 0, 2)):
    roll = lambda a: np.roll(a, by, axis=axis)
    with prog.bordered(extent, modes) as bor:
      plain = _dense(prog, bor, ins, iterate)
      rolled = _dense(prog, bor, {n: roll(a) for n, a in ins.items()}, iterate)
    _assert_same(rolled, {o: roll(a) for o, a in plain.items()}, str(modes))
    assert not all(periodic.same_bits(rolled[o], plain[o]) for o in plain)


@pytest.mark.gpu
def test_all_wrap_is_the_torus(programs):
  """The bits of run_periodic, at the torus's own refill interval."""
  _, stencil, extent, iterate, _, _, ins, want = _case('wrap')
  prog = programs('jacobi2d')
  with prog.bordered(extent, 'wrap') as bor, prog.periodic(extent) as per:
    assert bor.info() == per.info()
    assert bor.info()['refill_every'] == max(
        p.fused_iters for p in prog.module.passes) == 4
    got = _dense(prog, bor, ins, iterate)
  _assert_same(got, prog.run_periodic(ins, iterate), 'run_periodic')
  _assert_same(got, periodic.expected(stencil, ins, iterate), 'torus')
  _assert_same(got, want, 'per iteration')


@pytest.mark.gpu
def test_dense_entry_on_a_side_stream_ahead_of_its_inputs(programs):
  _, stencil, extent, iterate, modes, cst, ins, want = _case('mirror_constant')
  prog = programs('jacobi2d')
  shape = extent[::-1]
  with prog.bordered(extent, modes, cst) as bor:
    _dense(prog, bor, ins, iterate)       # sizes and times the program on P
    got = asyncrun.late_fill(
        'bordered dense entry', ins, {'t0': (shape, np.float32)},
        lambda run: bor.run_device(run.outs(), run.ins(), iterate,
                                   stream=run.ptr))
  _assert_same(got, want, 'late fill')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mirror101', 'heat3d'])
def test_dense_entry_captured_and_replayed(programs, name):
  import torch
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  ins2, want2 = _case(name, seed=5)[6:]
  prog = programs(pname)
  i_name, o_name = stencil.input_names[0], stencil.output_names[0]
  S = torch.cuda.Stream()
  with prog.bordered(extent, modes, cst) as bor:
    t_in = asyncrun._bytes(ins[i_name])
    t_out = asyncrun._bytes(asyncrun.poison_like(want[o_name]))
    read = lambda: t_out.cpu().numpy().view(np.float32).reshape(extent[::-1])
    call = lambda: bor.run_device([t_out.data_ptr()], [t_in.data_ptr()],
                                  iterate, stream=S.cuda_stream)
    torch.cuda.synchronize()
    call()                                        # eager: sizes the scratch
    S.synchronize()
    _assert_same({o_name: read()}, want, name + ', eager')
    warm, held = prog.scratch(), bor.info()['scratch_bytes']
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
    assert prog.scratch() == warm and bor.info()['scratch_bytes'] == held
    del g


@pytest.mark.gpu
def test_refusals_launch_nothing_and_allocate_nothing(programs, built):
  from soda_amd import runtime, util
  _, stencil, extent, iterate, modes, cst, ins, _ = _case('clamp')
  prog = programs('jacobi2d')
  with prog.bordered(extent, modes) as bor:
    _dense(prog, bor, ins, iterate)
  launches, scratch = prog.last_launches(), prog.scratch()
  with pytest.raises(util.InputError, match='unknown mode'):
    prog.bordered(extent, 'reflect')
  with pytest.raises(util.InputError):
    prog.bordered(extent, ('clamp',))
  with pytest.raises(util.InputError, match='no inputs'):
    prog.bordered(extent, 'constant', {'t9': 1.0})
  # the library's own refusals, through the raw entry
  lo, hi = runtime.border_ghosts(stencil, 'clamp')
  for mode, k, what in (((1, 9), 1, 'mode'), ((1, 1), 2, 'refill')):
    desc = runtime._border_desc(runtime._periodic_desc(
        2, extent, k, lo, hi, False), mode, (0,))
    codes, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
    handle = ctypes.c_void_p()
    rc = runtime.library().soda_hip_border_create(
        prog._handle, ctypes.byref(desc), codes, sizes, ctypes.byref(handle))
    assert rc != 0 and not handle.value and what in runtime.last_error()
  assert prog.last_launches() == launches and prog.scratch() == scratch
  assert prog._periodic == []
  # `border: preserve`
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3, border='preserve'),
                       _opts(fuse=(2,))) as pres:
    before = pres.last_launches(), pres.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*preserve'):
      pres.bordered(extent, 'clamp')
    assert (pres.last_launches(), pres.scratch()) == before
  # a batched plan
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3),
                       _opts(fuse=(2,), batch=True)) as bat:
    before = bat.last_launches(), bat.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      bat.bordered(extent, 'mirror')
    assert (bat.last_launches(), bat.scratch()) == before
  # iterate > 1 on sobel2d: refused by both run entries, no byte written
  sobel = _stencil('sobel2d.soda')
  sext = (32, 6)
  sins = periodic.inputs(sobel, sext)
  with runtime.Program(sobel, _opts()) as sp, \
      sp.bordered(sext, 'mirror101') as bor, periodic.Device(sp) as dev:
    info = bor.info()
    got = _dense(sp, bor, sins, 1)                # one iteration is served
    _assert_same(got, borders.expected(sobel, sins, 1, 'mirror101'), 'sobel2d')
    before = sp.last_launches(), sp.scratch(), info['scratch_bytes']
    planted = np.full(info['padded'][::-1], 0xA5A5, np.uint16)
    d_out = dev.upload(planted)
    d_in = dev.upload(borders.pad(sins['img'], info['ghost_lo'],
                                  info['ghost_hi'], 'mirror101'))
    d_dense = dev.upload(sins['img'])
    with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
      bor.run_padded([d_out], [d_in], 2)
    with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
      bor.run_device([d_out], [d_dense], 2)
    with pytest.raises(util.BackendError, match='invalid'):
      bor.run_device([d_out], [d_dense], 0)
    # the contract: an output that is an input
    with pytest.raises(util.BackendError, match='overlaps an input'):
      bor.run_padded([d_in], [d_in], 1)
    assert periodic.same_bits(dev.download(d_out, planted.shape, np.uint16),
                              planted)
    assert (sp.last_launches(), sp.scratch(),
            bor.info()['scratch_bytes']) == before
