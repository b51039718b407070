"""Exact L1 / L2 norms of the residual (soda_hip_norms_t, soda_hip_norms_* and
soda_hip_run_device_norms / _until_norm).

Every comparison is `==`: the counts and every word of both sums against the
oracle of tests/norms.py (Python integers), `value()` against
fractions.Fraction.  The carry and slow-path cases are the ones that catch a
kernel that is merely close.

CPU: fold / value / the plain C++ reduction on random and planted arrays of
every cell type, rounding ties, sums above DBL_MAX, bands, the kernels of all
ten cell types compiled for gfx950 without scratch, the struct's size, the
host functions under a sanitizer in a program of their own, what the feature
leaves untouched.  GPU: seams, carries, the slow path, non-finite deltas,
accumulation without zeroing, runs through a program between guard bands,
run_until, a captured graph, refusals."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import guarded
import norms
import values

TYPES = ('float32', 'float64', 'int8', 'uint8', 'int16', 'uint16', 'int32',
         'uint32', 'int64', 'uint64')


def _stencil(name, **kw):
  from soda_amd import core
  kw = {k: v for k, v in kw.items() if v is not None}
  return core.from_file(soda_path(name), **kw)


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('residual', True)
  return lower.LowerOptions(**kw)


def _plan_box(name, extent, iterate):
  """The box soda_hip_plan_residual_box gives for a program of the corpus."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  plan = runtime.make_plan(lower.lower(_stencil(name, iterate=3),
                                       _opts(peel=0)))
  (lo, hi), = runtime.plan_residual_box(plan, extent, iterate)
  return lo, hi


# ---------------------------------------------------------------------------
# planted arrays: name -> (cur, prev), flat or shaped; run on the CPU through
# soda_hip_norms_host and on the GPU through the kernels
# ---------------------------------------------------------------------------

def _alternating(dtype, big, shape=(6, 1028)):
  """Deltas that alternate between 2^big and 2^-big along the row: no two
  neighbours of a lane share a window."""
  prev = np.zeros(shape, dtype)
  cur = np.empty(shape, dtype)
  cur.reshape(-1)[0::2] = np.ldexp(dtype(1.5), big)
  cur.reshape(-1)[1::2] = np.ldexp(dtype(1.25), -big)
  # ... and along the columns too: a lane meets both in turn
  cur[1::2] = np.roll(cur[1::2], 1, axis=-1)
  return cur, prev


def _planted(name):
  f32, f64 = np.float32, np.float64
  if name == 'two_2^-86':          # sum 2^-85: carries from word 0 to word 1
    cur = np.zeros((3, 40), f32)
    cur[1, 7] = cur[2, 33] = np.ldexp(f32(1), -86)
    return cur, np.zeros_like(cur)
  if name == '4096_x_0x1.fffffep-86':
    cur = np.full((4, 1024), np.float32(float.fromhex('0x1.fffffep-86')), f32)
    return cur, np.zeros_like(cur)
  if name == 'uint64_300':         # l1 and the 128-bit squares carry
    cur = np.full((3, 100), 2**64 - 1, np.uint64)
    prev = np.zeros_like(cur)
    cur[1, 5], prev[1, 5] = 0, 2**64 - 1
    return cur, prev
  if name == 'int8_extremes':
    rng = np.random.default_rng(3)
    cur, prev = norms.random_pair(rng, (5, 48), np.int8)
    cur[0, 0], prev[0, 0] = -128, 127
    cur[4, 47], prev[4, 47] = 127, -128
    cur[2, 16], prev[2, 16] = -128, -128
    return cur, prev
  if name == 'alternating_f32':
    return _alternating(f32, 100)
  if name == 'alternating_f64':
    return _alternating(f64, 1000, shape=(6, 514))
  if name == 'subnormal_f32':
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 23, (4, 260), dtype=np.uint32)
    cur = bits.view(f32).copy()
    prev = np.zeros_like(cur)
    prev[::2] = np.ldexp(f32(1), -149)
    return cur, prev
  if name == 'subnormal_f64':
    rng = np.random.default_rng(6)
    bits = rng.integers(0, 1 << 52, (4, 130), dtype=np.uint64)
    cur = bits.view(f64).copy()
    return cur, np.zeros_like(cur)
  if name == 'one_lane_outside':   # one value far from every other lane's
    rng = np.random.default_rng(8)
    cur, prev = norms.random_pair(rng, (9, 520), f32, spread=3)
    cur[4, 259], prev[4, 259] = np.ldexp(f32(1.75), 120), 0
    cur[5, 259], prev[5, 259] = np.ldexp(f32(1.75), -140), 0
    return cur, prev
  if name == 'wide_spread_f64':    # every exponent of the type, in one grid
    rng = np.random.default_rng(9)
    e = rng.integers(-1070, 1023, (5, 258))
    cur = np.ldexp(1 + rng.random((5, 258)), e).astype(f64)
    return cur, np.zeros_like(cur)
  raise KeyError(name)


CARRIES = ['two_2^-86', '4096_x_0x1.fffffep-86', 'uint64_300', 'int8_extremes']
SLOW = ['alternating_f32', 'alternating_f64', 'subnormal_f32', 'subnormal_f64',
        'one_lane_outside', 'wide_spread_f64']


def _nonfinite(dtype, shape, lo, hi):
  """NaN and both infinities at a fragment seam and at the box's corners; +0
  against -0 beside them."""
  rng = np.random.default_rng(12)
  cur, prev = norms.random_pair(rng, shape, dtype, spread=4)
  corners = [(lo[1], lo[0]), (lo[1], hi[0] - 1), (hi[1] - 1, lo[0]),
             (hi[1] - 1, hi[0] - 1)]
  cur[corners[0]] = np.nan
  cur[corners[1]], prev[corners[1]] = np.inf, 1.0
  cur[corners[2]], prev[corners[2]] = -np.inf, np.inf
  cur[corners[3]], prev[corners[3]] = np.inf, np.inf          # inf - inf: NaN
  # just outside the box: must not count
  cur[lo[1] - 1, lo[0]] = np.nan
  cur[hi[1], hi[0] - 1] = np.inf
  cur[lo[1], lo[0] - 1] = np.inf
  y = (lo[1] + hi[1]) // 2
  for x in (255, 256, 1023, 1024):             # 4- and 1-cell fragment seams
    if lo[0] < x < hi[0] - 1:
      cur[y, x], prev[y, x] = (np.nan, 0) if x % 2 else (np.inf, -1.0)
  cur[y + 1, lo[0] + 1], prev[y + 1, lo[0] + 1] = 0.0, -0.0
  cur[y + 1, lo[0] + 2], prev[y + 1, lo[0] + 2] = -0.0, 0.0
  return cur, prev


def _whole(arr):
  return (0,) * arr.ndim, arr.shape[::-1]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_struct_and_entries(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert runtime.ABI_VERSION == 9 and lib.soda_hip_abi_version() == 9
  assert ctypes.sizeof(runtime.NormsStruct) == 8 * (4 + 34 + 67) == 840
  assert lib.soda_hip_sizeof(14) == ctypes.sizeof(runtime.NormsStruct)
  assert lib.soda_hip_sizeof(13) == 0
  # the structs of ABI 9 are what they were
  assert lib.soda_hip_sizeof(3) == ctypes.sizeof(runtime.Plan)
  assert lib.soda_hip_sizeof(11) == 32
  for name in ('soda_hip_norms_fold', 'soda_hip_norms_value',
               'soda_hip_norms_host', 'soda_hip_norms_create',
               'soda_hip_norms_destroy', 'soda_hip_norms_zero',
               'soda_hip_norms_accumulate', 'soda_hip_run_device_norms',
               'soda_hip_run_device_until_norm'):
    assert name in runtime.API and hasattr(lib, name), name
  from soda_amd.codegen.hip import norms as gen
  assert (gen.L1_WORDS, gen.L2_WORDS) == (norms.L1_WORDS, norms.L2_WORDS)
  assert gen.UNITS == norms.UNITS
  for dt in TYPES:
    cell, size, kind = gen.CELLS[norms.c_type(dt)]
    elem = ctypes.c_int32()
    assert lib.soda_hip_norms_kind_of(cell, ctypes.byref(elem)) == kind
    assert elem.value == size == np.dtype(dt).itemsize
    assert kind == norms.kind_of(dt)


@pytest.mark.parametrize('dtype', TYPES)
def test_host_reduction_on_random_arrays(built, dtype):
  """2-D and 3-D, a box offset on every side, deltas over many binary orders:
  the words, the counts and both rounded values."""
  from soda_amd import runtime
  rng = np.random.default_rng(TYPES.index(dtype))
  for shape, lo, hi in (((7, 19), (2, 1), (17, 6)),
                        ((4, 5, 9), (1, 2, 1), (8, 5, 3)),
                        ((33,), (0,), (33,))):
    cur, prev = norms.random_pair(rng, shape, dtype, spread=60)
    acc = runtime.norms_host(cur, prev, lo, hi)
    want = norms.oracle(norms.cut(cur, lo, hi), norms.cut(prev, lo, hi))
    assert norms.same(acc, want)
    assert want['count'] == int(np.prod([h - l for l, h in zip(lo, hi)]))
    for which in ('l1', 'l2'):
      assert runtime.norms_value(acc, which) == \
          norms.expected_value(want, which), (dtype, which)


@pytest.mark.parametrize('name', CARRIES + SLOW)
def test_host_reduction_on_planted_arrays(built, name):
  from soda_amd import runtime
  cur, prev = _planted(name)
  lo, hi = _whole(cur)
  acc = runtime.norms_host(cur, prev, lo, hi)
  want = norms.oracle(cur, prev)
  assert norms.same(acc, want)
  for which in ('l1', 'l2'):
    assert runtime.norms_value(acc, which) == norms.expected_value(want, which)
  if name == 'two_2^-86':
    assert list(acc.l1[:3]) == [0, 1, 0]
    assert runtime.norms_value(acc, 'l1') == 2.0 ** -85


def test_host_nonfinite(built):
  from soda_amd import runtime
  for dtype in (np.float32, np.float64):
    lo, hi = (3, 2), (1030, 7)
    cur, prev = _nonfinite(dtype, (9, 1034), lo, hi)
    acc = runtime.norms_host(cur, prev, lo, hi)
    want = norms.oracle(norms.cut(cur, lo, hi), norms.cut(prev, lo, hi))
    assert norms.same(acc, want)
    assert want['unordered'] >= 3 and want['infinite'] >= 3
    assert want['count'] + want['unordered'] + want['infinite'] == \
        (hi[0] - lo[0]) * (hi[1] - lo[1])
    assert runtime.norms_value(acc, 'l1') == float('inf')
    assert runtime.norms_value(acc, 'l2') == float('inf')
    acc.infinite = 0
    assert math.isfinite(runtime.norms_value(acc, 'l1'))
  # +0 against -0 adds nothing
  z = runtime.norms_host(np.zeros(8, np.float32), np.full(8, -0.0, np.float32),
                         (0,), (8,))
  assert z.count == 8 and z.l1_int() == 0 and z.l2_int() == 0


def _struct(kind, l1=0, l2=0, **kw):
  from soda_amd import runtime
  acc = runtime.NormsStruct()
  acc.kind = kind
  for i, w in enumerate(norms.words(l1, norms.L1_WORDS)):
    acc.l1[i] = w
  for i, w in enumerate(norms.words(l2, norms.L2_WORDS)):
    acc.l2[i] = w
  for k, v in kw.items():
    setattr(acc, k, v)
  return acc


def test_value_rounds_to_nearest_even(built):
  from soda_amd import runtime
  rng = np.random.default_rng(21)
  cases = [2**53 + 1, 2**53 + 3, 2**54 + 2, 2**54 + 6, 2**53 - 1, 1, 0,
           (2**53 + 1) << 700, ((2**53 + 1) << 700) + 1,
           ((2**53 + 1) << 700) - 1, (2**54 - 1) << 900, 2**2161 + 2**2100]
  cases += [int(rng.integers(1, 2**62)) << int(rng.integers(0, 2000)) |
            int(rng.integers(0, 2**62)) for _ in range(200)]
  for kind in norms.UNITS:
    for n in cases:
      for which, nwords in (('l1', norms.L1_WORDS), ('l2', norms.L2_WORDS)):
        if n >= 1 << (64 * nwords):
          continue
        acc = _struct(kind, **{which: n})
        want = norms.expected_value(dict(kind=kind, infinite=0, **{which: n}),
                                    which)
        assert runtime.norms_value(acc, which) == want, (kind, which, n)
  # the subnormal range of fp64 squares: rounds at 2^-1074, ties to even
  for n, want in ((1 << 1073, 0.0), ((1 << 1073) + 1, 2.0 ** -1074),
                  (3 << 1073, 2.0 ** -1073), (1 << 1074, 2.0 ** -1074),
                  (1 << 1000, 0.0), (5 << 1073, 2.0 ** -1073)):
    acc = _struct(norms.KIND_F64, l2=n)
    assert runtime.norms_value(acc, 'l2') == want == norms.expected_value(
        dict(kind=norms.KIND_F64, infinite=0, l2=n), 'l2'), n


def test_a_sum_above_dbl_max(built):
  from soda_amd import runtime
  big = np.finfo(np.float64).max
  cur = np.array([big, big, 1.0, big])
  prev = np.array([0.0, -big, 0.0, 0.0])      # big - -big: an infinite delta
  acc = runtime.norms_host(cur, prev, (0,), (1,))
  assert runtime.norms_value(acc, 'l1') == big           # DBL_MAX itself fits
  assert runtime.norms_value(acc, 'l2') == float('inf')
  acc = runtime.norms_host(cur, prev, (2,), (4,))        # 1 + DBL_MAX
  assert acc.infinite == 0 and runtime.norms_value(acc, 'l1') == big
  acc = runtime.norms_host(cur[[0, 3]], prev[[0, 3]], (0,), (2,))
  assert acc.infinite == 0 and acc.count == 2
  assert norms.same(acc, norms.oracle(cur[[0, 3]], prev[[0, 3]]))
  assert runtime.norms_value(acc, 'l1') == float('inf')  # finite cells, no room
  acc = runtime.norms_host(cur, prev, (0,), (4,))
  assert acc.infinite == 1 and runtime.norms_value(acc, 'l1') == float('inf')
  # the struct takes 2^64 cells of DBL_MAX: the top words hold them
  top = _struct(norms.KIND_F64, l1=(2**1024 - 2**971) * 2**1074 * (2**64 - 1))
  assert top.l1[33] != 0 and runtime.norms_value(top, 'l1') == float('inf')


def test_fold_of_row_bands_is_the_whole_grid(built):
  from soda_amd import runtime, util
  rng = np.random.default_rng(4)
  for dtype in ('float32', 'float64', 'int16', 'uint64'):
    cur, prev = norms.random_pair(rng, (23, 37), dtype, spread=50)
    lo, hi = (2, 1), (35, 22)
    whole = runtime.norms_host(cur, prev, lo, hi)
    total = runtime.norms_empty(norms.c_type(dtype))
    for a, b in ((1, 2), (2, 9), (9, 9), (9, 22)):
      band = runtime.norms_host(cur, prev, (lo[0], a), (hi[0], b))
      assert runtime.norms_fold(total, band) is total
    assert bytes(total) == bytes(whole)
    assert norms.same(total, norms.oracle(norms.cut(cur, lo, hi),
                                          norms.cut(prev, lo, hi)))
    # ... and adding into one struct is the same as folding
    into = runtime.norms_empty(norms.c_type(dtype))
    for a, b in ((1, 9), (9, 22)):
      runtime.norms_host(cur, prev, (lo[0], a), (hi[0], b), acc=into)
    assert bytes(into) == bytes(whole)
  with pytest.raises(util.BackendError):
    runtime.norms_fold(runtime.norms_empty('float'),
                       runtime.norms_empty('double'))
  with pytest.raises(util.BackendError):          # a box outside the arrays
    runtime.norms_host(np.zeros((3, 4), np.float32),
                       np.zeros((3, 4), np.float32), (0, 0), (5, 3))


@pytest.mark.parametrize('dtype', TYPES)
def test_the_kernels_compile_without_scratch(built, dtype):
  """The norms module of every cell type, for gfx950: one kernel per fragment
  width from 16 bytes down to one cell, none with scratch, the block's words in
  840 bytes of LDS.  (DESIGN.md 4.10 records the register counts.)"""
  from soda_amd import runtime
  from soda_amd.codegen.hip import norms as gen
  ct = norms.c_type(dtype)
  for dim in ((2, 3) if dtype in ('float32', 'float64') else (2,)):
    _, res = runtime.norms_resources(ct, dim)
    names = [gen.kernel_name(ct, v) for v in gen.widths(ct)]
    assert gen.widths(ct)[0] * np.dtype(dtype).itemsize == 16
    assert gen.widths(ct)[-1] == 1
    assert sorted(res) == sorted(names + ['soda_norms_zero'])
    for n in names:
      assert res[n]['scratch'] == 0, (n, res[n])
      assert 0 < res[n]['vgpr'] <= 64, (n, res[n])
      assert res[n]['lds'] == 840
    assert res['soda_norms_zero']['scratch'] == 0


def test_residual_modules_are_untouched():
  """A `residual=True` module is what it was: its text, kernels and plan know
  nothing of the norms, whether or not the norms code was ever imported."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  for name, kw in (('jacobi2d.soda', dict(fuse=(13, 4))),
                   ('heat3d.soda', dict(fuse=(2,)))):
    stencil = _stencil(name, iterate=13)
    before = lower.lower(stencil, _opts(peel=0, **kw))
    from soda_amd.codegen.hip import norms as gen
    gen.source('float', stencil.dim)
    after = lower.lower(stencil, _opts(peel=0, **kw))
    assert before.source == after.source
    assert 'norms' not in after.source
    assert [k.name for k in before.kernels] == [k.name for k in after.kernels]
    assert not any('norms' in k.name for k in after.kernels)
    assert bytes(runtime.make_plan(before)) == bytes(runtime.make_plan(after))
  # and no LowerOptions field was added for it
  assert not any('norm' in f for f in lower.LowerOptions.__dataclass_fields__)


def test_host_functions_under_a_sanitizer(built, tmp_path):
  """tests/host/norms_main.cpp + soda_norms.cpp as one program with its own
  main, -fsanitize=address,undefined: nothing loaded into Python."""
  exe = os.path.join(str(tmp_path), 'norms_main')
  subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
                  '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined',
                  '-I', os.path.join(ROOT, 'include'),
                  os.path.join(ROOT, 'tests', 'host', 'norms_main.cpp'),
                  os.path.join(ROOT, 'soda_amd', 'csrc', 'soda_norms.cpp'),
                  '-o', exe], check=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 0 and run.stdout.startswith('OK'), (
      run.stdout + run.stderr)


def test_command_line_has_the_norm():
  run = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', '--help'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode == 0
  assert '--hip-norm' in run.stdout and '{max,l1,l2}' in run.stdout


def test_python_refusals_without_a_gpu(built):
  from soda_amd import runtime, util
  with pytest.raises(util.InputError, match='norms'):
    runtime.norms_empty('half')
  with pytest.raises(util.InputError, match='one dtype and shape'):
    runtime.norms_host(np.zeros(4, np.float32), np.zeros(4, np.float64), (0,),
                       (4,))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

_HANDLES = {}


@pytest.fixture(scope='module')
def handles(built):
  """Norms handles by (dtype, dim), made on first use."""
  from soda_amd import runtime

  def get(dtype, dim):
    key = (np.dtype(dtype).name, dim)
    if key not in _HANDLES:
      _HANDLES[key] = runtime.Norms(norms.c_type(dtype), dim)
    return _HANDLES[key]

  yield get
  for h in _HANDLES.values():
    h.close()
  _HANDLES.clear()


def _on_device(handles, cur, prev, boxes, zero=True):
  """The struct after accumulating every box of `boxes` into one (0xFF bytes
  before the zeroing kernel)."""
  nm = handles(cur.dtype, cur.ndim)
  with norms.Device() as dev:
    dc, dp = dev.upload(cur), dev.upload(prev)
    acc = dev.alloc(840, fill=0xFF)
    if zero:
      nm.zero(acc)
    for lo, hi in boxes:
      nm.accumulate(dc, dp, cur.shape[::-1], lo, hi, acc)
    got = nm.fetch(acc)
    # the arrays are only read
    assert np.array_equal(dev.download(dc, cur.shape, cur.dtype).view(np.uint8),
                          cur.view(np.uint8))
    assert np.array_equal(dev.download(dp, prev.shape, prev.dtype).view(np.uint8),
                          prev.view(np.uint8))
  return got


SEAMS = [
    # dtype, extent, program of the box, iterate of the box
    ('float32', (1030, 7), 'jacobi2d.soda', 3),    # rows of 2-cell fragments
    ('float32', (200, 9), 'jacobi2d.soda', 3),
    ('float32', (1028, 7), 'jacobi2d.soda', 3),    # 257 4-cell fragments a row
    ('float32', (1030, 7), 'jacobi2d.soda', 1),
    ('int16', (1030, 7), 'jacobi2d.soda', 3),
    ('int16', (200, 9), 'jacobi2d.soda', 3),
    ('int16', (2056, 5), 'jacobi2d.soda', 1),      # 257 8-cell fragments a row
    ('float64', (72, 5, 6), 'heat3d.soda', 3),     # (this box is empty)
    ('float64', (72, 5, 6), 'heat3d.soda', 1),
    ('float64', (515, 5, 6), 'heat3d.soda', 1),    # one-cell fragments, 3 segments
]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,extent,name,iterate', SEAMS)
def test_seams(handles, dtype, extent, name, iterate):
  """Rows that are not whole 16-byte fragments, rows a little longer than a
  segment of 256 fragments, the box soda_hip_plan_residual_box gives -- offset
  from the array on every side -- and the whole array."""
  from soda_amd import runtime
  lo, hi = _plan_box(name, extent, iterate)
  assert all(l > 0 and h < e for l, h, e in zip(lo, hi, extent))
  rng = np.random.default_rng(len(extent) * 100 + extent[0])
  cur, prev = norms.random_pair(rng, extent[::-1], dtype, spread=20)
  got = _on_device(handles, cur, prev, [(lo, hi)])
  want = norms.oracle(norms.cut(cur, lo, hi), norms.cut(prev, lo, hi))
  assert norms.same(got, want)
  assert bytes(got) == bytes(runtime.norms_host(cur, prev, lo, hi))
  whole = _on_device(handles, cur, prev, [_whole(cur)])
  assert norms.same(whole, norms.oracle(cur, prev))
  assert whole.count == cur.size


@pytest.mark.gpu
@pytest.mark.parametrize('name', CARRIES)
def test_carries(handles, name):
  from soda_amd import runtime
  cur, prev = _planted(name)
  got = _on_device(handles, cur, prev, [_whole(cur)])
  assert norms.same(got, norms.oracle(cur, prev))
  if name == 'two_2^-86':
    assert list(got.l1[:3]) == [0, 1, 0]
  if name == 'uint64_300':
    assert list(got.l1[:3]) == [2**64 - 300, 299, 0]
    assert list(got.l2[:4]) == [300, 2**64 - 600, 299, 0]
  for which in ('l1', 'l2'):
    assert runtime.norms_value(got, which) == \
        norms.expected_value(norms.oracle(cur, prev), which)


@pytest.mark.gpu
@pytest.mark.parametrize('name', SLOW)
def test_slow_path_is_exact(handles, name):
  """Deltas no window holds together: every one sends its lane to the block's
  words.  The words are the oracle's all the same -- that is the point."""
  cur, prev = _planted(name)
  got = _on_device(handles, cur, prev, [_whole(cur)])
  assert norms.same(got, norms.oracle(cur, prev))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_nonfinite_deltas(handles, dtype):
  from soda_amd import runtime
  lo, hi = (3, 2), (1030, 7)
  cur, prev = _nonfinite(np.dtype(dtype).type, (9, 1034), lo, hi)
  got = _on_device(handles, cur, prev, [(lo, hi)])
  want = norms.oracle(norms.cut(cur, lo, hi), norms.cut(prev, lo, hi))
  assert norms.same(got, want)
  assert got.unordered >= 3 and got.infinite >= 3
  assert runtime.norms_value(got, 'l1') == float('inf')
  assert runtime.norms_value(got, 'l2') == float('inf')
  # +0 against -0 adds nothing
  z = _on_device(handles, np.zeros((3, 64), dtype), np.full((3, 64), -0.0, dtype),
                 [((0, 0), (64, 3))])
  assert z.count == 192 and z.l1_int() == 0 and z.l2_int() == 0
  assert z.unordered == 0 and z.infinite == 0


@pytest.mark.gpu
def test_accumulate_without_zeroing(handles):
  """Two disjoint boxes into one struct are one call over their union; two
  structs filled on the device fold on the host to the same bytes."""
  from soda_amd import runtime
  rng = np.random.default_rng(31)
  cur, prev = norms.random_pair(rng, (21, 1036), np.float32, spread=30)
  a, b = ((4, 2), (1030, 9)), ((4, 9), (1030, 20))
  union = ((4, 2), (1030, 20))
  both = _on_device(handles, cur, prev, [a, b])
  one = _on_device(handles, cur, prev, [union])
  assert bytes(both) == bytes(one)
  assert norms.same(one, norms.oracle(norms.cut(cur, *union),
                                      norms.cut(prev, *union)))
  sa = _on_device(handles, cur, prev, [a])
  sb = _on_device(handles, cur, prev, [b])
  assert bytes(runtime.norms_fold(sa, sb)) == bytes(one)
  # an empty box launches nothing and adds nothing
  none = _on_device(handles, cur, prev, [((5, 5), (5, 9))])
  assert none.count == 0 and none.kind == norms.KIND_F32
  assert none.l1_int() == 0 and none.l2_int() == 0


_ORACLES = {}


def _states(stencil, ins, iterate):
  """({output: array after `iterate`}, {output: array after iterate - 1}) from
  the C oracle."""
  from oracle import c_oracle
  key = str(stencil)
  if key not in _ORACLES:
    _ORACLES[key] = c_oracle.COracle(stencil, openmp=False)
  cur = _ORACLES[key].run(ins, iterate=iterate)
  if iterate > 1:
    prev = _ORACLES[key].run(ins, iterate=iterate - 1)
  else:
    prev = {o: np.asarray(ins[i]) for i, o in zip(stencil.input_names,
                                                  stencil.output_names)}
  return cur, prev


def _expected(stencil, ins, extent, iterate):
  cur, prev = _states(stencil, ins, iterate)
  want = None
  for o in stencil.output_names:
    lo, hi = stencil.valid_box(extent, o, iterate)
    want = norms.oracle(norms.cut(cur[o], lo, hi), norms.cut(prev[o], lo, hi),
                        into=want)
  return want, cur


def _inputs(stencil, extent, seed=7):
  rng = np.random.default_rng(seed)
  return {n: rng.random(extent[::-1], dtype=np.float64).astype(t.np_name)
          for n, t in zip(stencil.input_names, stencil.input_types)}


PROGRAMS = [
    ('jacobi2d.soda', dict(fuse=(13, 4), chunk_rows=16, peel=1), 13,
     (520, 120), (1, 5, 14)),
    ('heat3d.soda', dict(fuse=(2,), chunk_rows=8, peel=1), 3, (72, 24, 36),
     (3,)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,kw,build_iterate,extent,iterates', PROGRAMS,
                         ids=['jacobi2d', 'heat3d'])
def test_through_the_program(built, name, kw, build_iterate, extent, iterates):
  """run_device(norms=...) between guard bands: the struct is the oracle's over
  the states N and N - 1 of the C oracle, the outputs are those of a plain
  run bit for bit, no byte outside the outputs and the struct is written, the
  run ends in the one-iteration pass."""
  from soda_amd import runtime
  stencil = _stencil(name, iterate=build_iterate)
  ins = _inputs(stencil, extent)
  with runtime.Program(stencil, _opts(**kw), calibrate=False) as prog, \
      norms.Device() as dev:
    band = 4096
    arena = dev.alloc(2 * band + 840, fill=0xA5)
    for iterate in iterates:
      want, cur = _expected(stencil, ins, extent, iterate)
      outs, bad, _ = guarded.run(prog, stencil, extent, ins, iterate,
                                 norms=arena + band)
      assert bad is None, bad
      assert prog.last_residual() == ('generic', 1)
      img = dev.download(arena, (2 * band + 840,), np.uint8)
      assert (img[:band] == 0xA5).all() and (img[band + 840:] == 0xA5).all()
      got = runtime.NormsStruct.from_buffer_copy(img[band:band + 840].tobytes())
      assert norms.same(got, want), iterate
      assert got.count > 0
      plain, bad, _ = guarded.run(prog, stencil, extent, ins, iterate)
      assert bad is None, bad
      for o in stencil.output_names:
        lo, hi = stencil.valid_box(extent, o, iterate)
        assert values.same_bits(norms.cut(outs[o], lo, hi),
                                norms.cut(plain[o], lo, hi)).all()
        assert values.same_bits(norms.cut(outs[o], lo, hi),
                                norms.cut(cur[o], lo, hi)).all()
      dev.rt.check(dev.lib.soda_hip_memset(ctypes.c_void_p(arena), 0xA5,
                                           2 * band + 840, None), 'memset')


@pytest.mark.gpu
def test_run_until_a_norm_is_small(built):
  """jacobi2d border='preserve' at 64 x 40, a look every 8 iterations: stops
  where a Python loop over the oracle stops, with the oracle's struct and
  outputs; norm=None is today's entry."""
  from soda_amd import runtime
  stencil = _stencil('jacobi2d.soda', iterate=8, border='preserve')
  extent = (64, 40)
  ins = {'t1': np.random.default_rng(7).random((40, 64), dtype=np.float32)}
  keep = ins['t1'].copy()
  with runtime.Program(stencil, _opts(fuse=(8, 4), peel=1),
                       calibrate=False) as prog:
    for which, tol in (('l2', 0.03), ('l1', 1.0)):
      stop, want, cur = None, None, None
      for n in range(8, 201, 8):
        want, cur = _expected(stencil, ins, extent, n)
        v = norms.expected_value(want, which)
        if want['unordered'] == 0 and want['infinite'] == 0 and \
            (math.sqrt(v) if which == 'l2' else v) <= tol:
          stop = n
          break
      assert stop is not None and 16 <= stop <= 48, (which, stop)
      outs, done, acc = prog.run_until(ins, tol, 200, check_every=8, norm=which)
      assert done == stop, (which, done, stop)
      assert isinstance(acc, runtime.NormsStruct) and norms.same(acc, want)
      assert values.same_bits(outs['t0'], cur['t0']).all()
      assert np.array_equal(ins['t1'], keep)
    # the limit reached unconverged, after an odd and an even number of chunks
    for limit in (8, 16, 20):
      want, cur = _expected(stencil, ins, extent, limit)
      outs, done, acc = prog.run_until(ins, 0.0, limit, check_every=8,
                                       norm='l2')
      assert done == limit and norms.same(acc, want)
      assert values.same_bits(outs['t0'], cur['t0']).all()
    # norm=None: the struct and the count of today's entry
    a = prog.run_until(ins, 2.0 ** -8, 200, check_every=8)
    b = prog.run_until(ins, 2.0 ** -8, 200, check_every=8, norm=None)
    assert isinstance(a[2], runtime.Residual) and a[1:] == b[1:]
    assert 16 <= a[1] <= 32
    assert values.same_bits(a[0]['t0'], b[0]['t0']).all()


@pytest.mark.gpu
def test_capture_and_replay(handles):
  """zero + accumulate captured once after an eager run, replayed three times
  on changed inputs: every replay is its oracle's.  A linear graph: two kernel
  nodes on one stream."""
  import torch
  nm = handles(np.float32, 2)
  extent = (1030, 12)
  lo, hi = (3, 2), (1027, 10)
  rng = np.random.default_rng(41)
  pairs = [norms.random_pair(rng, extent[::-1], np.float32, spread=25)
           for _ in range(4)]
  S = torch.cuda.Stream()
  cur = torch.from_numpy(pairs[0][0]).cuda()
  prev = torch.from_numpy(pairs[0][1]).cuda()
  acc = torch.full((105,), -1, dtype=torch.int64, device='cuda')
  torch.cuda.synchronize()

  def enqueue():
    nm.zero(acc.data_ptr(), stream=S.cuda_stream)
    nm.accumulate(cur.data_ptr(), prev.data_ptr(), extent, lo, hi,
                  acc.data_ptr(), stream=S.cuda_stream)

  def struct():
    from soda_amd import runtime
    return runtime.NormsStruct.from_buffer_copy(acc.cpu().numpy().tobytes())

  def want(k):
    return norms.oracle(norms.cut(pairs[k][0], lo, hi),
                        norms.cut(pairs[k][1], lo, hi))

  enqueue()
  S.synchronize()
  assert norms.same(struct(), want(0))
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g, stream=S):
    enqueue()
  for k in (1, 2, 3):
    cur.copy_(torch.from_numpy(pairs[k][0]))
    prev.copy_(torch.from_numpy(pairs[k][1]))
    acc.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert norms.same(struct(), want(k)), k
  del g


MIXED_2D = '''kernel: mixed2d
burst width: 64
unroll factor: 2
iterate: 2
input float: a(32, *)
input int32: c(32, *)
output float: b(0, 0) = (a(0, 1) + a(0, -1)) * 0.5f
output int32: d(0, 0) = c(1, 0) - c(-1, 0)
'''


@pytest.mark.gpu
def test_refusals(built):
  """A program without `residual`; pairs of two kinds; `batch`: nothing is
  launched, no byte is written."""
  from soda_amd import core, runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=2)
  extent = (256, 24)
  nbytes = 256 * 24 * 4
  with norms.Device() as dev:
    a = dev.alloc(nbytes, fill=0)
    b = dev.alloc(nbytes, fill=0xA5)
    acc = dev.alloc(840, fill=0xA5)
    with runtime.Program(stencil, lower.LowerOptions(fuse=(2,), peel=0),
                         calibrate=False) as plain:
      with pytest.raises(util.BackendError, match='(?i)unsupported|cannot serve'):
        plain.run_device([b], [a], extent, norms=acc)
      assert plain.last_launches()[0] == 0
      with pytest.raises(util.BackendError, match='residual'):
        plain.run_until({'t1': np.zeros((24, 256), np.float32)}, 0.0, 4,
                        norm='l2')
    with runtime.Program(stencil, _opts(fuse=(2,), peel=0),
                         calibrate=False) as prog:
      with pytest.raises(util.InputError, match='batch'):
        prog.run_device([b], [a], extent, norms=acc, batch=2)
      with pytest.raises(util.InputError, match='residual'):
        prog.run_device([b], [a], extent, norms=acc, residual=acc)
      with pytest.raises(util.BackendError, match='aligned'):
        prog.run_device([b], [a], extent, norms=acc + 4)
      with pytest.raises(util.BackendError, match='overlaps'):
        prog.run_device([b], [a], extent, norms=b + 64)
      # a handle of another cell size is not this program's
      with runtime.Norms('double', 2) as wide:
        rc = prog._lib.soda_hip_run_device_norms(
            prog._handle, wide._handle, (ctypes.c_void_p * 1)(b),
            (ctypes.c_void_p * 1)(a), (ctypes.c_int32 * 2)(*extent), 2,
            ctypes.c_void_p(acc), None)
        assert rc == 6                              # SODA_HIP_ERR_UNSUPPORTED
      with pytest.raises(util.InputError, match="norm is None, 'l1' or 'l2'"):
        prog.run_until({'t1': np.zeros((24, 256), np.float32)}, 0.0, 4,
                       norm='max')
    mixed = core.from_text(MIXED_2D)
    with runtime.Program(mixed, _opts(peel=0), calibrate=False) as prog:
      c, d = dev.alloc(nbytes, fill=0), dev.alloc(nbytes, fill=0xA5)
      with pytest.raises(util.InputError, match='one kind of units'):
        prog.run_device([b, d], [a, c], extent, norms=acc)
    dev.sync()
    assert (dev.download(b, (nbytes,), np.uint8) == 0xA5).all()
    assert (dev.download(acc, (840,), np.uint8) == 0xA5).all()
