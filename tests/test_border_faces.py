"""Bordered domains with a border mode and a constant per FACE
(soda_hip_border_faces_t, the `_faces` entries, soda_hip_extend_faces_host;
DESIGN.md 4.16).

Every comparison is on bit patterns.  The expected value is that of
tests/faces.py: for every dimension, dimension 0 first, the low part is np.pad
in the low face's mode and the high part np.pad in the high face's, both of
the array as it stood before that dimension; programs advance one iteration at
a time on inputs re-extended that way.

CPU: the host twin against that closed form on all 16 pairs of wall modes,
four cell sizes, frames wider than the domain, the corner rule, a NaN payload;
a symmetric request is extend_host; refusals; the plan twins; the faces kernels
compiled for gfx950; what the feature leaves untouched; the host twin under a
sanitizer in a program of its own; the command line.
GPU: fills, the dense and the padded entry, the fused form, batches,
convergence on a plate with a hot and a cold wall, the identity of a symmetric
request, refusals, a captured graph, random programs."""
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
import domains
import faces
import fuzz_nest
import guarded
import norms
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


def _cells(rng, extent, size):
  raw = rng.integers(0, 256, size=extent[::-1] + (size,), dtype=np.uint8)
  return np.ascontiguousarray(raw).view(SIZES[size]).reshape(extent[::-1])


def _planted(domain, lo, hi):
  """A padded array whose interior is `domain` and whose ghosts are garbage."""
  shape = tuple(l + n + h for l, n, h in zip(lo[::-1], domain.shape, hi[::-1]))
  arr = np.full(shape, 0x5A, domain.dtype)
  periodic.interior(arr, dict(ghost_lo=lo, ghost_hi=hi))[...] = domain
  return arr


def _same(got, want, what):
  assert periodic.same_bits(got, want), (what, periodic.differing(got, want))


def _assert_same(got, want, what):
  assert sorted(got) == sorted(want)
  for o in want:
    assert periodic.same_bits(got[o], want[o]), \
        '%s: %d cells of %s differ in their bits' % (
            what, periodic.differing(got[o], want[o]), o)


# ---------------------------------------------------------------------------
# CPU: the host twin
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('where', [0, 1])
def test_host_twin_on_every_pair(built, size, where):
  """All 16 pairs of the four wall modes and (wrap, wrap) in dimension
  `where` of a 3 x 5 domain under ghosts (4, 6) / (7, 2): mirrors bounce more
  than once; the other dimension has a pair of its own."""
  from soda_amd import runtime
  lo, hi = (4, 6), (7, 2)
  rng = np.random.default_rng(size + where)
  domain = _cells(rng, (3, 5), size)
  mask = (1 << (8 * size)) - 1
  cst = [tuple(SIZES[size]((0xF1E2D3C4B5A69788 + 0x0101010101010101 * k) & mask)
               for k in (2 * d, 2 * d + 1)) for d in range(2)]
  other = ('constant', 'mirror101')
  for pair in faces.PAIRS:
    for spelled in (pair, '/'.join(pair)):
      modes = [spelled, other] if where == 0 else [other, spelled]
      want = faces.pad(domain, lo, hi, modes, cst)
      got = _planted(domain, lo, hi)
      assert runtime.extend_host(got, lo, hi, modes, cst) is got
      _same(got, want, modes)


def test_host_twin_other_shapes(built):
  """N = 1 in a dimension, one 3-D and one 4-D case, one-sided frames."""
  from soda_amd import runtime
  rng = np.random.default_rng(9)
  cases = [
      ((1, 4), (3, 2), (2, 3),
       [('mirror101', 'mirror'), ('clamp', 'constant')]),
      ((6, 1), (2, 5), (0, 4), [('constant', 'clamp'), ('mirror', 'mirror101')]),
      ((6, 4, 3), (1, 2, 0), (2, 0, 4),
       [('clamp', 'constant'), 'wrap', ('constant', 'mirror')]),
      ((5, 3, 2, 2), (1, 0, 2, 1), (0, 2, 1, 3),
       [('mirror', 'clamp'), 'mirror101/constant', ('constant', 'constant'),
        ('wrap', 'wrap')]),
  ]
  for extent, lo, hi, modes in cases:
    for size in sorted(SIZES):
      domain = _cells(rng, extent, size)
      cst = [(SIZES[size](3 + 2 * d), SIZES[size](4 + 2 * d))
             for d in range(len(extent))]
      got = _planted(domain, lo, hi)
      runtime.extend_host(got, lo, hi, modes, cst)
      _same(got, faces.pad(domain, lo, hi, modes, cst), (extent, modes, size))


def test_the_corner_rule(built):
  """Four distinct constants: a corner takes that of dimension 1 -- the
  highest -- and of the face it is outside through; next to a clamped face of
  dimension 1 it takes dimension 0's."""
  from soda_amd import runtime
  lo, hi = (2, 1), (1, 2)
  domain = np.arange(12, dtype=np.int32).reshape(3, 4) + 100
  cst = [(1, 2), (3, 4)]
  got = _planted(domain, lo, hi)
  runtime.extend_host(got, lo, hi, 'constant', cst)
  _same(got, faces.pad(domain, lo, hi, 'constant', cst), 'constant')
  assert (got[0] == 3).all() and (got[-2:] == 4).all()      # whole rows
  assert (got[1:4, :2] == 1).all() and (got[1:4, -1:] == 2).all()
  mixed = [('constant', 'constant'), ('constant', 'clamp')]
  got = _planted(domain, lo, hi)
  runtime.extend_host(got, lo, hi, mixed, cst)
  _same(got, faces.pad(domain, lo, hi, mixed, cst), mixed)
  assert (got[0] == 3).all()
  assert (got[-2:, :2] == 1).all() and (got[-2:, -1:] == 2).all()
  assert (got[-2:, 2:6] == domain[-1]).all()


def test_a_nan_payload_as_a_face_constant(built):
  from soda_amd import runtime
  nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
  other = np.array([0xFFC00001], np.uint32).tobytes()
  lo, hi = (2, 1), (3, 2)
  a = np.zeros((2 + 1 + 1, 2 + 4 + 3), np.float32)
  periodic.interior(a, dict(ghost_lo=lo, ghost_hi=hi))[...] = 1.0
  runtime.extend_host(a, lo, hi, [('constant', 'constant'), 'clamp'],
                      [(nan, other), 0.0])
  bits = a.view(np.uint32)
  assert (bits[:, :2] == 0x7FC12345).all() and (bits[:, 6:] == 0xFFC00001).all()
  assert (bits[:, 2:6] == 0x3F800000).all()


def test_a_symmetric_request_is_extend_host(built):
  from soda_amd import runtime
  rng = np.random.default_rng(4)
  domain = _cells(rng, (5, 3), 4)
  lo, hi = (4, 6), (7, 2)
  for m0 in borders.MODES:
    for m1 in borders.MODES:
      want = runtime.extend_host(_planted(domain, lo, hi), lo, hi, (m0, m1), 77)
      _same(want, borders.pad(domain, lo, hi, (m0, m1), 77), (m0, m1))
      for modes, cst in ((((m0, m0), (m1, m1)), 77),
                         ((m0 + '/' + m0, m1), [(77, 77), 77]),
                         ((m0, m1), [77, (77, 77)])):
        got = runtime.extend_host(_planted(domain, lo, hi), lo, hi, modes, cst)
        _same(got, want, modes)
  # the library's twin itself, on equal pairs and one constant
  i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
  got = _planted(domain, lo, hi)
  assert runtime.library().soda_hip_extend_faces_host(
      got.ctypes.data, 4, 2, i32(5, 3), i32(*lo), i32(*hi), i32(2, 4),
      i32(2, 4), (ctypes.c_uint64 * 4)(9, 9, 9, 9)) == 0
  _same(got, borders.pad(domain, lo, hi, ('mirror', 'constant'), 9), 'raw')


def test_refusals_without_a_gpu(built):
  from soda_amd import runtime, util
  a = np.zeros((4, 6), np.float32)
  for modes in (('wrap', 'clamp'), 'clamp/wrap'):
    with pytest.raises(util.InputError, match='wraps on both faces or on none'):
      runtime.extend_host(a, (1, 1), (1, 1), [modes, 'clamp'])
  with pytest.raises(util.InputError, match='unknown mode'):
    runtime.extend_host(a, (1, 1), (1, 1), [('clamp', 'reflect'), 'clamp'])
  with pytest.raises(util.InputError, match='unknown mode'):
    runtime.extend_host(a, (1, 1), (1, 1), 'clamp/edge')
  with pytest.raises(util.InputError, match='pair'):
    runtime.extend_host(a, (1, 1), (1, 1),
                        [('clamp', 'mirror', 'clamp'), 'clamp'])
  with pytest.raises(util.InputError, match='pair'):
    runtime.extend_host(a, (1, 1), (1, 1), ['clamp/mirror/clamp', 'clamp'])
  with pytest.raises(util.InputError, match='per dimension'):
    runtime.extend_host(a, (1, 1), (1, 1), 'constant', [(1, 2)])
  with pytest.raises(util.InputError, match='pair'):
    runtime.extend_host(a, (1, 1), (1, 1), 'constant', [(1, 2, 3), 0])
  assert not a.any()
  # the library itself: a one-sided wrap, a face mode it does not know
  lib = runtime.library()
  i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
  four = (ctypes.c_uint64 * 4)()
  for mlo, mhi in (((0, 1), (1, 1)), ((1, 1), (1, 0)), ((1, 1), (5, 1)),
                   ((-1, 1), (1, 1))):
    assert lib.soda_hip_extend_faces_host(
        a.ctypes.data, 4, 2, i32(4, 2), i32(1, 1), i32(1, 1), i32(*mlo),
        i32(*mhi), four) != 0
  assert not a.any()
  # the plan twins, names and raw numbers
  st = _stencil('jacobi2d.soda')
  plan = _plan(st, fuse=(4,))
  ok = lambda modes, **kw: runtime.border_plan(plan, (40, 7), modes, (1, 1),
                                               (1, 1), **kw)
  assert ok([('clamp', 'mirror'), 'constant'])[0]['padded'] == (44, 9)
  with pytest.raises(util.InputError, match='wraps on both'):
    ok([('wrap', 'mirror'), 'clamp'])
  with pytest.raises(util.BackendError, match='invalid.*wrap'):
    ok([(0, 2), 1])
  with pytest.raises(util.BackendError, match='invalid.*wrap'):
    ok([(2, 0), (1, 1)])
  with pytest.raises(util.BackendError, match='invalid.*face mode'):
    ok([(1, 5), 1])
  with pytest.raises(util.BackendError, match='invalid.*face mode'):
    ok([(1, -1), (1, 2)])
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    ok([('clamp', 'mirror'), 'wrap'], refill_every=2)
  with pytest.raises(util.InputError):
    ok([('clamp', 'mirror')])                    # one entry per dimension
  with pytest.raises(util.InputError):
    ok([(1, 2), (1, 2), (1, 2)])
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(
      st, [('clamp', 'mirror'), 'constant'], 4)
  fused = lambda modes, **kw: runtime.border_fused_plan(
      plan, (64, 48), modes, 4, rlo, rhi, lo, hi, **kw)
  assert fused([('clamp', 'mirror'), 'constant'])[0]['depth'] == 4
  with pytest.raises(util.BackendError, match='invalid.*wrap'):
    fused([(0, 2), 1])
  with pytest.raises(util.BackendError, match='invalid.*face mode'):
    runtime.border_fused_residual_boxes(plan, (64, 48), [(1, 7), 1], 4, rlo,
                                        rhi, lo, hi)
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    fused([('clamp', 'mirror'), 'clamp'], refill_every=2)
  with pytest.raises(util.InputError, match='wraps on both'):
    runtime.border_fused_ghosts(st, [('wrap', 'clamp'), 'clamp'], 2)
  # a batched plan: the batch twin serves it, the fused twin does not
  bplan = _plan(st, fuse=(4,), batch=True)
  info, _ = runtime.border_plan(bplan, (40, 7), [('clamp', 'mirror'), 'clamp'],
                                (1, 1), (1, 1), batch=3)
  assert info == runtime.border_plan(bplan, (40, 7), 'clamp', (1, 1), (1, 1),
                                     batch=3)[0]
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.border_fused_plan(bplan, (64, 48), [('clamp', 'mirror'), 'clamp'],
                              4, rlo, rhi, lo, hi)


# ---------------------------------------------------------------------------
# CPU: the plan twins
# ---------------------------------------------------------------------------

PLANS = [('jacobi2d.soda', dict(iterate=9), dict(fuse=(4,)), (40, 7), 9),
         ('heat3d.soda', dict(iterate=5), dict(fuse=(2,)), (32, 6, 5), 5)]


def _faces_of(dim, mode_hi):
  from soda_amd import runtime
  f = runtime.BorderFaces()
  for d in range(dim):
    f.mode_hi[d] = mode_hi[d]
  return f


@pytest.mark.parametrize('name,skw,okw,extent,iterate', PLANS,
                         ids=[p[0][:-5] for p in PLANS])
def test_plan_twins(built, name, skw, okw, extent, iterate):
  """With NULL or symmetric faces the twins return what the old entries
  return; an asymmetric request has the geometry of the symmetric one with
  the same wall dimensions."""
  from soda_amd import runtime
  st = _stencil(name, **skw)
  plan = _plan(st, **okw)
  dim = st.dim
  lib = runtime.library()
  lo, hi = runtime.border_ghosts(st, 'clamp')
  names = ['clamp', 'mirror', 'constant'][:dim]
  raw = runtime._border_modes(names, dim)
  old = runtime.border_plan(plan, extent, names, lo, hi, iterate)
  desc = runtime._border_desc(runtime._periodic_desc(
      dim, extent, 0, lo, hi, False), raw, ())

  def twin(faces_struct):
    info, n = runtime.PeriodicInfo(), ctypes.c_int32()
    chunks = (ctypes.c_int32 * iterate)()
    rc = lib.soda_hip_border_plan_faces(
        ctypes.byref(plan), ctypes.byref(desc),
        ctypes.byref(faces_struct) if faces_struct is not None else None,
        iterate, ctypes.byref(info), iterate, chunks, ctypes.byref(n))
    assert rc == 0, runtime.last_error()
    return runtime._periodic_info(info, dim), list(chunks[:n.value])
  assert twin(None) == old
  assert twin(_faces_of(dim, raw)) == old
  flipped = [[1, 2, 3, 4][(m + d) % 4] for d, m in enumerate(raw)]
  assert twin(_faces_of(dim, flipped)) == old
  asym = [('clamp', 'constant'), ('mirror', 'mirror101'),
          ('constant', 'clamp')][:dim]
  assert runtime.border_plan(plan, extent, asym, lo, hi, iterate) == old
  assert runtime.border_plan(plan, extent, [tuple(runtime._border_modes(
      p, 2)) for p in asym], lo, hi, iterate) == old
  # a wrapped dimension is a wrapped dimension
  if dim == 3:
    assert runtime.border_plan(plan, extent, asym[:2] + ['wrap'], lo, hi,
                               iterate) == runtime.border_plan(
                                   plan, extent, ('clamp', 'mirror', 'wrap'),
                                   lo, hi, iterate)
  # the fused twins
  depth = okw['fuse'][0]
  big = tuple(8 * n for n in extent)
  rlo, rhi, flo, fhi = runtime.border_fused_ghosts(st, names, depth)
  assert runtime.border_fused_ghosts(st, asym, depth) == (rlo, rhi, flo, fhi)
  args = (depth, rlo, rhi, flo, fhi)
  assert runtime.border_fused_plan(plan, big, asym, *args, iterate) == \
      runtime.border_fused_plan(plan, big, names, *args, iterate)
  assert runtime.border_fused_residual_boxes(plan, big, asym, *args) == \
      runtime.border_fused_residual_boxes(plan, big, names, *args)
  assert runtime.border_fused_plan(plan, big, names, *args)[0]['depth'] == depth


def test_abi_and_structs(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == 9
  assert lib.soda_hip_sizeof(17) == ctypes.sizeof(runtime.BorderDesc) == 208
  assert lib.soda_hip_sizeof(22) == ctypes.sizeof(runtime.BorderFaces) == 1056
  for name in ('soda_hip_extend_faces_host', 'soda_hip_border_plan_faces',
               'soda_hip_border_plan_batch_faces',
               'soda_hip_border_create_faces',
               'soda_hip_border_create_batch_faces',
               'soda_hip_border_fused_plan_faces',
               'soda_hip_border_fused_create_faces',
               'soda_hip_border_fused_residual_boxes_faces'):
    assert name in runtime.API and hasattr(lib, name), name


# ---------------------------------------------------------------------------
# CPU: the kernels, and what stays untouched
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('batch', [False, True], ids=['plain', 'bt'])
@pytest.mark.parametrize('dim', (1, 2, 3, 4))
def test_the_kernels_compile_without_scratch(built, dim, batch):
  """The faces module of every cell size and dimension count, for gfx950: one
  kernel, no scratch, no LDS, at most 64 VGPRs, plain C++."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import faces as gen
  for elem in sorted(SIZES):
    _, res = runtime.faces_resources(elem, dim, batch)
    name = gen.kernel_name(elem, dim, batch)
    assert sorted(res) == [name]
    assert res[name]['scratch'] == 0, res[name]
    assert res[name]['lds'] == 0 and 0 < res[name]['vgpr'] <= 64, res[name]
    text = gen.source(elem, dim, batch)
    assert 'asm' not in text.split('soda_rt_faces.h', 1)[1]
  assert 'asm' not in gen.faces_runtime_text()
  with pytest.raises(util.SemanticError):
    gen.source(3, 2)
  with pytest.raises(util.SemanticError):
    gen.source(4, 5)


def test_existing_modules_are_untouched():
  """The wrap and extend modules and the programs' modules are what they were:
  none mentions the faces module, no LowerOptions field was added."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import extend, faces as gen, lower, wrap
  for elem in sorted(SIZES):
    for dim in (1, 2, 3, 4):
      for batch in (False, True):
        gen.source(elem, dim, batch)
        for text in (wrap.source(elem, dim, batch),
                     extend.source(elem, dim, batch)):
          assert 'soda_faces' not in text and 'SODA_FACES' not in text and \
              'soda_rt_faces' not in text and 'faces_args' not in text
  assert extend.MODES == dict(wrap=0, clamp=1, mirror=2, mirror101=3,
                              constant=4)
  asym = [('clamp', 'constant'), 'mirror', ('mirror101', 'clamp')]
  for name, skw, okw in [('jacobi2d.soda', dict(iterate=13), dict(fuse=(4,))),
                         ('heat3d.soda', dict(iterate=4), dict(fuse=(2,))),
                         ('blur.soda', {}, {})]:
    stencil = _stencil(name, **skw)
    opts = runtime.resolve_options(stencil, _opts(**okw), None, probe=False)
    before = lower.lower(stencil, opts)
    plan = runtime.make_plan(before)
    lo, hi = runtime.border_ghosts(stencil, asym[:stencil.dim])
    runtime.border_plan(plan, (64,) * stencil.dim, asym[:stencil.dim], lo, hi)
    after = lower.lower(stencil, opts)
    assert before.source == after.source
    assert 'soda_faces' not in after.source and \
        'SODA_FACES' not in after.source
    assert bytes(plan) == bytes(runtime.make_plan(after))
  assert not any('border' in f or 'face' in f
                 for f in lower.LowerOptions.__dataclass_fields__)


def test_host_twin_under_a_sanitizer(built, tmp_path):
  """tests/host/faces_main.cpp + soda_extend.cpp as one program with its own
  main, -fsanitize=address,undefined: nothing loaded into Python."""
  exe = os.path.join(str(tmp_path), 'faces_main')
  subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
                  '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined',
                  '-I', os.path.join(ROOT, 'include'),
                  os.path.join(ROOT, 'tests', 'host', 'faces_main.cpp'),
                  os.path.join(ROOT, 'soda_amd', 'csrc', 'soda_extend.cpp'),
                  '-o', exe], check=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
  assert run.returncode == 0 and run.stdout.startswith('OK'), (
      run.stdout + run.stderr)


def test_command_line_has_the_faces():
  from soda_amd.codegen.hip import core as cli
  assert cli.parse_border('constant/clamp,mirror', 2) == [
      ('constant', 'clamp'), 'mirror']
  assert cli.parse_border('clamp', 2) == 'clamp'
  assert cli.parse_border_values('100/0,0', 2) == [(100.0, 0.0), 0.0]
  assert cli.parse_border_values('-1.5', 2) == [-1.5, -1.5]
  run = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', '--help'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode == 0 and '--hip-border-values' in run.stdout
  run = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', '--hip-backend',
       '--hip-border', 'constant/clamp,mirror', '--hip-border-values',
       '100/0,0', '--hip-extent', '64', '8', '--hip-until', '1e-3',
       soda_path('jacobi2d.soda')],
      capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode != 0 and '--hip-border runs on one GPU' in (
      run.stdout + run.stderr), (run.stdout, run.stderr)
  # one way to give the constants at a time
  run = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', '--hip-backend',
       '--hip-border', 'constant', '--hip-extent', '64', '8',
       '--hip-border-value', '2.5', '--hip-border-values', '100/0,0',
       soda_path('jacobi2d.soda')],
      capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode != 0 and 'not both' in (run.stdout + run.stderr), (
      run.stdout, run.stderr)


def test_constants_no_face_shows_do_not_make_a_request_asymmetric(built):
  """Only a `constant` face shows its constant: per-face constants that
  differ on other faces alone leave the request the old one."""
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda')
  bits = lambda v: runtime._cell_bits(v, 'float32')
  low, fstruct, flat = runtime._border_request(st, ['constant', 'clamp'],
                                               [(5, 5), (1, 2)])
  assert fstruct is None and flat == [bits(5)] and low == [4, 1]
  low, fstruct, flat = runtime._border_request(st, 'wrap', [(5, 6), (1, 2)])
  assert fstruct is None
  low, fstruct, flat = runtime._border_request(
      st, [('clamp', 'constant'), 'mirror'], [(9, 5), 7])
  assert fstruct is not None and flat == [bits(5)]        # the pair differs
  assert runtime._border_request(st, ['constant', 'clamp'],
                                 [(5, 6), 0])[1] is not None
  # the host twin agrees that they never show
  dom = np.arange(6, dtype=np.float32).reshape(2, 3)
  a = runtime.extend_host(_planted(dom, (1, 1), (1, 1)), (1, 1), (1, 1),
                          ['constant', 'clamp'], [(5, 5), (1, 2)])
  _same(a, borders.pad(dom, (1, 1), (1, 1), ['constant', 'clamp'], 5), 'host')


def test_the_ab_tool_compiles(built):
  """tools/faces_ab.py --compile-only: every case lowered and built for
  gfx950, no GPU."""
  run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools',
                                                     'faces_ab.py'),
                        '--compile-only'],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
  assert run.returncode == 0, run.stdout + run.stderr
  import json
  out = json.loads(run.stdout)
  assert [c['depth'] for c in out['cases']] == [1, 13, 1]
  for case in out['cases']:
    regs = case['registers']
    assert any(k.startswith('soda_faces_e4') for k in regs) and \
        any(k.startswith('soda_extend_e4') for k in regs)
    assert all(r['scratch'] == 0 and r['lds'] == 0 for r in regs.values())


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ct(t):
  return lambda: celltypes.stencil_of(t, 2, 'main', 5)


# program name -> (stencil, LowerOptions keywords)
PROGRAMS = {
    'jacobi2d': (lambda: _stencil('jacobi2d.soda', iterate=9),
                 dict(fuse=(4,), residual=True)),
    'jacobi2d_bt': (lambda: _stencil('jacobi2d.soda', iterate=5),
                    dict(fuse=(2,), batch=True)),
    'seidel2d': (lambda: _stencil('seidel2d.soda'), {}),
    'coupled2d': (lambda: _stencil('coupled2d.soda'), dict(fuse=(2,))),
    'blur': (lambda: _stencil('blur.soda'), {}),
    'blur_bt': (lambda: _stencil('blur.soda'), dict(batch=True)),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=5), dict(fuse=(2,))),
    'heat4d': (lambda: _stencil('heat4d.soda', iterate=2),
               dict(strategy='direct')),
    'double': (_ct('double'), dict(fuse=(4,), chunk_rows=16)),
    'uint8': (_ct('uint8'), dict(fuse=(4,), chunk_rows=16)),
}
PLATE = [('constant', 'constant'), 'clamp']
PLATE_CST = {'t1': [(100.0, 0.0), 0.0]}
_PROGRAMS = {}


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


def _framed(prog, extent, modes, constants, lo, hi):
  """A bordered handle with a frame of the test's choosing."""
  from soda_amd import runtime

  class Framed(runtime.Bordered):
    def __init__(self):
      st = prog.stencil
      not_iterable = self._begin(prog, extent, modes)
      low, fstruct, flat = runtime._border_request(st, modes, constants)
      desc = runtime._border_desc(runtime._periodic_desc(
          st.dim, self.extent, 1, lo, hi, False, not_iterable), low, flat)
      self._create(desc, [runtime.extend_resources], 'a framed domain',
                   fstruct)
  return Framed()


def _fill_case(prog, bor, modes, cst, leads=(0, 3)):
  """A planted pattern between guard bands: the interior keeps every byte,
  every ghost cell takes what the host twin and the closed form give."""
  from soda_amd import runtime
  dtype = np.dtype(prog.stencil.output_types[0].np_name)
  info = bor.info()
  lo, hi = info['ghost_lo'], info['ghost_hi']
  shape = info['padded'][::-1]
  cells = int(np.prod(shape))
  rng = np.random.default_rng(11)
  with periodic.Device(prog) as dev:
    for lead in leads:                           # cells behind a 16-byte line
      raw = rng.integers(0, 256, size=(lead + cells + 5) * dtype.itemsize,
                         dtype=np.uint8)
      base = dev.upload(raw)
      bor.fill([base + lead * dtype.itemsize])
      back = dev.download(base, raw.shape, np.uint8)
      view = lambda b: b[lead * dtype.itemsize:(lead + cells) *
                         dtype.itemsize].view(dtype).reshape(shape)
      before, after = view(raw), view(back)
      inner = periodic.interior(before, info)
      _same(periodic.interior(after, info), inner, 'interior')
      _same(after, faces.pad(inner, lo, hi, modes, cst), modes)
      twin = np.array(before, copy=True)
      runtime.extend_host(twin, lo, hi, modes, cst)
      _same(after, twin, 'host twin')
      n = lead * dtype.itemsize
      assert (back[:n] == raw[:n]).all()
      assert (back[-5 * dtype.itemsize:] == raw[-5 * dtype.itemsize:]).all()


_CST2 = [(1.5, -2.5), (3.25, -4.75)]


@pytest.mark.gpu
@pytest.mark.parametrize('where', [0, 1])
@pytest.mark.parametrize('frame', [((1, 1), (1, 1)), ((3, 2), (3, 2))], ids=str)
def test_fill_on_every_pair(programs, where, frame):
  """Each of the 16 pairs in dimension 0 (row ends and x-ghosts) and in
  dimension 1 (whole rows) of a 40 x 7 domain."""
  prog = programs('jacobi2d')
  other = ('constant', 'mirror')
  for pair in faces.PAIRS[:16]:
    modes = [pair, other] if where == 0 else [other, pair]
    with _framed(prog, (40, 7), modes, _CST2, *frame) as bor:
      _fill_case(prog, bor, modes, _CST2, leads=(1,))


@pytest.mark.gpu
def test_fill_on_a_frame_wider_than_the_domain(programs):
  prog = programs('jacobi2d')
  for modes in ([('mirror', 'mirror101'), ('constant', 'mirror')],
                [('mirror101', 'clamp'), ('mirror', 'constant')],
                [('constant', 'mirror'), ('clamp', 'mirror101')]):
    with _framed(prog, (3, 5), modes, _CST2, (4, 6), (7, 2)) as bor:
      _fill_case(prog, bor, modes, _CST2)


@pytest.mark.gpu
@pytest.mark.parametrize('name,extent,modes,cst', [
    ('uint8', (48, 5), [('constant', 'clamp'), ('mirror', 'constant')],
     [(77, 78), (79, 80)]),
    ('blur', (64, 8), [('mirror101', 'constant'), ('constant', 'mirror')],
     [(7, 8), (9, 10)]),
    ('double', (24, 5), [('clamp', 'constant'), ('constant', 'mirror101')],
     [(1.5, 2.5), (3.5, 4.5)]),
    ('heat3d', (32, 6, 5),
     [('constant', 'mirror'), 'wrap', ('clamp', 'constant')],
     [(1.0, 2.0), 0.0, (5.0, 6.0)]),
    ('heat4d', (5, 3, 2, 2),
     [('mirror', 'constant'), ('constant', 'clamp'), 'mirror101/mirror',
      ('constant', 'constant')], [(1.0, 2.0), (3.0, 4.0), 0.0, (7.0, 8.0)]),
], ids=['uint8', 'uint16', 'double', '3d', '4d'])
def test_fill_on_other_cells_and_dimensions(programs, name, extent, modes, cst):
  prog = programs(name)
  with prog.bordered(extent, modes, cst) as bor:
    _fill_case(prog, bor, modes, cst)


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


class _DenseEntry:
  """The dense entry with run_device's call shape, for tests/guarded.py."""

  def __init__(self, prog, bor):
    self.device, self.bor = prog.device, bor

  def run_device(self, outputs, inputs, extent, iterate=None, **kw):
    self.bor.run_device(outputs, inputs, iterate, **kw)


# case -> (program, extent, iterate, modes, constants)
CASES = {
    'jacobi2d': ('jacobi2d', (40, 7), 9,
                 [('constant', 'mirror'), ('clamp', 'constant')],
                 [(2.0, 0.0), (0.0, -3.5)]),
    'corners': ('seidel2d', (40, 7), 2, 'constant',
                [(1.0, 2.0), (3.0, 4.0)]),
    'coupled2d': ('coupled2d', (32, 9), 3,
                  [('constant', 'clamp'), ('mirror', 'constant')],
                  {'a': [(1.5, 2.5), 3.5], 'b': [-2.0, (4.0, -6.0)]}),
    'blur': ('blur', (64, 8), 1,
             [('mirror101', 'constant'), ('constant', 'clamp')],
             [(7, 201), (9, 65535)]),
    'heat3d': ('heat3d', (32, 6, 5), 5,
               [('constant', 'mirror'), 'wrap', ('clamp', 'mirror101')],
               [(1.0, 2.0), 0.0, 0.0]),
}
_EXPECTED = {}


def _case(name, seed=0):
  key = (name, seed)
  if key not in _EXPECTED:
    pname, extent, iterate, modes, cst = CASES[name]
    stencil = PROGRAMS[pname][0]()
    ins = periodic.inputs(stencil, extent, seed)
    _EXPECTED[key] = (pname, stencil, extent, iterate, modes, cst, ins,
                      faces.expected(stencil, ins, iterate, modes, cst))
  return _EXPECTED[key]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_dense_entry_between_guard_bands(programs, name):
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  prog = programs(pname)
  with prog.bordered(extent, modes, cst) as bor:
    assert bor.info()['refill_every'] == 1
    got, violation, _ = guarded.run(_DenseEntry(prog, bor), stencil, extent,
                                    ins, iterate)
  assert violation is None, violation
  _assert_same(got, want, name)
  if name in ('jacobi2d', 'coupled2d'):          # numpy in, numpy out
    _assert_same(prog.run_bordered(ins, modes, cst, iterate), want,
                 'run_bordered')


@pytest.mark.gpu
def test_padded_entry_across_calls(programs):
  """Two run_padded calls of 3 and 4 iterations equal one dense run of 7; the
  state stays extended in between; the inputs keep their bytes."""
  _, stencil, extent, _, modes, cst, ins, _ = _case('jacobi2d')
  prog = programs('jacobi2d')
  want = faces.expected(stencil, ins, 7, modes, cst)
  with prog.bordered(extent, modes, cst) as bor, periodic.Device(prog) as dev:
    info = bor.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    start = faces.pad(ins['t1'], lo, hi, modes, cst)
    assert start.shape == info['padded'][::-1]
    d0, d1, d2 = dev.upload(start), dev.alloc(start.nbytes), \
        dev.alloc(start.nbytes)
    bor.run_padded([d1], [d0], 3)
    bor.run_padded([d2], [d1], 4)
    after3 = dev.download(d1, start.shape, start.dtype)
    after7 = dev.download(d2, start.shape, start.dtype)
    _same(dev.download(d0, start.shape, start.dtype), start, 'inputs')
  _assert_same({'t0': periodic.interior(after7, info)}, want, 'padded 3 + 4')
  _assert_same({'t0': periodic.interior(after3, info)},
               faces.expected(stencil, ins, 3, modes, cst), 'padded 3')
  for arr in (after3, after7):                   # extended: ghosts current
    _same(arr, faces.pad(periodic.interior(arr, info), lo, hi, modes, cst),
          'extended')


FUSED_J = ([('constant', 'mirror'), ('clamp', 'constant')],
           [(2.0, -1.0), (0.0, -3.5)])
FUSED_H = ([('constant', 'mirror'), ('mirror101', 'clamp'),
            ('clamp', 'constant')], [(1.0, 2.0), 0.0, (0.0, -1.0)])


@pytest.mark.gpu
def test_fused_jacobi2d(programs):
  """128 x 64 x 30 at depths 1, 2, 4, 13 and 0: the bits of depth 1 and of the
  oracle."""
  prog = programs('jacobi2d')
  st = prog.stencil
  modes, cst = FUSED_J
  ins = periodic.inputs(st, (128, 64), 2)
  want = faces.expected(st, ins, 30, modes, cst)
  for depth in (1, 2, 4, 13, 0):
    with prog.bordered((128, 64), modes, cst, depth=depth) as bor:
      info = bor.info()
      got = _dense(prog, bor, ins, 30)
    _assert_same(got, want, 'depth %d' % depth)
    if depth != 1:
      assert info['depth'] == (depth or 4)
      assert [s['dim'] for s in info['strips']] == [0, 1]


@pytest.mark.gpu
def test_fused_heat3d(programs):
  prog = programs('heat3d')
  st = prog.stencil
  modes, cst = FUSED_H
  ins = periodic.inputs(st, (32, 24, 20), 2)
  want = faces.expected(st, ins, 6, modes, cst)
  for depth in (1, 2):
    with prog.bordered((32, 24, 20), modes, cst, depth=depth) as bor:
      got = _dense(prog, bor, ins, 6)
      if depth == 2:
        assert bor.info()['depth'] == 2 and len(bor.info()['strips']) == 3
    _assert_same(got, want, 'depth %d' % depth)


@pytest.mark.gpu
@pytest.mark.parametrize('pname,extent,iterate,modes,cst', [
    ('jacobi2d_bt', (40, 7), 5, CASES['jacobi2d'][3], CASES['jacobi2d'][4]),
    ('blur_bt', (64, 8), 1, CASES['blur'][3], CASES['blur'][4]),
], ids=['jacobi2d', 'blur'])
def test_batch(programs, pname, extent, iterate, modes, cst):
  """3 items: per item the expected bits of the unbatched domain; residual,
  norms and until on the batched handle stay refused, no byte written."""
  from soda_amd import util
  prog = programs(pname)
  st = prog.stencil
  items = [periodic.inputs(st, extent, seed) for seed in (0, 1, 2)]
  name, out = st.input_names[0], st.output_names[0]
  stacked = {name: np.stack([i[name] for i in items])}
  got = prog.run_bordered_batch(stacked, modes, cst, iterate)
  for k, ins in enumerate(items):
    _assert_same({out: got[out][k]},
                 faces.expected(st, ins, iterate, modes, cst), 'item %d' % k)
  with prog.bordered(extent, modes, cst, batch=3) as bor, \
      periodic.Device(prog) as dev:
    info = bor.info()
    cells = 3 * int(np.prod(info['padded']))
    dtype = np.dtype(st.output_types[0].np_name)
    planted = np.full(cells, 0x5A, dtype)
    d_in, d_out = dev.upload(planted), dev.upload(planted)
    word = dev.upload(np.full(840, 0xA5, np.uint8))
    before = prog.last_launches(), prog.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      bor.run_padded([d_out], [d_in], 1, residual=word)
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      bor.run_until([d_out], [d_in], 0.5, 4)
    if pname == 'jacobi2d_bt':
      with pytest.raises(util.BackendError, match='unsupported.*batched'):
        bor.run_padded([d_out], [d_in], 1, norms=word)
    assert (prog.last_launches(), prog.scratch()) == before
    _same(dev.download(d_out, planted.shape, dtype), planted, 'outputs')
    assert (dev.download(word, (840,), np.uint8) == 0xA5).all()


def _cpu_until(st, ins, tol, max_iterate, check_every, norm):
  """(iterations done, cur, prev) of the CPU loop on the plate under the
  library's stop rule."""
  done, state = 0, {0: {'t0': ins['t1']}}
  while done < max_iterate:
    for _ in range(min(check_every, max_iterate - done)):
      state[done + 1] = faces.expected(st, {'t1': state[done]['t0']}, 1, PLATE,
                                       PLATE_CST)
      done += 1
    cur, prev = state[done], state[done - 1]
    if norm is None:
      res = domains.residual_of(st, cur, prev)
      stop = res[1] == 0 and res[2] <= tol and res[3] <= 0
    else:
      want = domains.norms_of(st, cur, prev)
      value = norms.expected_value(want, norm) ** 0.5
      stop = not want['unordered'] and not want['infinite'] and value <= tol
    if stop:
      break
  return done, cur, prev


@pytest.mark.gpu
@pytest.mark.parametrize('norm,tol', [(None, 0.25), ('l2', 2.0)], ids=str)
@pytest.mark.parametrize('depth', [1, 0])
def test_convergence_on_the_plate(programs, depth, norm, tol):
  """jacobi2d 32 x 16, a hot and a cold `constant` wall in dimension 0, `clamp`
  in dimension 1: iterations done, every field of the residual, every word of
  the L2 norms and the output bits equal the CPU loop's."""
  prog = programs('jacobi2d')
  st = prog.stencil
  ins = {'t1': np.zeros((16, 32), np.float32)}
  done, cur, prev = _cpu_until(st, ins, tol, 200, 4, norm)
  assert 4 < done < 200, done
  outs, got_done, last = prog.run_bordered_until(
      ins, PLATE, tol, 200, constants=PLATE_CST, depth=depth, check_every=4,
      norm=norm)
  assert got_done == done
  if norm is None:
    assert domains.fields(last) == domains.residual_of(st, cur, prev)
  else:
    assert norms.same(last, domains.norms_of(st, cur, prev))
  _same(outs['t0'], cur['t0'], 'plate')
  # hot on the left, cold on the right, no gradient across the insulated walls
  assert outs['t0'][:, 0].min() > outs['t0'][:, -1].max()


@pytest.mark.gpu
def test_a_symmetric_request_is_the_old_handle(programs, monkeypatch):
  """Equal pairs and equal constants: the old entries, the extend kernels --
  the faces module is never built --, the same scratch, the same bits."""
  from soda_amd import runtime
  prog = programs('jacobi2d')
  st = prog.stencil
  extent, ins = (40, 7), periodic.inputs(st, (40, 7), 3)

  def never(*a, **kw):
    raise AssertionError('a symmetric request built the faces module')
  with prog.bordered(extent, ('mirror', 'constant'), -3.5) as old:
    want, old_info = _dense(prog, old, ins, 9), old.info()
    launches, scratch = prog.last_launches(), prog.scratch()
  monkeypatch.setattr(runtime, 'faces_resources', never)
  for modes, cst in (
      ([('mirror', 'mirror'), 'constant/constant'], [-3.5, (-3.5, -3.5)]),
      (['mirror/mirror', ('constant', 'constant')], {'t1': [(-3.5, -3.5)] * 2}),
      # constants that differ where no face shows one
      (('mirror', 'constant'), [(1.0, 2.0), (-3.5, -3.5)])):
    with prog.bordered(extent, modes, cst) as bor:
      assert type(bor) is type(old) and bor.info() == old_info
      _assert_same(_dense(prog, bor, ins, 9), want, str(modes))
      assert (prog.last_launches(), prog.scratch()) == (launches, scratch)
  # the fused twin: the old fused handle, strip for strip
  big, bins = (64, 48), periodic.inputs(st, (64, 48), 3)
  with prog.bordered(big, ('mirror', 'constant'), -3.5, depth=2) as old2:
    want2, info2 = _dense(prog, old2, bins, 9), old2.info()
    after2 = prog.last_launches(), prog.scratch()
  assert info2['depth'] == 2 and len(info2['strips']) == 2
  with prog.bordered(big, [('mirror', 'mirror'), 'constant/constant'],
                     [(1.0, 2.0), (-3.5, -3.5)], depth=2) as bor:
    assert type(bor) is type(old2) and bor.info() == info2
    _assert_same(_dense(prog, bor, bins, 9), want2, 'fused')
    assert (prog.last_launches(), prog.scratch()) == after2
  scratch = prog.scratch()
  # the twin itself on a symmetric BorderFaces: the old entry's handle
  low, _, flat = runtime._border_request(st, ('mirror', 'constant'), -3.5)
  lo, hi = runtime.border_ghosts(st, 'mirror')
  desc = runtime._border_desc(runtime._periodic_desc(2, extent, 1, lo, hi,
                                                     False), low, flat)
  sym = _faces_of(2, low)
  codes, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
  code, _ = runtime.extend_resources(4, 2)
  buf = ctypes.create_string_buffer(code, len(code))
  codes[2], sizes[2] = ctypes.cast(buf, ctypes.c_void_p), len(code)
  handle = ctypes.c_void_p()
  lib = runtime.library()
  assert lib.soda_hip_border_create_faces(
      prog._handle, ctypes.byref(desc), ctypes.byref(sym), codes, sizes, None,
      None, ctypes.byref(handle)) == 0, runtime.last_error()
  raw = runtime.PeriodicInfo()
  assert lib.soda_hip_border_info(handle, ctypes.byref(raw)) == 0
  assert runtime._periodic_info(raw, 2) == old_info
  assert lib.soda_hip_border_destroy(handle) == 0
  # an asymmetric one needs the faces modules
  asym = _faces_of(2, [3, 4])
  assert lib.soda_hip_border_create_faces(
      prog._handle, ctypes.byref(desc), ctypes.byref(asym), codes, sizes, None,
      None, ctypes.byref(handle)) != 0 and not handle.value
  assert 'faces' in runtime.last_error()
  assert prog.scratch() == scratch
  # the fused twin on a symmetric BorderFaces whose constants differ only
  # where no face shows one: the old fused entry's handle, no faces module
  rlo, rhi, flo, fhi = runtime.border_fused_ghosts(st, ('mirror', 'constant'),
                                                   2)
  fdesc = runtime._border_fused_desc(runtime._border_desc(
      runtime._periodic_desc(2, big, 0, flo, fhi, False), low, flat), 2, rlo,
                                     rhi)
  sym.per_face_constants = 1
  for side in (0, 1):
    sym.constant[0][0][side] = 1 + side           # dimension 0 mirrors
    sym.constant[0][1][side] = flat[0]
  bcode, _ = runtime.box_resources(4, 2)
  bbuf = ctypes.create_string_buffer(bcode, len(bcode))
  bcodes, bsizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
  bcodes[2], bsizes[2] = ctypes.cast(bbuf, ctypes.c_void_p), len(bcode)
  assert lib.soda_hip_border_fused_create_faces(
      prog._handle, ctypes.byref(fdesc), ctypes.byref(sym), codes, sizes,
      bcodes, bsizes, None, None, ctypes.byref(handle)) == 0, \
      runtime.last_error()
  fraw = runtime.BorderFusedInfo()
  assert lib.soda_hip_border_fused_info(handle, ctypes.byref(fraw)) == 0
  assert runtime._border_fused_info(fraw, 2) == info2
  assert lib.soda_hip_border_fused_destroy(handle) == 0
  assert prog.scratch() == scratch


@pytest.mark.gpu
def test_refusals_launch_nothing_and_allocate_nothing(programs):
  from soda_amd import runtime, util
  prog = programs('jacobi2d')
  st = prog.stencil
  extent = (40, 7)
  with prog.bordered(extent, CASES['jacobi2d'][3], CASES['jacobi2d'][4]) as bor:
    _dense(prog, bor, periodic.inputs(st, extent), 2)
  before = prog.last_launches(), prog.scratch()
  with pytest.raises(util.InputError, match='wraps on both'):
    prog.bordered(extent, [('wrap', 'clamp'), 'clamp'])
  with pytest.raises(util.InputError, match='unknown mode'):
    prog.bordered(extent, [('clamp', 'edge'), 'clamp'])
  with pytest.raises(util.InputError, match='pair'):
    prog.bordered(extent, [('clamp', 'clamp', 'clamp'), 'clamp'])
  with pytest.raises(util.InputError, match='per dimension'):
    prog.bordered(extent, 'constant', [(1.0, 2.0)])
  with pytest.raises(util.InputError, match='no inputs'):
    prog.bordered(extent, 'constant', {'t9': [(1.0, 2.0), 0.0]})
  lo, hi = runtime.border_ghosts(st, 'clamp')
  lib = runtime.library()
  codes, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
  fcode, _ = runtime.faces_resources(4, 2)
  buf = ctypes.create_string_buffer(fcode, len(fcode))
  fcodes, fsizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
  fcodes[2], fsizes[2] = ctypes.cast(buf, ctypes.c_void_p), len(fcode)
  for low, high, k, what in (((0, 1), (1, 1), 1, 'wrap'),
                             ((1, 1), (1, 9), 1, 'face mode'),
                             ((1, 1), (2, 1), 2, 'refill')):
    desc = runtime._border_desc(runtime._periodic_desc(
        2, extent, k, lo, hi, False), low, (0,))
    fstruct = _faces_of(2, high)
    for create, more in (
        (lib.soda_hip_border_create_faces, ()),
        (lib.soda_hip_border_fused_create_faces, (codes, sizes))):
      handle = ctypes.c_void_p()
      d = desc
      if more:
        d = runtime._border_fused_desc(desc, 2, (1, 1), (1, 1))
      rc = create(prog._handle, ctypes.byref(d), ctypes.byref(fstruct), codes,
                  sizes, *more, fcodes, fsizes, ctypes.byref(handle))
      assert rc != 0 and not handle.value and what in runtime.last_error(), (
          what, runtime.last_error())
  assert (prog.last_launches(), prog.scratch()) == before
  assert prog._periodic == []


@pytest.mark.gpu
def test_dense_entry_captured_and_replayed(programs):
  import torch
  pname, stencil, extent, iterate, modes, cst, ins, want = _case('heat3d')
  ins2, want2 = _case('heat3d', seed=5)[6:]
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
    _assert_same({o_name: read()}, want, 'eager')
    warm, held = prog.scratch(), bor.info()['scratch_bytes']
    t_out.copy_(asyncrun._bytes(asyncrun.poison_like(want[o_name])))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
      call()
    assert np.isnan(read()).all()                 # capture records only
    t_in.copy_(asyncrun._bytes(ins2[i_name]))     # new inputs
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_same({o_name: read()}, want2, 'replay on new inputs')
    assert prog.scratch() == warm and bor.info()['scratch_bytes'] == held
    del g


# -- random programs ---------------------------------------------------------

FUZZ = [(s, f) for f in ('plain', 'rich', 'window') for s in (1, 2, 3, 5)]
_WALLS = faces.WALLS


def _fuzz_faces(seed, family, dim):
  """A pair per dimension from the seed; one dimension of a 2-D or 3-D program
  wraps on every third seed."""
  fi = ('plain', 'rich', 'window').index(family)
  modes = [(_WALLS[(seed + fi + d) % 4], _WALLS[(2 * seed + fi + 3 * d + 1) % 4])
           for d in range(dim)]
  if dim > 1 and seed % 3 == 2:
    modes[seed % dim] = ('wrap', 'wrap')
  return modes


def _nest_run(prog, ins, extent, modes, cst, iterate):
  """fuzz_nest.Program.run_bordered with tests/faces.py's extension: the
  one-iteration nest on inputs extended over pad_margin(), the domain cut
  out, outputs becoming inputs by position."""
  m = prog.pad_margin()
  big = tuple(n + 2 * w for n, w in zip(extent, m))
  one = fuzz_nest.Program(prog.name, prog.dim, 1, prog.inputs, prog.stmts)
  cut = tuple(slice(w, w + n) for w, n in zip(m[::-1], extent[::-1]))
  state = {n: np.ascontiguousarray(ins[n], dtype=fuzz_nest.NPTYPES[t])
           for n, t in prog.inputs}
  cur = None
  for it in range(iterate):
    padded = {n: faces.pad(state[n], m, m, modes, cst[n])
              for n, _ in prog.inputs}
    whole = one.run(padded, big)
    cur = {o: np.ascontiguousarray(a[cut]) for o, a in whole.items()}
    state = {n: cur[o.name] for (n, _), o in zip(prog.inputs, prog.outputs)} \
        if it + 1 < iterate else state
  return cur


def _fuzz_same(got, want, what, text):
  assert sorted(got) == sorted(want)
  for o in want:
    a, b = got[o], want[o]
    ok = a.dtype == b.dtype and a.shape == b.shape
    if ok and a.dtype.kind == 'f':
      bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
      eq = np.ascontiguousarray(a).view(bits) == \
          np.ascontiguousarray(b).view(bits)
      ok = bool((eq | (np.isnan(a) & np.isnan(b))).all())
    elif ok:
      ok = bool((a == b).all())
    assert ok, '%s, output %s differs\n%s' % (what, o, text)


@pytest.mark.gpu
@pytest.mark.parametrize('seed,family', FUZZ,
                         ids=['%s%d' % (f, s) for s, f in FUZZ])
def test_random_programs(built, seed, family):
  """A random program under random face pairs and constants, at depth 1 and
  fused, against the generator's own nest on inputs extended by
  tests/faces.py."""
  from soda_amd import core, runtime, util
  prog, _ = fuzz_nest.program(seed, family)
  text = prog.soda_text()
  st = core.from_text(text)
  dim = prog.dim
  modes = _fuzz_faces(seed, family, dim)
  cst = {n: [(3 + 2 * i + d, 4 + 2 * i + 3 * d) for d in range(dim)]
         for i, (n, _) in enumerate(prog.inputs)}
  extent = ((7, 12, 33)[seed % 3],) + tuple(4 + (seed + d) % 5
                                            for d in range(1, dim))
  ins = fuzz_nest.inputs_for(prog, extent, seed)
  iterate = prog.iterate
  want = _nest_run(prog, ins, extent, modes, cst, iterate)
  with runtime.Program(st, _opts(fuse=(2,))) as hip:
    _fuzz_same(hip.run_bordered(ins, modes, cst, iterate), want,
               'depth 1 %s %s' % (extent, modes), text)
    if prog.iterable() and iterate >= 2:
      deepest = max(p.fused_iters for p in hip.module.passes)
      if _fused_served(seed, family, deepest):
        got = hip.run_bordered(ins, modes, cst, iterate, depth=0)
        _fuzz_same(got, want, 'fused %s %s' % (extent, modes), text)
      else:                         # refused in its own words, and counted
        with pytest.raises(util.InputError, match='reach more than'):
          hip.run_bordered(ins, modes, cst, iterate, depth=0)


def _fused_served(seed, family, depth=2):
  """Whether border_fused_ghosts serves the program under its faces."""
  from soda_amd import core, runtime, util
  prog, _ = fuzz_nest.program(seed, family)
  if not (prog.iterable() and prog.iterate >= 2):
    return False
  try:
    runtime.border_fused_ghosts(core.from_text(prog.soda_text()),
                                _fuzz_faces(seed, family, prog.dim), depth)
  except util.InputError as e:
    assert 'reach more than' in str(e), str(e)
    return False
  return True


def test_the_random_programs_cover_the_fused_form():
  """A change of the generator cannot hollow the fused arm out: most of the
  dozen programs iterate and are served fused under their faces, some of them
  with a wrapped dimension, in more than one dimension count."""
  served = [(s, f) for s, f in FUZZ if _fused_served(s, f)]
  assert len(FUZZ) == 12 and len(served) >= 8, served
  dims = {fuzz_nest.program(s, f)[0].dim for s, f in served}
  assert len(dims) >= 2, dims
  for s, f in FUZZ:
    for pair in _fuzz_faces(s, f, fuzz_nest.program(s, f)[0].dim):
      assert pair == ('wrap', 'wrap') or 'wrap' not in pair
