"""Bordered domains fused away from the walls (soda_hip_border_fused_*,
soda_hip_box_host): the interior of a chunk runs fused on the
padded domain, a narrow strip per wall dimension mends the rim.

Every comparison is on bit patterns.  The expected value is that of
tests/borders.py -- np.pad and the oracle, iteration by iteration -- and never
uses the code under test.

CPU: box_host against numpy slicing; the same under a sanitizer in a program
of its own; the plan; THE SCHEME ITSELF emulated with the numpy oracle from the
plan's numbers alone (tests/rims.py); the box modules compiled for gfx950; what
the feature leaves untouched; refusals.
GPU: parity with borders.expected and with the depth-1 handle per mode,
program, depth and extent; the padded entry across calls; guard bands; planted
bytes around arrays aligned to the cell only; a live stream; a captured graph;
refusals."""
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
import rims

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
  raw = rng.integers(0, 256, size=tuple(extent[::-1]) + (size,), dtype=np.uint8)
  return np.ascontiguousarray(raw).view(SIZES[size]).reshape(extent[::-1])


def _slices(origin, size):
  return tuple(slice(o, o + n) for o, n in zip(origin[::-1], size[::-1]))


# ---------------------------------------------------------------------------
# CPU: the host twin of the box mover
# ---------------------------------------------------------------------------

BOX_CASES = [
    # (dst extent, src extent, [(dst origin, src origin, size)]), dim 0 first
    ((23,), (31,), [((0,), (0,), (23,))]),
    ((23,), (31,), [((1,), (3,), (7,)), ((9,), (20,), (11,))]),
    ((23,), (31,), [((5,), (5,), (0,))]),                      # empty
    ((19, 6), (25, 9), [((0, 0), (0, 0), (19, 6))]),
    ((19, 6), (25, 9), [((1, 0), (2, 3), (5, 6)), ((6, 0), (19, 3), (6, 6))]),
    ((19, 6), (25, 9), [((3, 1), (1, 1), (13, 0)), ((0, 5), (24, 8), (1, 1))]),
    ((9, 5, 4), (7, 8, 4), [((1, 1, 0), (0, 2, 1), (6, 3, 3)),
                            ((0, 0, 3), (3, 0, 0), (4, 5, 1))]),
    ((9, 5, 4), (7, 8, 4), [((2, 0, 0), (0, 0, 0), (3, 0, 4)),   # empty
                            ((8, 4, 3), (6, 7, 3), (1, 1, 1))]),
    ((6, 4, 3, 3), (5, 5, 4, 2), [((1, 0, 1, 0), (0, 1, 0, 0), (5, 3, 2, 2)),
                                  ((0, 3, 0, 2), (2, 4, 3, 1), (3, 1, 1, 1))]),
    # the two parts of a gather and of a scatter, as the handle cuts them
    ((18, 7), (42, 7), [((1, 1), (1, 1), (8, 5)), ((9, 1), (33, 1), (8, 5))]),
    ((42, 7), (18, 7), [((1, 1), (1, 1), (3, 5)), ((38, 1), (14, 1), (3, 5))]),
]


@pytest.mark.parametrize('size', sorted(SIZES))
@pytest.mark.parametrize('case', BOX_CASES, ids=lambda c: 'x'.join(
    map(str, c[0])) + '_' + str(len(c[2])))
def test_box_host_is_numpy_slicing(built, size, case):
  from soda_amd import runtime
  dext, sext, boxes = case
  rng = np.random.default_rng(size + len(dext))
  src = _cells(rng, sext, size)
  dst = _cells(rng, dext, size)
  want = dst.copy()
  for to, frm, n in boxes:
    want[_slices(to, n)] = src[_slices(frm, n)]
  before = src.copy()
  assert runtime.box_host(dst, src, boxes) is dst
  assert periodic.same_bits(dst, want), periodic.differing(dst, want)
  assert periodic.same_bits(src, before)


def test_box_host_at_addresses_aligned_to_the_cell_only(built):
  """The arrays start 1, 2 and 3 cells behind a 16-byte line."""
  from soda_amd import runtime
  for size in sorted(SIZES):
    for lead_d, lead_s in ((1, 0), (0, 3), (2, 1), (3, 3)):
      rng = np.random.default_rng(size)
      raw_s = _cells(rng, (lead_s + 25 * 9,), size)
      raw_d = _cells(rng, (lead_d + 19 * 6 + 2,), size)
      kept = raw_d.copy()
      src = raw_s[lead_s:].reshape(9, 25)
      dst = raw_d[lead_d:lead_d + 19 * 6].reshape(6, 19)
      want = dst.copy()
      want[0:6, 1:6] = src[3:9, 2:7]
      want[1:5, 6:19] = src[0:4, 12:25]
      runtime.box_host(dst, src, [((1, 0), (2, 3), (5, 6)),
                                  ((6, 1), (12, 0), (13, 4))])
      assert periodic.same_bits(dst, want)
      assert (raw_d[:lead_d] == kept[:lead_d]).all() and \
          (raw_d[-2:] == kept[-2:]).all()


def test_box_host_refusals(built):
  from soda_amd import runtime, util
  src = np.arange(24, dtype=np.float32).reshape(4, 6)
  dst = np.zeros((3, 5), np.float32)
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.box_host(dst, src, [((0, 0), (0, 0), (6, 3))])     # leaves dst
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.box_host(dst, src, [((0, 0), (2, 0), (5, 3))])     # leaves src
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.box_host(dst, src, [((-1, 0), (0, 0), (2, 2))])
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.box_host(dst, src, [((0, 0), (0, 0), (2, -2))])
  with pytest.raises(util.InputError):
    runtime.box_host(dst, src, [((0,), (0, 0), (2, 2))])
  with pytest.raises(util.InputError):
    runtime.box_host(dst, src.astype(np.float64), [])
  with pytest.raises(util.InputError):
    runtime.box_host(dst, src[:, ::2], [])
  with pytest.raises(util.InputError, match='overlap'):
    runtime.box_host(src[:2], src[1:], [])
  assert not dst.any()
  # a good box after a bad one: nothing is written
  with pytest.raises(util.BackendError):
    runtime.box_host(dst, src, [((0, 0), (0, 0), (2, 2)),
                                ((4, 2), (0, 0), (2, 2))])
  assert not dst.any()


def test_host_twin_under_a_sanitizer(built, tmp_path):
  """tests/host/box_main.cpp + soda_box.cpp as one program with its own main,
  -fsanitize=address,undefined: nothing loaded into Python."""
  exe = os.path.join(str(tmp_path), 'box_main')
  subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fno-omit-frame-pointer',
                  '-fsanitize=address,undefined',
                  '-fno-sanitize-recover=undefined',
                  '-I', os.path.join(ROOT, 'include'),
                  os.path.join(ROOT, 'tests', 'host', 'box_main.cpp'),
                  os.path.join(ROOT, 'soda_amd', 'csrc', 'soda_box.cpp'),
                  '-o', exe], check=True)
  run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert run.returncode == 0 and run.stdout.startswith('OK'), (
      run.stdout + run.stderr)


# ---------------------------------------------------------------------------
# CPU: the plan
# ---------------------------------------------------------------------------

DEPTH = 4
# name, stencil keywords, LowerOptions keywords, modes, constants, the reach
# of one iteration (lo, hi) restated by hand
GEOMETRY = {
    'jacobi2d': ('jacobi2d.soda', dict(iterate=9), dict(fuse=(4,)), 'clamp',
                 None, ([1, 1], [1, 1])),
    'blur': ('blur.soda', dict(iterate=9), {}, 'mirror101', None,
             ([0, 0], [2, 2])),                                 # one-sided
    'skew2d': ('skew2d.soda', dict(iterate=9), {}, ('constant', 'mirror101'),
               2.0, ([2, 2], [2, 2])),
    'coupled2d': ('coupled2d.soda', dict(iterate=9), dict(fuse=(2,)),
                  'constant', {'a': 1.5, 'b': -2.0}, None),
    'heat3d': ('heat3d.soda', dict(iterate=9), dict(fuse=(2,)),
               ('mirror', 'clamp', 'wrap'), None, ([1, 1, 1], [1, 1, 1])),
}


def _geometry(name, depth=DEPTH):
  """(stencil, plan, modes, constants, reach_lo, reach_hi, ghost_lo,
  ghost_hi)."""
  from soda_amd import runtime
  fname, skw, okw, modes, cst, reach = GEOMETRY[name]
  st = _stencil(fname, **skw)
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, modes, depth)
  assert (rlo, rhi) == (reach or tuple(periodic.reach(st, 1)))
  return st, _plan(st, **okw), modes, cst, rlo, rhi, lo, hi


def _smallest(st, modes, rlo, rhi, depth=DEPTH, roomy=24):
  """N[d] = L + H in every wall dimension that has a strip, `roomy`
  elsewhere."""
  raw = borders.per_dim(modes, st.dim)
  return tuple(2 * depth * (rlo[d] + rhi[d])
               if raw[d] != 'wrap' and rlo[d] + rhi[d] else roomy
               for d in range(st.dim))


@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_plan_strips_and_chunks(built, name):
  from soda_amd import runtime
  st, plan, modes, _, rlo, rhi, lo, hi = _geometry(name)
  raw = borders.per_dim(modes, st.dim)
  # the frame: one iteration's reach at a wall, DEPTH times that where it wraps
  assert lo == [r * (DEPTH if m == 'wrap' else 1) for r, m in zip(rlo, raw)]
  assert hi == [r * (DEPTH if m == 'wrap' else 1) for r, m in zip(rhi, raw)]
  vec = max(1, max(q.vec for q in plan.kernels[:plan.num_kernels]))
  per_cell = sum(plan.elem_size[i] for i in range(plan.num_inputs)) + \
      2 * sum(plan.elem_size[plan.num_inputs + o]
              for o in range(plan.num_outputs))
  small = _smallest(st, modes, rlo, rhi)
  for extent in (tuple(n + 7 + d for d, n in enumerate(small)), small):
    info, chunks = runtime.border_fused_plan(plan, extent, modes, DEPTH, rlo,
                                             rhi, lo, hi, 9)
    assert info['depth'] == DEPTH and chunks == [4, 4, 1]
    assert info['refill_every'] == 1
    main, _ = runtime.border_plan(plan, extent, modes, lo, hi, 9)
    for key in ('ghost_lo', 'ghost_hi', 'padded'):
      assert info[key] == main[key]
    walls = [d for d in range(st.dim)
             if raw[d] != 'wrap' and rlo[d] + rhi[d]]
    assert [s['dim'] for s in info['strips']] == walls      # none for a wrap
    total = main['scratch_bytes']
    for s in info['strips']:
      d = s['dim']
      assert s['lo'] == s['hi'] == DEPTH * (rlo[d] + rhi[d])
      assert (s['take_lo'], s['take_hi']) == ((DEPTH - 1) * rlo[d],
                                              (DEPTH - 1) * rhi[d])
      want = list(extent)
      want[d] = s['lo'] + s['hi']
      assert s['extent'] == tuple(want) and want[d] <= extent[d]
      assert s['ghost_lo'] == tuple(lo) and s['ghost_hi'][1:] == tuple(hi[1:])
      p0 = lo[0] + want[0] + hi[0]
      assert s['padded'][0] == -(-p0 // vec) * vec
      assert s['padded'][1:] == tuple(
          l + n + h for l, n, h in zip(lo[1:], want[1:], hi[1:]))
      assert s['scratch_bytes'] == int(np.prod(s['padded'])) * per_cell
      total += s['scratch_bytes']
    assert info['scratch_bytes'] == total
  # one cell narrower along any wall: the depth resolves to 1, Bordered's plan
  for d in walls:
    narrow = list(small)
    narrow[d] -= 1
    info, chunks = runtime.border_fused_plan(plan, narrow, modes, DEPTH, rlo,
                                             rhi, lo, hi, 9)
    main, ones = runtime.border_plan(plan, narrow, modes, lo, hi, 9)
    assert info['depth'] == 1 and info['strips'] == [] and chunks == ones == \
        [1] * 9
    assert info['scratch_bytes'] == main['scratch_bytes']
  # depth 1 as given; depth 0: the plan's deepest pass
  info, chunks = runtime.border_fused_plan(plan, small, modes, 1, rlo, rhi, lo,
                                           hi, 9)
  assert info['depth'] == 1 and info['strips'] == [] and chunks == [1] * 9
  deepest = max(p.fused_iters for p in plan.passes[:plan.num_passes])
  big = tuple(8 * n for n in small)
  info, chunks = runtime.border_fused_plan(plan, big, modes, 0, rlo, rhi, lo,
                                           hi, 9)
  assert info['depth'] == deepest
  assert chunks == [deepest] * (9 // deepest) + (
      [9 % deepest] if 9 % deepest else [])


def test_an_all_wrap_plan_is_the_periodic_plan(built):
  from soda_amd import runtime
  st = _stencil('jacobi2d.soda', iterate=9)
  plan = _plan(st, fuse=(4,))
  for depth in (0, 1, 2, 4, 6):
    rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, 'wrap', depth or 4)
    assert (lo, hi) == runtime.periodic_ghosts(st, depth or 4)
    info, chunks = runtime.border_fused_plan(plan, (40, 7), 'wrap', depth, rlo,
                                             rhi, lo, hi, 9)
    want, want_chunks = runtime.periodic_plan(plan, (40, 7), depth, lo, hi, 9)
    assert info['depth'] == want['refill_every'] == (depth or 4)
    assert info['strips'] == [] and chunks == want_chunks
    assert {k: info[k] for k in want} == want


def test_plan_refusals(built):
  from soda_amd import runtime, util
  st = _stencil('jacobi2d.soda')
  plan = _plan(st, fuse=(4,))

  def ok(**kw):
    return runtime.border_fused_plan(
        plan, kw.pop('extent', (40, 30)), kw.pop('modes', ('clamp', 'mirror')),
        kw.pop('depth', 4), kw.pop('rlo', (1, 1)), kw.pop('rhi', (1, 1)),
        kw.pop('lo', (1, 1)), kw.pop('hi', (1, 1)), **kw)
  assert ok()[0]['depth'] == 4 and len(ok()[0]['strips']) == 2
  # its own
  with pytest.raises(util.BackendError, match='invalid.*depth'):
    ok(depth=-1)
  with pytest.raises(util.BackendError, match='invalid.*negative reach'):
    ok(rlo=(-1, 1))
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(rhi=(1, 0))                             # below the plan's reach
  with pytest.raises(util.BackendError, match='invalid.*frame'):
    ok(rlo=(2, 1))                             # a wall's frame below the reach
  with pytest.raises(util.BackendError, match='invalid.*frame'):
    ok(modes=('wrap', 'clamp'))                # a wrapped frame of one iteration
  assert ok(modes=('wrap', 'clamp'), lo=(4, 1), hi=(4, 1))[0]['depth'] == 4
  with pytest.raises(util.BackendError, match='invalid.*frame'):
    ok(modes='wrap', lo=(4, 3), hi=(4, 4))
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    ok(refill_every=2)
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    ok(modes='wrap', lo=(4, 4), hi=(4, 4), refill_every=4)
  # what soda_hip_border_plan refuses
  with pytest.raises(util.BackendError, match='invalid.*mode'):
    ok(modes=(1, 5))
  with pytest.raises(util.InputError, match='unknown mode'):
    ok(modes='edge')
  with pytest.raises(util.BackendError, match='unsupported.*preserve'):
    ok(preserve=True)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.border_fused_plan(_plan(st, fuse=(4,), batch=True), (40, 30),
                              'clamp', 4, (1, 1), (1, 1), (1, 1), (1, 1))
  with pytest.raises(util.BackendError, match='invalid.*last dimension'):
    ok(lo=(1, 0))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(extent=(0, 30))
  with pytest.raises(util.BackendError, match='invalid'):
    ok(lo=(-1, 1))
  # a program that cannot iterate: depth 1, one iteration served
  sobel = _stencil('sobel2d.soda')
  splan = _plan(sobel)
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(sobel, 'mirror101', 3)
  info, chunks = runtime.border_fused_plan(splan, (64, 48), 'mirror101', 3,
                                           rlo, rhi, lo, hi, 1,
                                           not_iterable=True)
  assert info['depth'] == 1 and chunks == [1] and info['strips'] == []
  with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
    runtime.border_fused_plan(splan, (64, 48), 'mirror101', 3, rlo, rhi, lo,
                              hi, 2, not_iterable=True)
  # P[0] of the domain beyond a kernel's max_extent0
  xs = _plan(st, (256, 8), fuse=(2,), xshare=True, row_cells=256)
  limit = max(q.max_extent0 for q in xs.kernels[:xs.num_kernels])
  with pytest.raises(util.BackendError, match='invalid.*rows of at most'):
    runtime.border_fused_plan(xs, (limit, 30), 'clamp', 2, (1, 1), (1, 1),
                              (1, 1), (1, 1))
  # the python layer: depth, and a window that does not grow linearly
  with pytest.raises(util.InputError, match='depth'):
    runtime.border_fused_ghosts(st, 'clamp', 0)


# ---------------------------------------------------------------------------
# CPU: the scheme itself, by the numpy oracle from the plan's numbers
# ---------------------------------------------------------------------------

SCHEME = [(n, None, None) for n in sorted(GEOMETRY)] + [
    ('jacobi2d', m, -3.5) for m in borders.MODES if m != 'clamp'] + [
        ('jacobi2d', ('wrap', 'clamp'), None),
        ('jacobi2d', ('mirror', 'constant'), -3.5),
        ('blur', 'clamp', None)]


@pytest.mark.parametrize('name,modes,cst', SCHEME, ids=[
    '%s-%s' % (n, m if isinstance(m, (str, type(None))) else '.'.join(m))
    for n, m, _ in SCHEME])
def test_the_scheme_by_the_oracle(built, name, modes, cst):
  """Interior as DEPTH open-box iterations on the padded array, strips as
  bordered runs of their own, scattered by the plan's widths, at N = L + H in
  every wall dimension: the bits of borders.expected, with 1, DEPTH - 1, DEPTH
  iterations in the last chunk."""
  from soda_amd import runtime
  st, plan, m0, c0, rlo, rhi, _, _ = _geometry(name)
  if modes is None:
    modes, cst = m0, c0
  rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, modes, DEPTH)
  extent = _smallest(st, modes, rlo, rhi, roomy=7)
  ins = periodic.inputs(st, extent, seed=2)
  for iterate in (DEPTH + 1, 2 * DEPTH - 1, DEPTH):
    info, chunks = runtime.border_fused_plan(plan, extent, modes, DEPTH, rlo,
                                             rhi, lo, hi, iterate)
    all_wrap = set(borders.per_dim(modes, st.dim)) == {'wrap'}
    assert info['depth'] == DEPTH and sum(chunks) == iterate
    assert bool(info['strips']) != all_wrap
    got = rims.emulate(st, ins, modes, cst, info, chunks)
    want = borders.expected(st, ins, iterate, modes, cst)
    for o in want:
      assert periodic.same_bits(got[o], want[o]), (
          iterate, o, periodic.differing(got[o], want[o]))


def test_the_emulation_sees_a_scatter_that_is_too_narrow(built):
  """The test above is no tautology: with the scatter one cell short, cells
  differ."""
  from soda_amd import runtime
  st, plan, modes, cst, rlo, rhi, lo, hi = _geometry('blur')
  extent = _smallest(st, modes, rlo, rhi)
  ins = periodic.inputs(st, extent, seed=2)
  info, chunks = runtime.border_fused_plan(plan, extent, modes, DEPTH, rlo, rhi,
                                           lo, hi, DEPTH)
  want = borders.expected(st, ins, DEPTH, modes, cst)
  short = dict(info, strips=[dict(s, take_hi=s['take_hi'] - 1)
                             for s in info['strips']])
  got = rims.emulate(st, ins, modes, cst, short, chunks)
  assert not all(periodic.same_bits(got[o], want[o]) for o in want)


# ---------------------------------------------------------------------------
# CPU: the modules, the interface
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dim', (1, 2, 3, 4))
def test_the_kernels_compile_without_scratch(built, dim):
  """The box module of every cell size and dimension count, for gfx950: one
  kernel, no scratch, no LDS, plain C++."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import box as gen
  for elem in sorted(SIZES):
    _, res = runtime.box_resources(elem, dim)
    name = gen.kernel_name(elem, dim)
    assert name == 'soda_box_e%d_d%d' % (elem, dim)
    assert sorted(res) == [name]
    assert res[name]['scratch'] == 0, res[name]
    assert res[name]['lds'] == 0 and 0 < res[name]['vgpr'] <= 64, res[name]
    text = gen.source(elem, dim)
    own = text.split('soda_rt_box.h', 1)[1]
    assert 'asm' not in own and '__shared__' not in own
  with pytest.raises(util.SemanticError):
    gen.source(3, 2)
  with pytest.raises(util.SemanticError):
    gen.source(4, 5)


def test_existing_modules_are_untouched():
  """The wrap and extend modules and the programs' modules are what they
  were: none mentions the box module, no LowerOptions field was added."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import box, extend, lower, wrap
  for elem in sorted(SIZES):
    for dim in (1, 2, 3, 4):
      box.source(elem, dim)
      for text in (wrap.source(elem, dim), extend.source(elem, dim)):
        assert 'soda_box' not in text and 'SODA_BOX' not in text
  for name, skw, okw in [('jacobi2d.soda', dict(iterate=13), dict(fuse=(4,))),
                         ('heat3d.soda', dict(iterate=4), dict(fuse=(2,))),
                         ('blur.soda', {}, {})]:
    stencil = _stencil(name, **skw)
    opts = runtime.resolve_options(stencil, _opts(**okw), None, probe=False)
    before = lower.lower(stencil, opts)
    runtime.border_fused_ghosts(stencil, 'clamp', 3)
    after = lower.lower(stencil, opts)
    assert before.source == after.source
    assert 'soda_box' not in after.source and 'SODA_BOX' not in after.source
    assert bytes(runtime.make_plan(before)) == bytes(runtime.make_plan(after))
  assert not any('border' in f or 'box' in f or 'depth' in f
                 for f in lower.LowerOptions.__dataclass_fields__)


def test_abi_and_structs(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == 9
  assert lib.soda_hip_sizeof(17) == ctypes.sizeof(runtime.BorderDesc) == 208
  assert lib.soda_hip_sizeof(18) == ctypes.sizeof(runtime.BorderFusedDesc) == \
      248
  assert lib.soda_hip_sizeof(19) == ctypes.sizeof(runtime.BorderStrip) == 104
  assert lib.soda_hip_sizeof(20) == ctypes.sizeof(runtime.BorderFusedInfo) == \
      496
  for name in ('soda_hip_box_host', 'soda_hip_border_fused_plan',
               'soda_hip_border_fused_create', 'soda_hip_border_fused_destroy',
               'soda_hip_border_fused_info', 'soda_hip_border_fused_move',
               'soda_hip_border_fused_run_padded',
               'soda_hip_border_fused_run_device'):
    assert name in runtime.API and hasattr(lib, name), name
  import inspect
  for fn in (runtime.Program.bordered, runtime.Program.run_bordered):
    assert inspect.signature(fn).parameters['depth'].default == 1


def test_command_line_has_the_depth():
  run = subprocess.run([sys.executable, '-m', 'soda_amd.sodac', '--help'],
                       capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode == 0 and '--hip-border-depth' in run.stdout
  run = subprocess.run(
      [sys.executable, '-m', 'soda_amd.sodac', '--hip-backend',
       '--hip-extent', '64', '8', '--hip-border-depth', '4',
       soda_path('jacobi2d.soda')],
      capture_output=True, text=True, cwd=ROOT, timeout=120)
  assert run.returncode != 0 and '--hip-border-depth needs --hip-border' in (
      run.stdout + run.stderr), (run.stdout, run.stderr)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _ct(t):
  return lambda: celltypes.stencil_of(t, 2, 'main', 9)


# program name -> (stencil, LowerOptions keywords)
PROGRAMS = {
    'jacobi2d': (lambda: _stencil('jacobi2d.soda', iterate=9),
                 dict(fuse=(4,))),
    'jacobi2d_v1': (lambda: _stencil('jacobi2d.soda', iterate=9),
                    dict(fuse=(4,), vec=1)),
    'skew2d': (lambda: _stencil('skew2d.soda', iterate=5), {}),
    'coupled2d': (lambda: _stencil('coupled2d.soda', iterate=5),
                  dict(fuse=(2,))),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=5), dict(fuse=(2,))),
    'blur': (lambda: _stencil('blur.soda', iterate=5), {}),
    'ints2d': (lambda: _stencil('ints2d.soda', iterate=5), {}),
    'heat4d': (lambda: _stencil('heat4d.soda', iterate=3),
               dict(strategy='direct')),
    'double': (_ct('double'), dict(fuse=(4,), chunk_rows=16)),
    'uint8': (_ct('uint8'), dict(fuse=(4,), chunk_rows=16)),
}
# case name -> (program, extent, iterate, modes, constants, depth asked,
# depth resolved)
CASES = {
    # once per mode, all dimensions alike: chunks 4, 4, 1
    'wrap': ('jacobi2d', (40, 30), 9, 'wrap', None, 0, 4),
    'clamp': ('jacobi2d', (40, 30), 9, 'clamp', None, 0, 4),
    'mirror': ('jacobi2d', (40, 30), 9, 'mirror', None, 0, 4),
    'mirror101': ('jacobi2d', (40, 30), 9, 'mirror101', None, 0, 4),
    'constant': ('jacobi2d', (40, 30), 9, 'constant', -3.5, 0, 4),
    'wrap_clamp': ('jacobi2d', (40, 30), 9, ('wrap', 'clamp'), None, 0, 4),
    'mirror_constant': ('jacobi2d', (40, 30), 9, ('mirror', 'constant'), -3.5,
                        0, 4),
    # other programs
    'blur': ('blur', (48, 26), 5, 'mirror101', None, 3, 3),     # one-sided
    'skew2d': ('skew2d', (40, 28), 5, ('constant', 'mirror101'), 2.0, 3, 3),
    'coupled2d': ('coupled2d', (36, 25), 5, 'constant',
                  {'a': 1.5, 'b': -2.0}, 0, 2),
    'ints2d': ('ints2d', (36, 22), 5, ('clamp', 'constant'), 201, 3, 3),
    'heat3d': ('heat3d', (20, 14, 12), 5, ('mirror', 'clamp', 'wrap'), None,
               0, 2),
    'heat4d': ('heat4d', (5, 4, 4, 3), 3, 'mirror101', None, 0, 1),
    'double': ('double', (24, 21), 9, 'mirror', None, 0, 4),
    'uint8': ('uint8', (48, 19), 9, ('constant', 'clamp'), 77, 0, 4),
}
# the smallest extent that keeps depth 4 (the two parts of a strip abut), and
# one cell below it in either dimension
for _m in borders.MODES:
  if _m != 'wrap':
    CASES['16x16_' + _m] = ('jacobi2d', (16, 16), 9, _m, -3.5, 0, 4)
    CASES['15x16_' + _m] = ('jacobi2d', (15, 16), 9, _m, -3.5, 0, 1)
    CASES['16x15_' + _m] = ('jacobi2d', (16, 15), 9, _m, -3.5, 0, 1)

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
  """(program name, stencil, extent, iterate, modes, constants, depth asked,
  depth resolved, inputs, expected), computed once."""
  key = (name, seed)
  if key not in _EXPECTED:
    pname, extent, iterate, modes, cst, depth, resolved = CASES[name]
    stencil = PROGRAMS[pname][0]()
    ins = periodic.inputs(stencil, extent, seed)
    _EXPECTED[key] = (pname, stencil, extent, iterate, modes, cst, depth,
                      resolved, ins,
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
  pname, stencil, extent, iterate, modes, cst, depth, resolved, ins, want = \
      _case(name)
  assert all(np.isfinite(w).all() for w in want.values() if w.dtype.kind == 'f')
  prog = programs(pname)
  with prog.bordered(extent, modes, cst, depth=depth) as bor:
    info = bor.info()
    got = _dense(prog, bor, ins, iterate)
  assert info['depth'] == resolved
  all_wrap = set(borders.per_dim(modes, stencil.dim)) == {'wrap'}
  raw = borders.per_dim(modes, stencil.dim)
  rlo, rhi = periodic.reach(stencil, 1)
  if resolved > 1 and not all_wrap:
    assert [s['dim'] for s in info['strips']] == [
        d for d in range(stencil.dim) if raw[d] != 'wrap' and rlo[d] + rhi[d]]
    assert info['refill_every'] == 1
  else:
    assert info['strips'] == []
  if name.startswith('16x16_'):
    assert [s['extent'] for s in info['strips']] == [(16, 16), (16, 16)]
  _assert_same(got, want, name)
  with prog.bordered(extent, modes, cst) as plain:         # today's handle
    _assert_same(got, _dense(prog, plain, ins, iterate), name + ' at depth 1')
  if name in ('constant', 'coupled2d'):
    # numpy in, numpy out
    _assert_same(prog.run_bordered(ins, modes, cst, iterate, depth=depth),
                 want, 'run_bordered')


@pytest.mark.gpu
def test_every_depth_gives_the_same_bits(programs):
  _, stencil, extent, iterate, modes, cst, _, _, ins, want = _case(
      'mirror_constant')
  prog = programs('jacobi2d')
  plain = prog.run_bordered(ins, modes, cst, iterate)
  _assert_same(plain, want, 'the default')
  for depth, resolved in ((1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (6, 6)):
    with prog.bordered(extent, modes, cst, depth=depth) as bor:
      assert bor.info().get('depth', 1) == resolved
      got = _dense(prog, bor, ins, iterate)
    _assert_same(got, want, 'depth %d' % depth)
    _assert_same(got, plain, 'depth %d against the default' % depth)


@pytest.mark.gpu
def test_all_wrap_is_the_torus(programs):
  _, stencil, extent, iterate, _, _, _, _, ins, want = _case('wrap')
  prog = programs('jacobi2d')
  with prog.bordered(extent, 'wrap', depth=0) as bor, \
      prog.periodic(extent) as per:
    info = bor.info()
    assert {k: info[k] for k in per.info()} == per.info()
    assert info['refill_every'] == info['depth'] == 4
    got = _dense(prog, bor, ins, iterate)
  _assert_same(got, prog.run_periodic(ins, iterate), 'run_periodic')
  _assert_same(got, want, 'per iteration')


@pytest.mark.gpu
def test_padded_entry_across_calls(programs):
  """Two run_padded calls of 3 and 4 iterations equal one dense run of 7; the
  outputs come back extended; the inputs are byte-identical afterwards."""
  _, stencil, extent, _, _, _, _, _, ins, _ = _case('clamp')
  prog = programs('jacobi2d')
  for modes, cst in (('clamp', 0), (('mirror101', 'constant'), -3.5),
                     (('wrap', 'mirror'), 0)):
    want = borders.expected(stencil, ins, 7, modes, cst)
    with prog.bordered(extent, modes, cst, depth=3) as bor, \
        periodic.Device(prog) as dev:
      info = bor.info()
      assert info['depth'] == 3
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
                                  'blur', '16x16_mirror101'])
def test_dense_entry_between_guard_bands(programs, name):
  pname, stencil, extent, iterate, modes, cst, depth, resolved, ins, want = \
      _case(name)
  prog = programs(pname)
  with prog.bordered(extent, modes, cst, depth=depth) as bor:
    assert bor.info()['depth'] == resolved > 1
    got, violation, _ = guarded.run(_DenseEntry(prog, bor), stencil, extent,
                                    ins, iterate)
  assert violation is None, violation
  _assert_same(got, want, name)


@pytest.mark.gpu
@pytest.mark.parametrize('modes,cst', [('mirror101', 0),
                                       (('constant', 'clamp'), -3.5)])
def test_padded_entry_at_addresses_aligned_to_the_cell_only(programs, modes,
                                                            cst):
  """The padded entry of a program without vector accesses, on arrays that
  start 1 and 3 cells behind a 16-byte line: the gather reads such inputs,
  the scatter writes such outputs.  Every byte in front of and behind the
  outputs and every byte of the inputs stays what was planted; the outputs
  come out extended, bit for bit."""
  _, stencil, extent, _, _, _, _, _, ins, _ = _case('clamp')
  prog = programs('jacobi2d_v1')
  want = borders.expected(stencil, ins, 4, modes, cst)
  with prog.bordered(extent, modes, cst, depth=4) as bor, \
      periodic.Device(prog) as dev:
    info = bor.info()
    assert info['depth'] == 4 and len(info['strips']) == 2
    lo, hi = info['ghost_lo'], info['ghost_hi']
    start = borders.pad(ins['t1'], lo, hi, modes, cst)
    rng = np.random.default_rng(11)
    for lead_in, lead_out in ((1, 3), (3, 1), (0, 2)):
      raw_in = rng.integers(0, 256, size=(lead_in + start.size + 5) * 4,
                            dtype=np.uint8)
      raw_in[lead_in * 4:(lead_in + start.size) * 4] = start.view(
          np.uint8).reshape(-1)
      raw_out = rng.integers(0, 256, size=(lead_out + start.size + 5) * 4,
                             dtype=np.uint8)
      d_in, d_out = dev.upload(raw_in), dev.upload(raw_out)
      bor.run_padded([d_out + lead_out * 4], [d_in + lead_in * 4], 4)
      back_in = dev.download(d_in, raw_in.shape, np.uint8)
      back_out = dev.download(d_out, raw_out.shape, np.uint8)
      assert (back_in == raw_in).all()
      n = lead_out * 4
      assert (back_out[:n] == raw_out[:n]).all()
      assert (back_out[-20:] == raw_out[-20:]).all()
      arr = back_out[n:n + start.nbytes].view(np.float32).reshape(start.shape)
      _assert_same({'t0': periodic.interior(arr, info)}, want,
                   'lead %d / %d' % (lead_in, lead_out))
      form = borders.closed_form(periodic.interior(arr, info), lo, hi, modes,
                                 cst)
      assert periodic.same_bits(arr, form), periodic.differing(arr, form)


def _strip_cut(info, strip, extent, along):
  """Index of the domain's cells in a padded array, `along` = (start, stop)
  in domain coordinates along the strip's dimension."""
  idx = []
  for d in range(len(extent)):
    g = info['ghost_lo'][d]
    lo, hi = along if d == strip['dim'] else (0, extent[d])
    idx.append(slice(g + lo, g + hi))
  return tuple(idx[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['clamp', 'blur', 'heat3d', 'double',
                                  'uint8'])
def test_gather_and_scatter_on_planted_bytes(programs, name):
  """The two primitives on random bytes, both sides 0, 1 and 3 cells behind a
  16-byte line: the gather writes the strip's domain and nothing else, the
  scatter the two rims of the main array and nothing else; the source keeps
  every byte.  Expected by numpy slicing from the numbers of info()."""
  pname, stencil, extent, _, modes, cst, depth, _, _, _ = _case(name)
  prog = programs(pname)
  dtype = np.dtype(stencil.output_types[0].np_name)
  isz = dtype.itemsize
  with prog.bordered(extent, modes, cst, depth=depth) as bor, \
      periodic.Device(prog) as dev:
    info = bor.info()
    assert info['strips']
    shape = info['padded'][::-1]
    rng = np.random.default_rng(11)
    for k, strip in enumerate(info['strips']):
      sshape = strip['padded'][::-1]
      d, L, H = strip['dim'], strip['lo'], strip['hi']
      tl, th, n = strip['take_lo'], strip['take_hi'], extent[strip['dim']]
      sext = strip['extent']
      for lead_m, lead_s in ((0, 0), (1, 3), (3, 2)):
        for gather in (True, False):
          raw_m = rng.integers(0, 256, dtype=np.uint8, size=(
              lead_m + int(np.prod(shape)) + 5) * isz)
          raw_s = rng.integers(0, 256, dtype=np.uint8, size=(
              lead_s + int(np.prod(sshape)) + 5) * isz)
          cells = lambda raw, lead, shp: raw[lead * isz:(
              lead + int(np.prod(shp))) * isz].view(dtype).reshape(shp)
          want_m, want_s = raw_m.copy(), raw_s.copy()
          m, st = cells(want_m, lead_m, shape), cells(want_s, lead_s, sshape)
          if gather:
            st[_strip_cut(info, strip, sext, (0, L))] = \
                m[_strip_cut(info, strip, extent, (0, L))]
            st[_strip_cut(info, strip, sext, (L, L + H))] = \
                m[_strip_cut(info, strip, extent, (n - H, n))]
          else:
            m[_strip_cut(info, strip, extent, (0, tl))] = \
                st[_strip_cut(info, strip, sext, (0, tl))]
            m[_strip_cut(info, strip, extent, (n - th, n))] = \
                st[_strip_cut(info, strip, sext, (L + H - th, L + H))]
          d_m, d_s = dev.upload(raw_m), dev.upload(raw_s)
          if gather:
            bor.gather(k, [d_s + lead_s * isz], [d_m + lead_m * isz])
          else:
            bor.scatter(k, [d_m + lead_m * isz], [d_s + lead_s * isz])
          got_m = dev.download(d_m, raw_m.shape, np.uint8)
          got_s = dev.download(d_s, raw_s.shape, np.uint8)
          assert (got_m == want_m).all(), (k, lead_m, lead_s, gather)
          assert (got_s == want_s).all(), (k, lead_m, lead_s, gather)
          assert not (gather and (want_s == raw_s).all())
          assert gather or tl + th == 0 or not (want_m == raw_m).all()
    # refusals: no such strip, a misaligned array
    from soda_amd import util
    d_m = dev.alloc(int(np.prod(shape)) * isz + 16)
    with pytest.raises(util.BackendError, match='invalid.*strip'):
      bor.gather(len(info['strips']), [d_m], [d_m])
    if isz > 1:
      with pytest.raises(util.BackendError, match='invalid.*aligned'):
        bor.gather(0, [d_m + 1], [d_m])


@pytest.mark.gpu
def test_dense_entry_on_a_side_stream_ahead_of_its_inputs(programs):
  _, stencil, extent, iterate, modes, cst, depth, _, ins, want = _case(
      'mirror_constant')
  prog = programs('jacobi2d')
  shape = extent[::-1]
  with prog.bordered(extent, modes, cst, depth=depth) as bor:
    _dense(prog, bor, ins, iterate)       # sizes and times the program
    got = asyncrun.late_fill(
        'fused bordered dense entry', ins, {'t0': (shape, np.float32)},
        lambda run: bor.run_device(run.outs(), run.ins(), iterate,
                                   stream=run.ptr))
  _assert_same(got, want, 'late fill')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mirror101', 'heat3d'])
def test_dense_entry_captured_and_replayed(programs, name):
  import torch
  pname, stencil, extent, iterate, modes, cst, depth, resolved, ins, want = \
      _case(name)
  ins2, want2 = _case(name, seed=5)[8:]
  prog = programs(pname)
  i_name, o_name = stencil.input_names[0], stencil.output_names[0]
  S = torch.cuda.Stream()
  with prog.bordered(extent, modes, cst, depth=depth) as bor:
    assert bor.info()['depth'] == resolved > 1
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
  _, stencil, extent, iterate, modes, cst, _, _, ins, _ = _case('clamp')
  prog = programs('jacobi2d')
  with prog.bordered(extent, modes, depth=0) as bor:
    _dense(prog, bor, ins, iterate)
    held = bor.info()['scratch_bytes']
    with pytest.raises(util.InputError, match='no fill'):
      bor.fill([])
    with pytest.raises(util.BackendError, match='invalid'):
      with periodic.Device(prog) as dev:
        d = dev.upload(ins['t1'])
        bor.run_device([d], [d], 0)
    with pytest.raises(util.BackendError, match='overlaps an input'):
      with periodic.Device(prog) as dev:
        d = dev.upload(ins['t1'])
        bor.run_device([d], [d], 4)
    assert bor.info()['scratch_bytes'] == held
  launches, scratch = prog.last_launches(), prog.scratch()
  with pytest.raises(util.InputError, match='unknown mode'):
    prog.bordered(extent, 'reflect', depth=4)
  with pytest.raises(util.InputError, match='depth'):
    prog.bordered(extent, 'clamp', depth=-2)
  with pytest.raises(util.InputError, match='no inputs'):
    prog.bordered(extent, 'constant', {'t9': 1.0}, depth=4)
  # the library's own refusals, through the raw entry
  for mode, depth, lo, rlo, what in (((1, 9), 4, (1, 1), (1, 1), 'mode'),
                                     ((1, 1), -1, (1, 1), (1, 1), 'depth'),
                                     ((1, 1), 4, (1, 1), (2, 1), 'frame'),
                                     ((0, 1), 4, (1, 1), (1, 1), 'frame')):
    desc = runtime._border_fused_desc(runtime._border_desc(
        runtime._periodic_desc(2, extent, 0, lo, (1, 1), False), mode, (0,)),
                                      depth, rlo, (1, 1))
    codes, sizes = (ctypes.c_void_p * 4)(), (ctypes.c_size_t * 4)()
    handle = ctypes.c_void_p()
    rc = runtime.library().soda_hip_border_fused_create(
        prog._handle, ctypes.byref(desc), codes, sizes, codes, sizes,
        ctypes.byref(handle))
    assert rc != 0 and not handle.value and what in runtime.last_error()
  assert prog.last_launches() == launches and prog.scratch() == scratch
  assert prog._periodic == []
  # `border: preserve`, a batched plan
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3, border='preserve'),
                       _opts(fuse=(2,))) as pres:
    before = pres.last_launches(), pres.scratch()
    with pytest.raises(util.BackendError, match='unsupported.*preserve'):
      pres.bordered(extent, 'clamp', depth=0)
    assert (pres.last_launches(), pres.scratch()) == before
  with runtime.Program(_stencil('jacobi2d.soda', iterate=3),
                       _opts(fuse=(2,), batch=True)) as bat:
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      bat.bordered(extent, 'mirror', depth=0)
  # sobel2d cannot iterate: depth 1, one iteration served, two refused
  sobel = _stencil('sobel2d.soda')
  sext = (32, 26)
  sins = periodic.inputs(sobel, sext)
  with runtime.Program(sobel, _opts()) as sp, \
      sp.bordered(sext, 'mirror101', depth=3) as bor, \
      periodic.Device(sp) as dev:
    assert bor.info()['depth'] == 1 and bor.info()['strips'] == []
    _assert_same(_dense(sp, bor, sins, 1),
                 borders.expected(sobel, sins, 1, 'mirror101'), 'sobel2d')
    d_dense = dev.upload(sins['img'])
    d_out = dev.alloc(sins['img'].nbytes)
    with pytest.raises(util.BackendError, match='invalid.*cannot iterate'):
      bor.run_device([d_out], [d_dense], 2)
