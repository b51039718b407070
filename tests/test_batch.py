"""Batched runs (`LowerOptions.batch`, soda_hip_run_device_batch): many
independent grids of one extent in one launch per kernel.

CPU: the default text is what it was, every family has a batched form that
compiles to the registers of the unbatched one, the launch geometry sees the
batch, the refusals, the command line.  GPU: bit for bit against the C oracle,
item by item, on programs built without an extent and never calibrated; every
case also runs the device entry on output buffers one item longer at each end
and checks that the two guard items keep their fill pattern -- which is what
catches a wrong item offset or stride."""
import ctypes
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, soda_path
import fuzz

SUFFIX = '_bt'
GUARD = 0xA5


def _stencil(name, **kw):
  from soda_amd import core
  kw = {k: v for k, v in kw.items() if v is not None}
  if name.endswith('.soda'):
    return core.from_file(soda_path(name), **kw)
  return core.from_text(name, **kw)


def _opts(batch=True, **kw):
  from soda_amd.codegen.hip import lower
  return lower.LowerOptions(batch=batch, **kw)


def _build(stencil, opts):
  """(module, {kernel: resources}) as runtime.Program builds them for no
  extent in particular."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  mod = lower.lower(stencil, runtime.resolve_options(stencil, opts, None))
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, '%s.hip' % stencil.app_name))
  return mod, res


def _fused(mod, depth):
  k, = [k for k in mod.kernels if k.tune and k.tune.get('fused') == depth]
  return k


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

# (program, iterate, options): one per kernel family, then the other forms of
# the marching kernels
FAMILIES = [
    ('jacobi2d.soda', 30, dict(fuse=(13,))),
    ('heat3d.soda', 4, dict(fuse=(2,))),
    ('blur.soda', None, dict()),
    ('contrast.soda', None, dict()),                         # ldswin
    ('heat4d.soda', None, dict()),                           # direct
    ('heat3d.soda', 4, dict(strategy='tile3d', fuse=(3,))),
]
FORMS = [
    ('heat3d.soda', 4, dict(fuse=(2,), xshare=True, row_cells=256), '_xs1'),
    ('heat3d.soda', 4, dict(fuse=(2,), xshare_block=2), '_xb2'),
    ('jacobi2d.soda', 30, dict(fuse=(4,), pipe=4), '_pipe4'),
]


@pytest.mark.parametrize('name,iterate,kw', FAMILIES)
def test_default_text_is_unchanged(name, iterate, kw):
  from soda_amd.codegen.hip import lower
  stencil = _stencil(name, iterate=iterate)
  plain = lower.lower(stencil, lower.LowerOptions(peel=0, **kw))
  same = lower.lower(stencil, lower.LowerOptions(batch=False, peel=0, **kw))
  assert same.source == plain.source
  assert 'blockIdx.y' not in plain.source
  assert 'soda_batch' not in plain.source
  assert not any(k.name.endswith(SUFFIX) for k in plain.kernels)
  assert not getattr(plain, 'batch', False)
  batched = lower.lower(stencil, lower.LowerOptions(batch=True, peel=0, **kw))
  assert [k.name for k in batched.kernels] == \
      [k.name + SUFFIX for k in plain.kernels]
  family = {'contrast.soda': 'ldswin', 'heat4d.soda': 'direct'}.get(name)
  if family:
    assert all(family in k.name for k in batched.kernels)
  if kw.get('strategy') == 'tile3d':
    assert any('tile3d' in k.name for k in batched.kernels)
  for k, text in zip(batched.kernels, batched.chunks):
    assert k.name + '(soda_hip_kargs_t soda_a0) {' in text
    assert 'blockIdx.y' in text
  # nothing else differs: a batched kernel is the unbatched one behind a head
  # that moves the tensor slots of a copy of the argument block
  for b, p in zip(batched.chunks, plain.chunks):
    body = b.split('(soda_hip_kargs_t soda_a0) {\n', 1)[1].split('\n')
    while body[0].startswith(('  // batched:', '  soda_hip_kargs_t a = soda_a0;',
                              '  const int64_t soda_item = ',
                              '  a.buf[')):
      body.pop(0)
    assert '\n'.join(body) == p.split('(soda_hip_kargs_t a) {\n', 1)[1]


def test_param_slots_are_not_moved():
  from soda_amd.codegen.hip import lower
  stencil = _stencil('conv2d.soda')
  assert stencil.param_names
  mod = lower.lower(stencil, _opts(peel=0))
  moved = len(stencil.input_names) + len(stencil.output_names) + \
      len(stencil.local_names)
  for text in mod.chunks:
    head = text[:text.index('soda_item);') + 400]
    for slot in range(moved):
      assert 'a.buf[%d] = soda_batch_base<' % slot in head
    for p in stencil.param_names:
      assert 'a.buf[%d] = soda_batch_base' % mod.slot[p] not in text


@pytest.mark.parametrize('name,iterate,kw,tag',
                         [f + (None,) for f in FAMILIES] + FORMS)
def test_batched_modules_compile_to_the_same_registers(built, name, iterate,
                                                       kw, tag):
  from soda_amd import runtime
  stencil = _stencil(name, iterate=iterate)
  plain, pres = _build(stencil, _opts(batch=False, **kw))
  mod, res = _build(stencil, _opts(**kw))
  assert len(mod.kernels) == len(plain.kernels)
  if tag:
    assert any(tag in k.name for k in mod.kernels), [k.name for k in mod.kernels]
  for k, p in zip(mod.kernels, plain.kernels):
    assert k.name == p.name + SUFFIX
    r, q = res[k.name], pres[p.name]
    assert r['scratch'] == 0, (k.name, r)
    assert runtime.waves_per_simd(r['vgpr']) >= \
        runtime.waves_per_simd(q['vgpr']), (k.name, r, q)
  assert runtime.make_plan(mod, res).batched == 1
  assert runtime.make_plan(plain, pres).batched == 0


def _chunk_checks(name, iterate, fuse, depth, extent):
  from soda_amd import runtime
  stencil = _stencil(name, iterate=iterate)
  mod, res = _build(stencil, _opts(fuse=fuse))
  plan = runtime.make_plan(mod, res)
  at = mod.kernels.index(_fused(mod, depth))
  row = [p.fused_iters for p in mod.sorted_passes()].index(depth)
  ax = stencil.dim - 1
  chunk, ns = {}, {}
  for batch in (1, 4, 16, 64):
    tiles, times = runtime.plan_geometry_batch(plan, extent, batch)
    chunk[batch], ns[batch] = tiles[at][ax], times[row]
  assert chunk[64] > chunk[1], chunk
  assert chunk[1] <= chunk[4] <= chunk[16] <= chunk[64], chunk
  assert 0 < ns[64] < 64 * ns[1], ns
  return plan, chunk


def test_geometry_sees_the_batch(built):
  from soda_amd import runtime
  plan, chunk = _chunk_checks('jacobi2d.soda', 100, (13,), 13, (512, 512))
  assert chunk[1] == 8, chunk            # what a lone 512^2 grid gets today
  for extent in ((512, 512), (1920, 1080), (8192, 8192)):
    assert runtime.plan_geometry_batch(plan, extent, 1) == \
        runtime.plan_geometry(plan, extent)
    assert runtime.plan_schedule_batch(plan, extent, 1, 100) == \
        runtime.plan_schedule(plan, extent, 100)
  plan3, _ = _chunk_checks('heat3d.soda', 50, (2,), 2, (128, 128, 128))
  assert runtime.plan_geometry_batch(plan3, (128, 128, 128), 1) == \
      runtime.plan_geometry(plan3, (128, 128, 128))


def test_refusals(built):
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=8)
  mod, res = _build(stencil, _opts(fuse=(4,)))
  plan = runtime.make_plan(mod, res)
  lib = runtime.library()
  ext = (ctypes.c_int32 * runtime.MAX_DIM)(512, 512, 1, 1)
  count = (ctypes.c_int32 * plan.num_passes)()
  for bad in (0, 65536, -1):
    assert lib.soda_hip_plan_geometry_batch(ctypes.byref(plan), ext, bad, None,
                                            None) == 1       # ERR_INVALID
    assert 'batch' in runtime.last_error()
    assert lib.soda_hip_plan_schedule_batch(ctypes.byref(plan), ext, bad, 8,
                                            count) == 1
    with pytest.raises(util.BackendError, match='batch'):
      runtime.plan_geometry_batch(plan, (512, 512), bad)
  assert lib.soda_hip_plan_geometry_batch(ctypes.byref(plan), ext, 65535, None,
                                          None) == 0
  with pytest.raises(util.SemanticError, match='batch'):
    lower.lower(stencil, _opts(fuse=(4,), banks={'t1': 2}))
  # run_device(batch=...) is a run on whole grids (checked before any call
  # into the library: an object with just what the check reads)
  class Stub(runtime.Program):
    def __init__(self):
      self.stencil = stencil
    def __del__(self):
      pass
  for extra in (dict(keep=(2, 30)), dict(ghosts=(1, 1)), dict(sends=(1, 1)),
                dict(origin=(0, 0))):
    with pytest.raises(util.InputError, match='batch'):
      Stub().run_device([1], [2], (64, 32), batch=2, **extra)


def test_sodac_prints_batched_kernels(built):
  for name, fuse in (('jacobi2d.soda', '4'), ('heat3d.soda', '2')):
    cmd = [sys.executable, '-m', 'soda_amd.sodac', soda_path(name),
           '--iterate', '8', '--hip-fuse', fuse, '--hip-no-probe',
           '--hip-kernel', '-']
    r = subprocess.run(cmd + ['--hip-batch'], capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr
    heads = [l for l in r.stdout.splitlines() if '__global__' in l]
    assert len(heads) == 2
    for l in heads:
      assert l.endswith(SUFFIX + '(soda_hip_kargs_t soda_a0) {'), l
    assert r.stdout.count('blockIdx.y') >= 2
    plain = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    assert plain.returncode == 0, plain.stderr
    assert 'blockIdx.y' not in plain.stdout and SUFFIX + '(' not in plain.stdout


def test_the_ldswin_case_is_the_smallest_program_the_family_accepts():
  """The GPU test of `ldswin` below is to use the smallest program under
  tests/golden that strategy='ldswin' accepts."""
  import glob
  import os
  from soda_amd import core, util
  from soda_amd.codegen.hip import lower
  from conftest import GOLDEN_DIR, SODA_DIR
  sizes = {}
  for path in glob.glob(os.path.join(GOLDEN_DIR, '*.soda')) + \
      glob.glob(os.path.join(SODA_DIR, '*.soda')):
    try:
      lower.lower(core.from_file(path), _opts(strategy='ldswin'))
    except util.SodaError:
      continue
    sizes[os.path.basename(path)] = os.path.getsize(path)
  assert min(sizes, key=sizes.get) == LDSWIN_PROGRAM, sizes


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

LDSWIN_PROGRAM = 'jacobi2d.soda'


def _inputs(stencil, extent, batch, seed=0):
  """Different random data per item; the param arrays are shared."""
  shape = (batch,) + tuple(extent[::-1])
  rng = np.random.default_rng(seed)
  out = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if t.is_float:
      out[name] = rng.random(shape, dtype=np.float64).astype(dt)
    else:
      out[name] = rng.integers(0, 201, size=shape).astype(dt)
  for p in stencil.param_stmts:
    dt = np.dtype(p.haoda_type.np_name)
    size = p.size or (1,)
    out[p.name] = (rng.random(size).astype(dt) if p.haoda_type.is_float else
                   rng.integers(-9, 10, size=size).astype(dt))
  return out


def _item(stencil, ins, i):
  return {n: (v if n in stencil.param_names else v[i]) for n, v in ins.items()}


def _same_bits(g, w):
  if g.dtype.kind == 'f':
    bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    nan = np.isnan(w)
    return (np.ascontiguousarray(g).view(bits) ==
            np.ascontiguousarray(w).view(bits)) | (nan & np.isnan(g))
  return g == w


def _oracle(stencil, ins, batch, iterate):
  from oracle import c_oracle
  orc = c_oracle.COracle(stencil, openmp=False)
  return [orc.run(_item(stencil, ins, i), iterate=iterate)
          for i in range(batch)]


def _compare(stencil, prog, extent, iterate, got, want, whole, what):
  """got: {output: (batch,) + shape}; want: per item, from the oracle."""
  names = [k.name for k in prog.module.kernels]
  for o in stencil.output_names:
    lo, hi = stencil.valid_box(extent, o, iterate)
    assert all(h > l for l, h in zip(lo, hi)), \
        'empty valid box: bad test %s' % (extent,)
    if whole:
      assert (tuple(lo), tuple(hi)) == ((0,) * stencil.dim, tuple(extent))
    idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
    for i, w in enumerate(want):
      same = _same_bits(got[o][i][idx], w[o][idx])
      assert same.all(), \
          '%s, %s on %s: %d cells of item %d of %s differ (%s)' % (
              what, stencil.app_name, tuple(extent), int((~same).sum()), i, o,
              names)


class _Device:
  """Device memory through the library's own calls."""

  def __init__(self, device=0):
    from soda_amd import runtime
    self.rt, self.lib, self.device, self.ptrs = \
        runtime, runtime.library(), device, []

  def alloc(self, nbytes, fill=None):
    p = ctypes.c_void_p()
    self.rt.check(self.lib.soda_hip_malloc(self.device, nbytes,
                                           ctypes.byref(p)), 'malloc')
    self.ptrs.append(p)
    if fill is not None:
      self.rt.check(self.lib.soda_hip_memset(p, fill, nbytes, None), 'memset')
      self.rt.check(self.lib.soda_hip_stream_synchronize(None), 'sync')
    return p.value

  def put(self, arr):
    arr = np.ascontiguousarray(arr)
    p = self.alloc(arr.nbytes)
    self.rt.check(self.lib.soda_hip_memcpy_h2d(p, arr.ctypes.data, arr.nbytes,
                                               None), 'h2d')
    return p

  def get(self, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    self.rt.check(self.lib.soda_hip_memcpy_d2h(out.ctypes.data, ptr,
                                               out.nbytes, None), 'd2h')
    return out

  def close(self):
    for p in self.ptrs:
      self.lib.soda_hip_free(self.device, p)
    self.ptrs = []


def _guarded_run(stencil, prog, extent, batch, iterate, ins):
  """The device entry on output buffers one item longer at each end, handed
  the address of the second item: ({output: (batch,) + shape}, guards ok)."""
  dev = _Device(prog.device)
  try:
    shape = tuple(extent[::-1])
    d_in = [dev.put(ins[n]) for n in stencil.input_names]
    d_in += [dev.put(ins[p.name].reshape(-1)) for p in stencil.param_stmts]
    d_out, item = [], []
    for t in stencil.output_types:
      dt = np.dtype(t.np_name)
      item.append(int(np.prod(shape)) * dt.itemsize)
      d_out.append(dev.alloc((batch + 2) * item[-1], fill=GUARD))
    prog.run_device([p + b for p, b in zip(d_out, item)], d_in, extent,
                    iterate, batch=batch)
    dev.rt.check(dev.lib.soda_hip_stream_synchronize(None), 'sync')
    got = {}
    for o, t, p in zip(stencil.output_names, stencil.output_types, d_out):
      full = dev.get(p, (batch + 2,) + shape, np.dtype(t.np_name))
      raw = full.view(np.uint8)
      assert (raw[0] == GUARD).all(), \
          '%s: the item BEFORE the batch was written' % o
      assert (raw[-1] == GUARD).all(), \
          '%s: the item BEHIND the batch was written' % o
      got[o] = full[1:-1]
    return got
  finally:
    dev.close()


def _check(stencil, prog, extent, batch, iterate=None, whole=False, seed=0,
           want_passes=()):
  """One batched run of `prog` against the C oracle run per item, through
  run_batch and through the guarded device entry."""
  iterate = stencil.iterate if iterate is None else iterate
  assert prog.plan.batched == 1
  assert all(k.name.endswith(SUFFIX) for k in prog.module.kernels)
  sched = prog.schedule(extent, iterate, batch)
  assert sum(t * c for t, c in sched.items()) == iterate, sched
  for depth in want_passes:
    assert sched.get(depth), 'pass T=%d is not scheduled: %s' % (depth, sched)
  assert not prog.pass_times(extent, batch)[1]        # never calibrated
  ins = _inputs(stencil, extent, batch, seed)
  want = _oracle(stencil, ins, batch, iterate)
  got = prog.run_batch(ins, iterate=iterate)
  _compare(stencil, prog, extent, iterate, got, want, whole, 'run_batch')
  for o in stencil.output_names:       # outside the box: zeros, as `run`
    lo, hi = stencil.valid_box(extent, o, iterate)
    mask = np.ones(got[o].shape, bool)
    mask[(slice(None),) + tuple(slice(l, h)
                                for l, h in zip(lo[::-1], hi[::-1]))] = False
    assert not got[o][mask].any()
  launches = prog.last_launches()[0]
  guarded = _guarded_run(stencil, prog, extent, batch, iterate, ins)
  _compare(stencil, prog, extent, iterate, guarded, want, whole,
           'run_device(batch)')
  # one launch per kernel of every scheduled pass, whatever the batch
  per_pass = {p.fused_iters: len(p.kernels)
              for p in prog.module.sorted_passes()}
  assert launches == prog.last_launches()[0] == \
      sum(c * per_pass[t] for t, c in sched.items())
  return sched


def _program(stencil, **kw):
  from soda_amd import runtime
  prog = runtime.Program(stencil, _opts(**kw), calibrate=False)
  assert all(k.name.endswith(SUFFIX) for k in prog.module.kernels)
  return prog


@pytest.mark.gpu
@pytest.mark.parametrize('fuse,pipe', [((13,), None), ((4,), 4)])
def test_jacobi2d_fused(built, fuse, pipe):
  """Two strips and a bit, three chunks and a ragged fourth, a fused pass and
  the remainder pass."""
  stencil = _stencil('jacobi2d.soda', iterate=15)
  with _program(stencil, fuse=fuse, chunk_rows=16, pipe=pipe) as prog:
    k = _fused(prog.module, fuse[0])
    assert ('_pipe4' in k.name) == (pipe == 4), k.name
    s = k.tile[0]
    extent = (2 * s + 36, 50)
    assert prog.geometry(extent, batch=3)[0][k.name][1] == 16
    sched = _check(stencil, prog, extent, 3, want_passes=(fuse[0], 1))
    assert sched == ({13: 1, 1: 2} if fuse == (13,) else {4: 3, 1: 3})


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['plain', 'xshare', 'xshare_block'])
def test_heat3d_two_iterations(built, form):
  stencil = _stencil('heat3d.soda', iterate=3)
  with _program(stencil, fuse=(2,)) as plain:
    k = _fused(plain.module, 2)
    s, v = k.tile[0], k.tune['vec']
  kw, tag = dict(), None
  if form == 'xshare':
    kw, tag = dict(xshare=True, row_cells=s + 9 * v), '_xs'
  elif form == 'xshare_block':
    kw, tag = dict(xshare_block=2), '_xb2'
  with _program(stencil, fuse=(2,), **kw) as prog:
    k = _fused(prog.module, 2)
    if tag:
      assert tag in k.name, k.name
    else:
      assert '_xs' not in k.name and '_xb' not in k.name, k.name
    if form == 'xshare_block':
      s = k.tile[0]
    extent = (s + 9 * v, 9, 12)
    _check(stencil, prog, extent, 3, want_passes=(2, 1))


@pytest.mark.gpu
def test_heat3d_tile3d(built):
  stencil = _stencil('heat3d.soda', iterate=4)
  with _program(stencil, strategy='tile3d', fuse=(3,)) as prog:
    assert 'tile3d' in _fused(prog.module, 3).name
    _check(stencil, prog, (100, 20, 9), 2, want_passes=(3, 1))


@pytest.mark.gpu
def test_ldswin(built):
  """One full tile and a ragged one in each dimension."""
  stencil = _stencil(LDSWIN_PROGRAM, iterate=1)
  with _program(stencil, strategy='ldswin') as prog:
    k, = prog.module.kernels
    assert 'ldswin' in k.name
    extent = (k.tile[0] + 40, k.tile[1] + 11)
    assert prog.geometry(extent, batch=2)[0][k.name][:2] == k.tile[:2]
    _check(stencil, prog, extent, 2, want_passes=(1,))


@pytest.mark.gpu
def test_direct_four_dimensions(built):
  """The item offset is the product of four extents."""
  stencil = _stencil('heat4d.soda', iterate=1)
  with _program(stencil) as prog:
    assert all('direct' in k.name for k in prog.module.kernels)
    _check(stencil, prog, (20, 6, 5, 4), 2, want_passes=(1,))


@pytest.mark.gpu
def test_direct_with_locals(built):
  """Several kernels per pass, library-owned locals sized for the batch."""
  stencil = _stencil('denoise2d.soda')
  with _program(stencil, strategy='direct') as prog:
    assert len(prog.module.kernels) > 1 and stencil.local_names
    assert all('direct' in k.name for k in prog.module.kernels)
    _check(stencil, prog, (72, 40), 3, want_passes=(1,))


@pytest.mark.gpu
def test_blur_one_shot(built):
  """uint16 cells, non-temporal stores, aligned strips.  (2 cells per lane:
  rows of 2 S + 6 cells are no multiple of the default 8.)"""
  stencil = _stencil('blur.soda')
  assert stencil.iterate == 1 and str(stencil.input_types[0]) == 'uint16'
  with _program(stencil, vec=2) as prog:
    k, = prog.module.kernels
    assert '_nts_' in k.name and '_al' in k.name, k.name
    _check(stencil, prog, (2 * k.tile[0] + 6, 37), 3, want_passes=(1,))


@pytest.mark.gpu
def test_border_preserve(built):
  stencil = _stencil('jacobi2d.soda', iterate=9, border='preserve')
  with _program(stencil, fuse=(4,)) as prog:
    _check(stencil, prog, (300, 40), 3, whole=True, want_passes=(4, 1))


@pytest.mark.gpu
def test_param_arrays_are_shared_by_all_items(built):
  stencil = _stencil('conv2d.soda')
  assert stencil.param_names
  with _program(stencil, fuse=(2,)) as prog:
    _check(stencil, prog, (264, 33), 3)


@pytest.mark.gpu
def test_one_handle_many_batch_sizes(built):
  """The scratch regrows, the (extent, batch) plans do not mix."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=9)
  extent = (300, 40)
  ins = _inputs(stencil, extent, 5, seed=3)
  want = _oracle(stencil, ins, 5, 9)
  with _program(stencil, fuse=(4,)) as prog:
    first = None
    for batch in (1, 5, 2):
      part = {n: v[:batch] for n, v in ins.items()}
      assert prog.schedule(extent, 9, batch) == {4: 2, 1: 1}
      got = prog.run_batch(part)
      _compare(stencil, prog, extent, 9, got, want[:batch], False,
               'batch %d' % batch)
      guarded = _guarded_run(stencil, prog, extent, batch, 9, part)
      _compare(stencil, prog, extent, 9, guarded, want[:batch], False,
               'guarded batch %d' % batch)
      first = got if first is None else first
    # through a one-grid entry the batched kernels run as a batch of 1
    solo = prog.run({n: v[0] for n, v in ins.items()})
    _compare(stencil, prog, extent, 9, {o: v[None] for o, v in solo.items()},
             want[:1], False, 'run on a batched program')
    times = prog.calibrate(extent, batch=5)
    assert set(times) == {4, 1} and all(v > 0 for v in times.values())
    assert prog.pass_times(extent, 5)[1]
    assert not prog.pass_times(extent, 2)[1]
    assert not prog.pass_times(extent, 1)[1]
    assert not prog.pass_times(extent)[1]
    sched = prog.schedule(extent, 9, 5)
    assert sum(t * c for t, c in sched.items()) == 9
    got = prog.run_batch(ins)
    _compare(stencil, prog, extent, 9, got, want, False, 'calibrated batch 5')
  with runtime.Program(stencil, lower.LowerOptions(fuse=(4,)),
                       calibrate=False) as plain:
    assert plain.plan.batched == 0
    one = plain.run({n: v[0] for n, v in ins.items()})
  lo, hi = stencil.valid_box(extent)
  idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
  for o in stencil.output_names:
    assert _same_bits(first[o][0][idx], one[o][idx]).all()


# programs of fuzz's plain generator that are iterated, on whose
# fuzz.extent_for rows are a multiple of the cells per lane: 2-D and 3-D,
# double / float / uint8 / int32 cells
FUZZ_SEEDS = (25, 594, 663, 1129, 434)


def test_the_fuzz_seeds_are_what_they_are_said_to_be():
  from soda_amd import core
  dims, kinds = set(), set()
  for seed in FUZZ_SEEDS:
    text, dim, _ = fuzz.program(seed)
    stencil = core.from_text(text)
    dims.add(stencil.dim)
    kinds |= {str(t) for t in stencil.input_types + stencil.output_types}
  assert dims == {2, 3}
  assert kinds & {'uint8', 'int32'}, kinds


@pytest.mark.gpu
@pytest.mark.parametrize('seed', FUZZ_SEEDS)
def test_fuzz(built, seed):
  from soda_amd import core
  text, dim, _ = fuzz.program(seed)
  stencil = core.from_text(text)
  with _program(stencil) as prog:
    _check(stencil, prog, tuple(fuzz.extent_for(seed, dim)), 2, seed=seed)


@pytest.mark.gpu
def test_an_unbatched_handle_is_refused(built):
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import lower
  stencil = _stencil('jacobi2d.soda', iterate=2)
  extent = (256, 24)
  dev = _Device()
  try:
    with runtime.Program(stencil, lower.LowerOptions(fuse=(2,)),
                         calibrate=False) as prog:
      nbytes = 2 * 256 * 24 * 4
      a = dev.alloc(nbytes, fill=0)
      b = dev.alloc(nbytes, fill=GUARD)
      prog.run_device([b], [a], extent)           # the handle itself is fine
      dev.rt.check(dev.lib.soda_hip_stream_synchronize(None), 'sync')
      before = prog.last_launches()
      dev.rt.check(dev.lib.soda_hip_memset(b, GUARD, nbytes, None), 'memset')
      with pytest.raises(util.BackendError,
                         match='invalid argument.*not batched'):
        prog.run_device([b], [a], extent, batch=2)
      assert prog.last_launches() == before
      assert (dev.get(b, (nbytes,), np.uint8) == GUARD).all()
      with pytest.raises(util.BackendError, match='not batched'):
        prog.schedule(extent, 2, batch=2)
      assert prog.schedule(extent, 2, batch=1) == prog.schedule(extent, 2)
    with _program(stencil, fuse=(2,)) as prog:
      for bad in (0, 65536):
        with pytest.raises(util.BackendError, match='invalid argument.*batch'):
          prog.run_device([b], [a], extent, batch=bad)
      # each tensor is `batch` items long: the second item of the input is
      # the first of the output
      with pytest.raises(util.BackendError, match='overlaps'):
        prog.run_device([a + nbytes // 2], [a], extent, batch=2)
      assert (dev.get(b, (nbytes,), np.uint8) == GUARD).all()
  finally:
    dev.close()
