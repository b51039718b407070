"""What tests/test_periodic.py shares: inputs, the expected value of a run on a
torus, padded views, device arrays.

The expected value never uses the code under test.  Each input is padded ONCE
on the host with np.pad(mode='wrap') by everything `iterate` iterations reach
(Stencil.window_bounds(iterate), the most over all outputs); the existing
oracle runs all `iterate` iterations on that open box; the cells that
correspond to the torus are cut out.  The oracle's valid box after `iterate`
iterations holds them all, by the choice of the pad.

Nothing here needs a GPU until `Device` is used."""
import ctypes

import numpy as np


def reach(stencil, iterate):
  """(lo, hi): cells `iterate` iterations reach below / above a cell, the most
  over all outputs, per dimension (dimension 0 first)."""
  boxes = stencil.window_bounds(iterate)
  dim = stencil.dim
  lo = [max(0, max(-boxes[o][0][d] for o in stencil.output_names))
        for d in range(dim)]
  hi = [max(0, max(boxes[o][1][d] for o in stencil.output_names))
        for d in range(dim)]
  return lo, hi


def wrap_pad(arr, lo, hi):
  """np.pad(mode='wrap') by `lo` / `hi` cells (dimension 0, the LAST axis,
  first) -- checked against the closed form a[(i - lo) mod n] per axis, so
  that a pad wider than the array is known to wrap more than once."""
  width = [(int(l), int(h)) for l, h in zip(lo, hi)][::-1]
  out = np.pad(arr, width, mode='wrap')
  form = arr
  for axis, (l, h) in enumerate(width):
    n = arr.shape[axis]
    form = np.take(form, np.arange(-l, n + h) % n, axis=axis)
  assert out.shape == form.shape and \
      out.tobytes() == np.ascontiguousarray(form).tobytes()
  return np.ascontiguousarray(out)


def inputs(stencil, extent, seed=0):
  """Finite inputs that raise no NaN: small integers in float cells,
  full-range integers in integer cells; param arrays small."""
  rng = np.random.default_rng(seed)
  shape = tuple(extent[::-1])
  out = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if t.is_float:
      out[name] = rng.integers(-8, 9, size=shape).astype(dt)
    else:
      info = np.iinfo(dt)
      out[name] = rng.integers(info.min, int(info.max) + 1, size=shape,
                               dtype=np.int64 if dt != np.uint64 else
                               np.uint64).astype(dt)
  for p in stencil.param_stmts:
    dt = np.dtype(p.haoda_type.np_name)
    out[p.name] = rng.integers(-3, 4, size=p.size or (1,)).astype(dt)
  return out


def expected(stencil, ins, iterate, run=None):
  """{output: array of the torus} by the padded oracle (`run`: the oracle's
  run function, default oracle.numpy_oracle.run)."""
  if run is None:
    from oracle import numpy_oracle
    run = lambda st, padded, it: numpy_oracle.run(st, padded, iterate=it)
  lo, hi = reach(stencil, iterate)
  padded = dict(ins)
  for n in stencil.input_names:
    padded[n] = wrap_pad(ins[n], lo, hi)
  shape = ins[stencil.input_names[0]].shape
  extent = padded[stencil.input_names[0]].shape[::-1]
  want = run(stencil, padded, iterate)
  cut = tuple(slice(l, l + n) for l, n in zip(lo[::-1], shape))
  out = {}
  for o in stencil.output_names:
    vlo, vhi = stencil.valid_box(extent, o, iterate)
    # the torus lies in the oracle's valid box
    assert all(a <= l and l + n <= b for a, b, l, n in
               zip(vlo, vhi, lo, shape[::-1])), (o, vlo, vhi, lo, shape)
    out[o] = np.ascontiguousarray(want[o][cut])
  return out


def same_bits(got, want):
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  return got.dtype == want.dtype and got.shape == want.shape and \
      got.tobytes() == want.tobytes()


def differing(got, want):
  """Number of cells whose bit patterns differ (for messages)."""
  g = np.ascontiguousarray(got).reshape(-1).view(np.uint8)
  w = np.ascontiguousarray(want).reshape(-1).view(np.uint8)
  size = got.dtype.itemsize
  return int((g.reshape(-1, size) != w.reshape(-1, size)).any(axis=1).sum())


def interior(arr, info):
  """The torus inside a padded array (a view)."""
  idx = tuple(slice(l, arr.shape[a] - h) for a, (l, h) in enumerate(
      zip(info['ghost_lo'][::-1], info['ghost_hi'][::-1])))
  return arr[idx]


class Device:
  """numpy arrays on the device a program runs on, through the library's own
  memory calls; freed on exit."""

  def __init__(self, prog):
    from soda_amd import runtime
    self._rt, self._lib, self.device = runtime, runtime.library(), prog.device
    self._ptrs = []

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self._lib.soda_hip_stream_synchronize(None)
    for p in self._ptrs:
      self._lib.soda_hip_free(self.device, p)
    self._ptrs = []

  def alloc(self, nbytes):
    ptr = ctypes.c_void_p()
    self._rt.check(self._lib.soda_hip_malloc(self.device, max(1, nbytes),
                                             ctypes.byref(ptr)), 'malloc')
    self._ptrs.append(ptr)
    return ptr.value

  def upload(self, arr):
    arr = np.ascontiguousarray(arr)
    ptr = self.alloc(arr.nbytes)
    self.write(ptr, arr)
    return ptr

  def write(self, ptr, arr):
    arr = np.ascontiguousarray(arr)
    self._rt.check(self._lib.soda_hip_memcpy_h2d(
        ctypes.c_void_p(ptr), arr.ctypes.data, arr.nbytes, None), 'h2d')

  def download(self, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    self._rt.check(self._lib.soda_hip_memcpy_d2h(
        out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes, None), 'd2h')
    return out
