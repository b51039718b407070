"""The device entry between guard bands.

`Program.run` hands the library host arrays; the library allocates the device
arrays itself and copies back the valid box only, so nothing a kernel writes
outside the box -- or outside the array: allocations are rounded up, a store a
few cells past the end faults nothing -- and nothing it reads outside its
inputs is ever seen.  Here every tensor of a `run_device` call lies in ONE
device allocation (the arena), apart from its neighbours by guards:

  guard | lead | input 0 | guard | lead | ... params ... | outputs ... | guard

* a guard is at least 4096 bytes and at least two rows of the larger
  neighbouring tensor (a plane and a row for 3-D and 4-D programs), rounded to
  16 bytes;
* tensor k starts `leads[k]` bytes behind its guard: multiples of 16 that are
  not multiples of 64 by default, so every address is 16-byte aligned and no
  tensor sits where an allocator would put it;
* before the run the inputs and the param arrays hold their data, every guard
  next to one of them holds 0xFF bytes (a NaN in both float types, -1 or the
  maximum in the integer types: a kernel that READS a guard cell cannot give a
  finite result from it unnoticed), every other guard and the output arrays
  hold 0xA5.

`run` uploads the arena, calls `prog.run_device`, synchronises, downloads the
whole arena and returns the outputs with `check(before, after, layout)`: the
first byte that changed outside the output arrays -- in a guard, in an input,
in a param array -- or None.  `check` is plain numpy on the two byte images.
"""
import collections
import ctypes

import numpy as np

GUARD_MIN = 4096
FILL_READ = 0xFF       # guards next to an input or a param array
FILL_WRITE = 0xA5      # the other guards and the output arrays
DEFAULT_LEADS = (16, 48, 80, 112)      # taken in turn

Tensor = collections.namedtuple(
    'Tensor', 'name role dtype shape start nbytes row_bytes')
Guard = collections.namedtuple('Guard', 'start nbytes fill')
Layout = collections.namedtuple('Layout', 'tensors guards nbytes dim')
# region: 'before' / 'behind' (a guard byte, named by the nearer tensor),
# 'input', 'param'; offset: bytes from the tensor's first byte (negative
# before it); row, column: that position in rows of the tensor's row length
# (row = the number of rows: the first row behind the array)
Violation = collections.namedtuple(
    'Violation', 'region tensor offset row column changed')


def _round_up(n, to):
  return -(-n // to) * to


def tensors_of(stencil, extent):
  """[(name, role, dtype, shape)] of a call: the inputs, the param arrays (C
  order, flat), then the outputs."""
  shape = tuple(int(e) for e in extent[::-1])
  out = [(n, 'input', np.dtype(t.np_name), shape)
         for n, t in zip(stencil.input_names, stencil.input_types)]
  for p in stencil.param_stmts:
    out.append((p.name, 'param', np.dtype(p.haoda_type.np_name),
                (int(stencil.param_elems(p)),)))
  out += [(n, 'output', np.dtype(t.np_name), shape)
          for n, t in zip(stencil.output_names, stencil.output_types)]
  return out


def guard_bytes(dim, tensor):
  """The least guard next to `tensor` (a (dtype, shape) pair)."""
  dtype, shape = tensor
  row = shape[-1] * dtype.itemsize
  need = 2 * row
  if dim >= 3 and len(shape) >= 2:
    need = shape[-2] * row + row
  return _round_up(max(GUARD_MIN, need), 16)


def layout(stencil, extent, leads=None):
  leads = DEFAULT_LEADS if leads is None else tuple(leads)
  items = tensors_of(stencil, extent)
  tensors, guards = [], []
  end = 0
  for k, (name, role, dtype, shape) in enumerate(items):
    need = guard_bytes(stencil.dim, (dtype, shape))
    if k:
      need = max(need, guard_bytes(stencil.dim, items[k - 1][2:]))
    start = _round_up(end + need, 64) + int(leads[k % len(leads)])
    read = role != 'output' or (k and items[k - 1][1] != 'output')
    guards.append(Guard(end, start - end, FILL_READ if read else FILL_WRITE))
    nbytes = int(np.prod(shape)) * dtype.itemsize
    tensors.append(Tensor(name, role, dtype, shape, start, nbytes,
                          shape[-1] * dtype.itemsize))
    end = start + nbytes
  last = guard_bytes(stencil.dim, items[-1][2:])
  total = _round_up(end + last, 16)
  guards.append(Guard(end, total - end, FILL_READ
                      if items[-1][1] != 'output' else FILL_WRITE))
  return Layout(tuple(tensors), tuple(guards), total, stencil.dim)


def image(lay, ins):
  """The arena's bytes before the run."""
  img = np.empty(lay.nbytes, np.uint8)
  for g in lay.guards:
    img[g.start:g.start + g.nbytes] = g.fill
  for t in lay.tensors:
    if t.role == 'output':
      img[t.start:t.start + t.nbytes] = FILL_WRITE
      continue
    arr = np.ascontiguousarray(ins[t.name]).reshape(t.shape)
    assert arr.dtype == t.dtype, (t.name, arr.dtype, t.dtype)
    img[t.start:t.start + t.nbytes] = arr.reshape(-1).view(np.uint8)
  return img


def read(lay, img, name):
  t, = [t for t in lay.tensors if t.name == name]
  return img[t.start:t.start + t.nbytes].view(t.dtype).reshape(t.shape).copy()


def check(before, after, lay):
  """The first byte of the arena that differs between the two images outside
  the output arrays, as a Violation (with the number of such bytes), or
  None."""
  assert before.dtype == after.dtype == np.uint8
  assert before.shape == after.shape == (lay.nbytes,)
  diff = before != after
  for t in lay.tensors:
    if t.role == 'output':
      diff[t.start:t.start + t.nbytes] = False
  at = np.flatnonzero(diff)
  if not at.size:
    return None
  b = int(at[0])
  region, near = None, None
  for t in lay.tensors:
    if t.start <= b < t.start + t.nbytes:
      region, near = t.role, t
  if near is None:
    ahead = [t for t in lay.tensors if t.start > b]
    back = [t for t in lay.tensors if t.start + t.nbytes <= b]
    if ahead and (not back or
                  ahead[0].start - b <= b - (back[-1].start + back[-1].nbytes) + 1):
      region, near = 'before', ahead[0]
    else:
      region, near = 'behind', back[-1]
  off = b - near.start
  return Violation(region, near.name, off, off // near.row_bytes,
                   (off % near.row_bytes) // near.dtype.itemsize, int(at.size))


class Arena:
  """The layout's bytes on the device `prog` runs on."""

  def __init__(self, prog, lay, ins):
    from soda_amd import runtime
    self.lay, self.device = lay, prog.device
    self.before = image(lay, ins)
    self._lib = runtime.library()
    self._ptr = ctypes.c_void_p()
    runtime.check(self._lib.soda_hip_malloc(self.device, lay.nbytes,
                                            ctypes.byref(self._ptr)),
                  'arena: malloc')
    try:
      runtime.check(self._lib.soda_hip_memcpy_h2d(
          self._ptr, self.before.ctypes.data, lay.nbytes, None), 'arena: h2d')
      self.sync()
    except Exception:
      self.close()
      raise

  @property
  def base(self):
    return self._ptr.value

  def address(self, name):
    t, = [t for t in self.lay.tensors if t.name == name]
    return self.base + t.start

  def inputs(self):
    return [self.base + t.start for t in self.lay.tensors
            if t.role != 'output']

  def outputs(self):
    return [self.base + t.start for t in self.lay.tensors
            if t.role == 'output']

  def sync(self):
    from soda_amd import runtime
    runtime.check(self._lib.soda_hip_stream_synchronize(None), 'arena: sync')

  def download(self):
    from soda_amd import runtime
    self.sync()
    after = np.empty(self.lay.nbytes, np.uint8)
    runtime.check(self._lib.soda_hip_memcpy_d2h(
        after.ctypes.data, self._ptr, self.lay.nbytes, None), 'arena: d2h')
    return after

  def close(self):
    if self._ptr:
      self._lib.soda_hip_free(self.device, self._ptr)
      self._ptr = ctypes.c_void_p()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


def run(prog, stencil, extent, ins, iterate=None, leads=None,
        **run_device_kw):
  """({output: array}, Violation or None, (before, after, layout))."""
  lay = layout(stencil, extent, leads)
  with Arena(prog, lay, ins) as arena:
    assert arena.base % 64 == 0
    prog.run_device(arena.outputs(), arena.inputs(), extent, iterate,
                    **run_device_kw)
    after = arena.download()
    before = arena.before
  got = {t.name: read(lay, after, t.name) for t in lay.tensors
         if t.role == 'output'}
  return got, check(before, after, lay), (before, after, lay)
