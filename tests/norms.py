"""What tests/test_norms.py shares: the oracle of the exact L1 / L2 norms in
Python integers, the comparison of a soda_hip_norms_t with it word by word,
planted arrays, and device memory by hand.

The oracle forms the deltas with numpy in the cell's dtype (one IEEE operation
for floats, as tests/test_residual.py does), takes every finite one apart with
`np.frexp` into an integer mantissa and an exponent, sums mantissas and their
squares per exponent and combines the sums as Python `int`: no floating-point
addition anywhere.  Nothing here needs a GPU."""
import ctypes
import fractions

import numpy as np

KIND_F32, KIND_F64, KIND_I32, KIND_I64 = 1, 2, 3, 4
UNITS = {KIND_F32: (-149, -298), KIND_F64: (-1074, -2148), KIND_I32: (0, 0),
         KIND_I64: (0, 0)}
L1_WORDS, L2_WORDS = 34, 67

C_TYPE = {'float32': 'float', 'float64': 'double'}


def c_type(dtype):
  dtype = np.dtype(dtype)
  return C_TYPE.get(dtype.name, dtype.name + '_t')


def kind_of(dtype):
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return KIND_F32 if dtype.itemsize == 4 else KIND_F64
  return KIND_I32 if dtype.itemsize < 8 else KIND_I64


def _scaled(mant, exp, unit):
  """mant x 2^exp in units of 2^unit, which it is a whole number of."""
  shift = exp - unit
  if shift >= 0:
    return mant << shift
  assert mant % (1 << -shift) == 0, (mant, exp, unit)
  return mant >> -shift


def empty(dtype):
  return dict(kind=kind_of(dtype), count=0, unordered=0, infinite=0, l1=0, l2=0)


def oracle(cur, prev, into=None):
  """The norms of `cur` against `prev` (arrays of one dtype and shape: the
  cells counted, already cut out) as a dict of Python ints, added to `into`."""
  cur, prev = np.asarray(cur), np.asarray(prev)
  assert cur.dtype == prev.dtype and cur.shape == prev.shape
  out = dict(into) if into is not None else empty(cur.dtype)
  assert out['kind'] == kind_of(cur.dtype)
  u1, u2 = UNITS[out['kind']]
  if cur.size == 0:
    return out
  if cur.dtype.kind == 'f':
    with np.errstate(all='ignore'):
      d = np.abs(cur - prev)              # one IEEE operation in the cell's type
    assert d.dtype == cur.dtype
    nan, inf = np.isnan(d), np.isinf(d)
    out['unordered'] += int(nan.sum())
    out['infinite'] += int(inf.sum())
    fin = d[~nan & ~inf].astype(np.float64)     # exact for both types
    out['count'] += int(fin.size)
    m, e = np.frexp(fin)                  # fin = m x 2^e, 0.5 <= m < 1 or m = 0
    mant = np.ldexp(m, 53).astype(np.int64)     # a whole number below 2^53
    assert (np.ldexp(mant.astype(np.float64), e - 53) == fin).all()
    for ex in np.unique(e):
      ms = [int(v) for v in mant[e == ex]]
      out['l1'] += _scaled(sum(ms), int(ex) - 53, u1)
      out['l2'] += _scaled(sum(v * v for v in ms), 2 * (int(ex) - 53), u2)
    return out
  a = [int(v) for v in cur.reshape(-1)]
  b = [int(v) for v in prev.reshape(-1)]
  ds = [abs(x - y) for x, y in zip(a, b)]
  out['count'] += len(ds)
  out['l1'] += sum(ds)
  out['l2'] += sum(v * v for v in ds)
  return out


def words(value, n):
  assert 0 <= value < 1 << (64 * n), 'the sum does not fit the struct'
  return [(value >> (64 * i)) & 0xffffffffffffffff for i in range(n)]


def fields(acc):
  """A NormsStruct as the oracle's dict, the sums word by word."""
  return dict(kind=int(acc.kind), count=int(acc.count),
              unordered=int(acc.unordered), infinite=int(acc.infinite),
              l1=[int(w) for w in acc.l1], l2=[int(w) for w in acc.l2])


def expected_fields(want):
  return dict(want, l1=words(want['l1'], L1_WORDS),
              l2=words(want['l2'], L2_WORDS))


def same(acc, want):
  """`==` on the counts and on every word of both sums."""
  got, exp = fields(acc), expected_fields(want)
  assert got == exp, {k: (got[k], exp[k]) for k in got if got[k] != exp[k]}
  assert int(acc.reserved) == 0
  return True


def expected_value(want, which):
  """The correctly rounded double of a sum, by fractions.Fraction."""
  if want['infinite']:
    return float('inf')
  unit = UNITS[want['kind']][0 if which == 'l1' else 1]
  try:
    return float(fractions.Fraction(want[which]) * fractions.Fraction(2) ** unit)
  except OverflowError:
    return float('inf')


def cut(arr, lo, hi):
  """The cells [lo, hi) -- dimension 0, the fastest, first -- of a numpy array
  (slowest dimension first)."""
  return arr[tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]]


def random_pair(rng, shape, dtype, spread=8):
  """Two arrays whose deltas span `spread` binary orders (floats) or the whole
  range (integers)."""
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    prev = rng.standard_normal(shape).astype(dtype)
    step = np.ldexp(rng.standard_normal(shape),
                    rng.integers(-spread, spread + 1, shape)).astype(dtype)
    return (prev + step).astype(dtype), prev
  info = np.iinfo(dtype)
  cur = rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
  prev = rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
  return cur, prev


class Device:
  """Device memory by hand (the library's own malloc / memcpy), freed on exit."""

  def __init__(self, device=0):
    from soda_amd import runtime
    self.rt, self.lib, self.device, self.ptrs = runtime, runtime.library(), \
        device, []

  def alloc(self, nbytes, fill=None):
    ptr = ctypes.c_void_p()
    self.rt.check(self.lib.soda_hip_malloc(self.device, max(int(nbytes), 16),
                                           ctypes.byref(ptr)), 'malloc')
    self.ptrs.append(ptr)
    if fill is not None:
      self.rt.check(self.lib.soda_hip_memset(ptr, fill, int(nbytes), None),
                    'memset')
      self.sync()
    return ptr.value

  def upload(self, arr):
    arr = np.ascontiguousarray(arr)
    ptr = self.alloc(arr.nbytes)
    self.write(ptr, arr)
    return ptr

  def write(self, ptr, arr):
    arr = np.ascontiguousarray(arr)
    self.rt.check(self.lib.soda_hip_memcpy_h2d(ctypes.c_void_p(ptr),
                                               arr.ctypes.data, arr.nbytes,
                                               None), 'h2d')
    self.sync()

  def download(self, ptr, shape, dtype):
    out = np.empty(shape, dtype)
    self.sync()
    self.rt.check(self.lib.soda_hip_memcpy_d2h(out.ctypes.data,
                                               ctypes.c_void_p(ptr),
                                               out.nbytes, None), 'd2h')
    return out

  def sync(self):
    self.rt.check(self.lib.soda_hip_stream_synchronize(None), 'sync')

  def close(self):
    for p in self.ptrs:
      self.lib.soda_hip_free(self.device, p)
    self.ptrs = []

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()
