"""What tests/test_border.py shares: np.pad under a border mode per dimension,
the closed forms of the modes, the expected value of a bordered run.

The expected value never uses the code under test.  For EVERY iteration each
input is padded on the host, axis by axis, with np.pad in the numpy mode of the
dimension's border mode by what ONE iteration reaches
(Stencil.window_bounds(1), the most over all outputs); the existing oracle runs
one iteration on that open box; the domain is cut out -- the oracle's valid
box holds it, by the choice of the pad -- and output o becomes input o of the
next iteration.

Nothing here needs a GPU (device arrays: tests/periodic.py's Device)."""
import numpy as np

import periodic

# border mode -> numpy's name
NUMPY = {'wrap': 'wrap', 'clamp': 'edge', 'mirror': 'symmetric',
         'mirror101': 'reflect', 'constant': 'constant'}
MODES = sorted(NUMPY)


def per_dim(modes, dim):
  return [modes] * dim if isinstance(modes, str) else list(modes)


def index_map(mode, n, lo, hi):
  """The closed form: for padded index i = 0 .. lo + n + hi - 1 the cell of
  [0, n) it takes, -1 for none (`constant`, outside)."""
  j = np.arange(-lo, n + hi)
  if mode == 'wrap':
    return j % n
  if mode == 'clamp':
    return np.clip(j, 0, n - 1)
  if mode == 'mirror':
    t = j % (2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)
  if mode == 'mirror101':
    if n == 1:
      return np.zeros_like(j)
    t = j % (2 * n - 2)
    return np.where(t < n, t, 2 * n - 2 - t)
  assert mode == 'constant', mode
  return np.where((j < 0) | (j >= n), -1, j)


def closed_form(arr, lo, hi, modes, constant=0):
  """`arr` extended by the closed forms, separably: a cell outside in any
  `constant` dimension takes the constant."""
  modes = per_dim(modes, arr.ndim)
  out = arr
  outside = np.zeros((), bool)
  for axis in range(arr.ndim):
    d = arr.ndim - 1 - axis
    m = index_map(modes[d], arr.shape[axis], int(lo[d]), int(hi[d]))
    out = np.take(out, np.maximum(m, 0), axis=axis)
    shape = [1] * arr.ndim
    shape[axis] = len(m)
    outside = outside | (m < 0).reshape(shape)
  out = np.array(out, copy=True)
  out[np.broadcast_to(outside, out.shape)] = np.asarray(constant).astype(
      arr.dtype)
  return np.ascontiguousarray(out)


def pad(arr, lo, hi, modes, constant=0):
  """np.pad axis by axis (dimension 0, the LAST axis, first) in the numpy mode
  of each dimension -- checked against the closed forms, so that a pad wider
  than the array is known to bounce more than once."""
  modes = per_dim(modes, arr.ndim)
  out = arr
  for d in range(arr.ndim):
    width = [(0, 0)] * arr.ndim
    width[arr.ndim - 1 - d] = (int(lo[d]), int(hi[d]))
    kw = {}
    if modes[d] == 'constant':
      kw['constant_values'] = np.asarray(constant).astype(arr.dtype)
    out = np.pad(out, width, mode=NUMPY[modes[d]], **kw)
  form = closed_form(arr, lo, hi, modes, constant)
  assert out.shape == form.shape and \
      np.ascontiguousarray(out).tobytes() == form.tobytes()
  return np.ascontiguousarray(out)


def constants_of(stencil, constants):
  """{input: scalar} from None, a scalar or a dict."""
  if constants is None:
    constants = 0
  if not isinstance(constants, dict):
    constants = {n: constants for n in stencil.input_names}
  return {n: constants.get(n, 0) for n in stencil.input_names}


def expected(stencil, ins, iterate, modes, constants=None, run=None):
  """{output: array of the domain} after `iterate` bordered iterations, by
  np.pad and the oracle (`run`: default oracle.numpy_oracle.run)."""
  if run is None:
    from oracle import numpy_oracle
    run = lambda st, padded, it: numpy_oracle.run(st, padded, iterate=it)
  cst = constants_of(stencil, constants)
  lo, hi = periodic.reach(stencil, 1)
  shape = ins[stencil.input_names[0]].shape
  cut = tuple(slice(l, l + n) for l, n in zip(lo[::-1], shape))
  state = dict(ins)
  out = {}
  for _ in range(iterate):
    padded = dict(state)
    for n in stencil.input_names:
      padded[n] = pad(state[n], lo, hi, modes, cst[n])
    extent = padded[stencil.input_names[0]].shape[::-1]
    want = run(stencil, padded, 1)
    out = {}
    for o in stencil.output_names:
      vlo, vhi = stencil.valid_box(extent, o, 1)
      # the domain lies in the oracle's valid box
      assert all(a <= l and l + n <= b for a, b, l, n in
                 zip(vlo, vhi, lo, shape[::-1])), (o, vlo, vhi, lo, shape)
      out[o] = np.ascontiguousarray(want[o][cut])
    for i, o in zip(stencil.input_names, stencil.output_names):
      state[i] = out[o]
  return out
