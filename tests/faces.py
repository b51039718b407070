"""What tests/test_border_faces.py shares: np.pad under a border mode per FACE
and a constant per (dimension, side), and the expected value of a run on such
a domain.

The expected arrays share nothing with the product.  For each dimension,
dimension 0 (the LAST numpy axis) first, the low part is
np.pad(a, (g_lo, 0), mode_lo)[:g_lo] and the high part
np.pad(a, (0, g_hi), mode_hi)[-g_hi:], both taken from the array as it stood
before that dimension and concatenated around it.  Programs are advanced one
iteration at a time on re-extended inputs, as tests/borders.expected does for
symmetric modes.

Nothing here needs a GPU."""
import numpy as np

import borders
import periodic

WALLS = ['clamp', 'mirror', 'mirror101', 'constant']
# all 16 pairs of the four wall modes, and the one pair `wrap` comes in
PAIRS = [(a, b) for a in WALLS for b in WALLS] + [('wrap', 'wrap')]


def pair_of(entry):
  if isinstance(entry, str):
    return tuple(entry.split('/')) if '/' in entry else (entry, entry)
  return tuple(entry)


def pairs(modes, dim):
  """[(low, high)] per dimension of `modes` in any of its spellings."""
  return [pair_of(m) for m in
          ([modes] * dim if isinstance(modes, str) else list(modes))]


def table(constants, dim):
  """[(low, high)] per dimension from a scalar or a sequence of scalars and
  pairs."""
  if not isinstance(constants, (list, tuple)):
    return [(constants, constants)] * dim
  assert len(constants) == dim
  return [tuple(c) if isinstance(c, (list, tuple)) else (c, c)
          for c in constants]


def _side(arr, axis, width, mode, constant, low):
  if not width:
    index = [slice(None)] * arr.ndim
    index[axis] = slice(0, 0)
    return arr[tuple(index)]
  widths = [(0, 0)] * arr.ndim
  widths[axis] = (width, 0) if low else (0, width)
  kw = {}
  if mode == 'constant':
    kw['constant_values'] = np.asarray(constant).astype(arr.dtype)
  out = np.pad(arr, widths, mode=borders.NUMPY[mode], **kw)
  index = [slice(None)] * arr.ndim
  index[axis] = slice(0, width) if low else slice(out.shape[axis] - width,
                                                  None)
  return out[tuple(index)]


def pad(arr, lo, hi, modes, constants=0):
  """`arr` extended by `lo` / `hi` ghost cells per dimension under a mode per
  face and a constant per (dimension, side)."""
  dim = arr.ndim
  faces, cst = pairs(modes, dim), table(constants, dim)
  out = arr
  for d in range(dim):
    axis = dim - 1 - d
    low = _side(out, axis, int(lo[d]), faces[d][0], cst[d][0], True)
    high = _side(out, axis, int(hi[d]), faces[d][1], cst[d][1], False)
    out = np.concatenate([low, out, high], axis=axis)
  return np.ascontiguousarray(out)


def constants_of(stencil, constants):
  """{input: scalar or per-face sequence} from None, either, or a dict."""
  if constants is None:
    constants = 0
  if not isinstance(constants, dict):
    constants = {n: constants for n in stencil.input_names}
  return {n: constants.get(n, 0) for n in stencil.input_names}


def expected(stencil, ins, iterate, modes, constants=None, run=None):
  """{output: array of the domain} after `iterate` iterations, every one on
  inputs extended by `pad` over what one iteration reaches (`run`: default
  oracle.numpy_oracle.run)."""
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
      assert all(a <= l and l + n <= b for a, b, l, n in
                 zip(vlo, vhi, lo, shape[::-1])), (o, vlo, vhi, lo, shape)
      out[o] = np.ascontiguousarray(want[o][cut])
    for i, o in zip(stencil.input_names, stencil.output_names):
      state[i] = out[o]
  return out
