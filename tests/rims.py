"""What tests/test_border_fused.py shares: the geometry of a fused bordered run
 emulated on the host from the numbers of the plan alone.

Nothing here runs the code under test.  A chunk of n iterations is
  interior  the existing oracle for n iterations on the open box of the padded
            state (np.pad by the plan's frame); every cell outside the
            oracle's valid box is then SPOILED (its bits inverted), so that a
            cell the scatter does not mend cannot pass by accident;
  strips    per strip of the plan the domain's cells [0, L) and [N - H, N)
            along its dimension side by side, advanced n iterations as a
            bordered domain of their own (tests/borders.py `expected`);
  scatter   the strip's cells [0, take_lo) and [L + H - take_hi, L + H) over
            the interior's result.
The result is compared with borders.expected on the whole domain."""
import numpy as np

import borders


def _axis(arr, d):
  return arr.ndim - 1 - d


def _cut(arr, d, lo, hi):
  idx = [slice(None)] * arr.ndim
  idx[_axis(arr, d)] = slice(lo, hi)
  return tuple(idx)


def spoil_outside(arr, lo, hi):
  """Inverts the bits of every cell outside the box [lo, hi) (dimension 0
  first), in place."""
  keep = np.zeros(arr.shape, bool)
  keep[tuple(slice(max(0, l), max(0, h)) for l, h in zip(lo[::-1], hi[::-1]))] \
      = True
  bits = arr.view(np.dtype('u%d' % arr.dtype.itemsize))
  bits[~keep] = ~bits[~keep]


def strip_inputs(stencil, state, strip):
  """The strip's inputs: the two rims of every input of `state` side by side
  along the strip's dimension; param arrays as they are."""
  d, L, H = strip['dim'], strip['lo'], strip['hi']
  out = dict(state)
  for name in stencil.input_names:
    a = state[name]
    n = a.shape[_axis(a, d)]
    out[name] = np.ascontiguousarray(np.concatenate(
        [a[_cut(a, d, 0, L)], a[_cut(a, d, n - H, n)]], axis=_axis(a, d)))
    assert out[name].shape[::-1] == tuple(strip['extent'])
  return out


def scatter(stencil, result, strip, strip_out):
  d, L, H = strip['dim'], strip['lo'], strip['hi']
  tl, th = strip['take_lo'], strip['take_hi']
  for o in stencil.output_names:
    a, s = result[o], strip_out[o]
    n = a.shape[_axis(a, d)]
    a[_cut(a, d, 0, tl)] = s[_cut(s, d, 0, tl)]
    a[_cut(a, d, n - th, n)] = s[_cut(s, d, L + H - th, L + H)]


def emulate(stencil, ins, modes, constants, info, chunks):
  """{output: array of the domain} after sum(chunks) iterations by the scheme,
  from `info` and `chunks` of runtime.border_fused_plan."""
  from oracle import numpy_oracle
  cst = borders.constants_of(stencil, constants)
  lo, hi = info['ghost_lo'], info['ghost_hi']
  shape = ins[stencil.input_names[0]].shape
  cut = tuple(slice(l, l + n) for l, n in zip(lo[::-1], shape))
  state = dict(ins)
  result = {}
  for n in chunks:
    assert 1 <= n <= info['depth']
    padded = dict(state)
    for name in stencil.input_names:
      padded[name] = borders.pad(state[name], lo, hi, modes, cst[name])
    extent = padded[stencil.input_names[0]].shape[::-1]
    assert tuple(extent) == tuple(info['padded'])
    open_box = numpy_oracle.run(stencil, padded, iterate=n)
    result = {}
    for o in stencil.output_names:
      whole = np.array(open_box[o], copy=True)
      vlo, vhi = stencil.valid_box(extent, o, n)
      spoil_outside(whole, vlo, vhi)
      result[o] = np.ascontiguousarray(whole[cut])
    for strip in info['strips']:
      sins = strip_inputs(stencil, state, strip)
      scatter(stencil, result, strip,
              borders.expected(stencil, sins, n, modes, constants))
    for i, o in zip(stencil.input_names, stencil.output_names):
      state[i] = result[o]
  return result
