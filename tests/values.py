"""Inputs from the whole value domain (shared by the CPU and GPU tests of
tests/test_values.py, imported like fuzz.py).

tests/fuzz.py feeds the random programs floats in [0.25, 2) and integers in
[0, 200]: no sign, no zero, nothing tiny, nothing huge.  The classes here fill
the rest of the domain, seeded and per input tensor:

  full       integers, uniform over the whole range of the type, about 5 % of
             the cells from {min, max, 0, 1, -1 (signed) / max - 1 (unsigned)}
  signed     floats, uniform in [-2, 2] with |x| >= 0.25 (the magnitudes of
             fuzz.inputs_for, so the float -> int32 casts of the rich generator
             stay in range), about 1 % +0.0 and 1 % -0.0
  tiny       `signed` with half of the cells scaled by 2^(minexp - nmant + k),
             k in 0..29, of the tensor's own type: subnormals and the normals
             just above them
  nonfinite  `signed` plus exactly six cells +inf, -inf, NaN, +inf, -inf, NaN,
             at the coordinates `at` or placed by the seed

An integer tensor is `full` in every class and a float tensor is `signed` in
class `full`, so one class name serves a whole program.  `same_bits` is the
comparison that goes with them: it tells -0.0 from +0.0, which
np.array_equal(..., equal_nan=True) does not."""
import re

import numpy as np

INT_CLASSES = ('full',)
FLOAT_CLASSES = ('signed', 'tiny', 'nonfinite')
NONFINITE = (np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan)


def classes_for(stencil, text=None):
  """The classes a program is run in: `full` for integer inputs; the three
  float classes otherwise -- without `nonfinite` where the program's `text`
  casts a float to an integer (undefined in C for inf / NaN; x86 and the GPU
  differ)."""
  if not any(t.is_float for t in stencil.input_types):
    return INT_CLASSES
  if text is not None and casts_to_integer(text):
    return FLOAT_CLASSES[:2]
  return FLOAT_CLASSES


def casts_to_integer(text):
  return re.search(r'\bu?int(8|16|32|64)\s*\(', text) is not None


def _signed(rng, shape, dt):
  x = rng.uniform(0.25, 2.0, shape)
  x = np.where(rng.random(shape) < 0.5, -x, x).astype(dt)
  r = rng.random(shape)
  x[r < 0.01] = 0.0
  x[(r >= 0.01) & (r < 0.02)] = -0.0
  return x


def _tiny(rng, shape, dt):
  x = _signed(rng, shape, dt)
  info = np.finfo(dt)
  e = info.minexp - info.nmant + rng.integers(0, 30, shape)
  return np.where(rng.random(shape) < 0.5, np.ldexp(x, e), x).astype(dt)


def _full(rng, shape, dt):
  info = np.iinfo(dt)
  x = rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
  edges = np.array([info.min, info.max, 0, 1,
                    -1 if info.min < 0 else info.max - 1], dtype=dt)
  pick = rng.random(shape) < 0.05
  x[pick] = rng.choice(edges, int(pick.sum()))
  # ... and each of them once for certain, whatever the draw
  flat = x.reshape(-1)
  flat[rng.choice(flat.size, len(edges), replace=False)] = edges
  return x


def params_for(stencil, seed):
  """Small values, as tests/test_batch.py draws them."""
  rng = np.random.default_rng(seed + 5151)
  out = {}
  for p in stencil.param_stmts:
    dt = np.dtype(p.haoda_type.np_name)
    size = p.size or (1,)
    out[p.name] = (rng.random(size).astype(dt) if p.haoda_type.is_float else
                   rng.integers(-9, 10, size=size).astype(dt))
  return out


def edge_inputs(stencil, extent, seed, kind, at=None):
  """{name: array shaped extent[::-1]} for the inputs and param arrays of
  `stencil`.  `at`: six coordinates (x, y[, z]) for the non-finite cells of
  every float tensor, in the order of NONFINITE."""
  assert kind in INT_CLASSES + FLOAT_CLASSES, kind
  rng = np.random.default_rng(seed + 6363)
  shape = tuple(extent[::-1])
  out = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    dt = np.dtype(t.np_name)
    if not t.is_float:
      out[name] = _full(rng, shape, dt)
      continue
    if kind == 'tiny':
      out[name] = _tiny(rng, shape, dt)
      continue
    x = _signed(rng, shape, dt)
    if kind == 'nonfinite':
      if at is None:
        flat = rng.choice(x.size, len(NONFINITE), replace=False)
        cells = [np.unravel_index(int(i), shape) for i in flat]
      else:
        cells = [tuple(c[::-1]) for c in at]
        assert len(set(cells)) == len(NONFINITE), at
      for c, v in zip(cells, NONFINITE):
        x[c] = v
    out[name] = x
  out.update(params_for(stencil, seed))
  return out


def nonfinite_cells(a):
  """[(x, y[, z])] of the cells of `a` that are not finite, in C order."""
  return [tuple(int(i) for i in c[::-1]) for c in np.argwhere(~np.isfinite(a))]


def same_bits(got, want):
  """Elementwise: integers by ==; floats by bit pattern, two NaNs counted
  equal whatever their sign and payload (those are the machine's).  -0.0 is
  not +0.0; infinities, subnormals and everything finite are exact."""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.dtype == want.dtype and got.shape == want.shape
  if got.dtype.kind != 'f':
    return got == want
  bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
  return (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))


def nan_share(a):
  """The share of NaN cells of `a` (0 for integers and for no cell at all)."""
  if a.dtype.kind != 'f' or not a.size:
    return 0.0
  return float(np.isnan(a).mean())


def special_values(dtype):
  """The operands of the operator tables, in the type's own precision."""
  dt = np.dtype(dtype)
  if dt.kind == 'f':
    info = np.finfo(dt)
    sub = float(info.smallest_subnormal)
    norm = float(info.smallest_normal)
    root = 2.0 ** (-96 if dt.itemsize == 4 else -767)   # hipcc's sqrt scales
    big = float(info.max)
    mags = [0.0, sub, 3 * sub, norm - sub, norm, 1.5 * norm, root, 2.0 ** -63,
            1e-3, 0.25, 1.0, 1.5, 2.0, 3.0, 1e3, big / 4, big, np.inf]
    return np.array([s * m for m in mags for s in (1.0, -1.0)] + [np.nan],
                    dtype=dt)
  info = np.iinfo(dt)
  lo, hi = int(info.min), int(info.max)
  vals = [lo, lo + 1, lo + 2, hi, hi - 1, hi - 2, 0, 1, -1, 2, -2, 3, -3, 7, -7,
          100, -100, 127, 128, -128, -129, 255, hi // 2, hi // 2 + 1, hi // 3,
          lo // 2, lo // 3]
  kept = []
  for v in vals:
    if lo <= v <= hi and v not in kept:
      kept.append(v)
  return np.array(kept, dtype=dt)


def table_inputs(stencil, extent, dtype=None):
  """a[y, x] = S[x % n], b[y, x] = S[y % n] (a third tensor: S[(x + y) % n]),
  S = special_values of the tensor's type (or of `dtype`): every ordered pair
  of special values meets in every two-tensor operator, on any grid of at
  least n valid cells each way."""
  shape = tuple(extent[::-1])
  idx = np.indices(shape)
  x, y = idx[-1], idx[-2]
  out = {}
  for i, (name, t) in enumerate(zip(stencil.input_names, stencil.input_types)):
    s = special_values(dtype or t.np_name)
    sel = (x, y, x + y)[min(i, 2)]
    out[name] = np.ascontiguousarray(s[sel % len(s)].astype(np.dtype(t.np_name)))
  out.update(params_for(stencil, 0))
  return out
