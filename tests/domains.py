"""What tests/test_domain_residual.py shares: the residual and the exact norms
of the last iteration on a torus or a bordered domain, from
the existing oracles; the partition of a fused bordered domain painted and
emulated; device runs of the padded entries.

The expected numbers never use the code under test: `cur` and `prev` are
tests/periodic.py's or tests/borders.py's `expected` at n and at n - 1 (the
inputs when n = 1), the per-cell delta is formed here in numpy in the cell's
dtype, the norms by tests/norms.py's integer oracle.  All N cells of every
pair are counted.  Nothing here needs a GPU until `Run` is used."""
import ctypes

import numpy as np

import borders
import norms
import periodic
import rims

_PAIRS = {}


def delta(cur, prev):
  """(changed, unordered, max_float, max_int) of two arrays of one dtype: the
  definition of soda_hip_residual_t."""
  assert cur.dtype == prev.dtype and cur.shape == prev.shape
  if cur.size == 0:
    return 0, 0, 0.0, 0
  if cur.dtype.kind == 'f':
    with np.errstate(all='ignore'):
      d = np.abs(cur - prev)            # one IEEE operation in the cell's type
    assert d.dtype == cur.dtype
    nan = np.isnan(d)
    ordered = d[~nan]
    return (int(np.count_nonzero(~(d == 0))), int(nan.sum()),
            float(ordered.max()) if ordered.size else 0.0, 0)
  if cur.dtype.itemsize < 8:
    d = np.abs(cur.astype(np.int64) - prev.astype(np.int64))
  else:
    hi, lo = np.maximum(cur, prev), np.minimum(cur, prev)
    d = hi.astype(np.uint64) - lo.astype(np.uint64)    # wraps to the exact value
  return int(np.count_nonzero(d)), 0, 0.0, int(d.max())


def fold(parts):
  """Residual tuples combined: counts add, maxima take the larger."""
  changed = unordered = max_int = 0
  max_float = 0.0
  for c, u, f, m in parts:
    changed, unordered = changed + c, unordered + u
    max_float, max_int = max(max_float, f), max(max_int, m)
  return changed, unordered, max_float, max_int


def states(stencil, ins, iterate, modes=None, constants=None, key=None):
  """(cur, prev): {output: array of the domain} after `iterate` iterations and
  {output: array} after iterate - 1 (the paired inputs when iterate = 1) --
  on a torus (`modes` None) or between walls.  `key`: remembered under it."""
  def at(n):
    k = (key, n, str(modes), str(constants))
    if key is not None and k in _PAIRS:
      return _PAIRS[k]
    if n == 0:
      out = {o: np.asarray(ins[i]) for i, o in zip(stencil.input_names,
                                                   stencil.output_names)}
    elif modes is None:
      out = periodic.expected(stencil, ins, n)
    else:
      out = borders.expected(stencil, ins, n, modes, constants)
    if key is not None:
      _PAIRS[k] = out
    return out
  return at(iterate), at(iterate - 1)


def residual_of(stencil, cur, prev):
  return fold(delta(cur[o], prev[o]) for o in stencil.output_names)


def norms_of(stencil, cur, prev):
  acc = None
  for o in stencil.output_names:
    acc = norms.oracle(cur[o], prev[o], acc)
  return acc


def fields(res):
  return (res.changed, res.unordered, res.max_float, res.max_int)


def raw_fields(raw):
  """The 32 bytes of a soda_hip_residual_t (4 uint64) as the tuple above."""
  raw = np.asarray(raw).view(np.uint64)
  return (int(raw[0]), int(raw[1]), float(raw[2:3].view(np.float64)[0]),
          int(raw[3]))


# -- the partition of a fused bordered domain ---------------------------------

def _slices(lo, hi):
  return tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]


def domain_boxes(boxes, info, extent):
  """The boxes of runtime.border_fused_residual_boxes moved back to the
  coordinates of the domain: [(what, lo, hi)]; `info` of border_fused_plan."""
  g = info['ghost_lo']
  lo, hi = boxes['trusted']
  out = [('trusted', [l - a for l, a in zip(lo, g)],
          [h - a for h, a in zip(hi, g)])]
  assert len(boxes['strips']) == len(info['strips'])
  for rim, strip in zip(boxes['strips'], info['strips']):
    d = strip['dim']
    assert rim['dim'] == d
    sg = strip['ghost_lo']
    for side in ('low', 'high'):
      lo = [l - a for l, a in zip(rim[side][0], sg)]
      hi = [h - a for h, a in zip(rim[side][1], sg)]
      if side == 'high':           # the strip's high part sits at the far wall
        shift = extent[d] - (strip['lo'] + strip['hi'])
        lo[d], hi[d] = lo[d] + shift, hi[d] + shift
      out.append(('strip %d %s' % (d, side), lo, hi))
  return out


def paint(boxes, info, extent):
  """How often each cell of the domain lies in a box."""
  count = np.zeros(tuple(extent[::-1]), np.int32)
  for what, lo, hi in domain_boxes(boxes, info, extent):
    assert all(0 <= l and h <= n for l, h, n in zip(lo, hi, extent)), (
        what, lo, hi)
    count[_slices(lo, hi)] += 1
  return count


def emulate(stencil, ins, modes, constants, info, boxes, chunks):
  """(residual tuple, norms dict) of the LAST chunk of a fused bordered run by
  the scheme, from the plan's numbers alone, in the manner of rims.emulate:
  the interior as open-box iterations on the padded state with everything
  outside the oracle's valid box spoiled, counted over the trusted box; every
  strip as a bordered run of its own, counted over its two rims."""
  from oracle import numpy_oracle
  cst = borders.constants_of(stencil, constants)
  before = sum(chunks[:-1])
  n = chunks[-1]
  pairs = list(zip(stencil.input_names, stencil.output_names))
  state = dict(ins)
  if before:
    got = borders.expected(stencil, ins, before, modes, constants)
    for i, o in pairs:
      state[i] = got[o]
  lo, hi = info['ghost_lo'], info['ghost_hi']
  padded = dict(state)
  for name in stencil.input_names:
    padded[name] = borders.pad(state[name], lo, hi, modes, cst[name])
  extent = padded[stencil.input_names[0]].shape[::-1]

  def open_box(k):
    if k == 0:
      return {o: padded[i] for i, o in pairs}
    run = numpy_oracle.run(stencil, padded, iterate=k)
    out = {}
    for o in stencil.output_names:
      whole = np.array(run[o], copy=True)
      rims.spoil_outside(whole, *stencil.valid_box(extent, o, k))
      out[o] = whole
    return out
  parts, acc = [], None
  cur, prev = open_box(n), open_box(n - 1)
  box = _slices(*boxes['trusted'])
  for o in stencil.output_names:
    parts.append(delta(cur[o][box], prev[o][box]))
    acc = norms.oracle(cur[o][box], prev[o][box], acc)
  for rim, strip in zip(boxes['strips'], info['strips']):
    sins = rims.strip_inputs(stencil, state, strip)
    cur = borders.expected(stencil, sins, n, modes, constants)
    prev = borders.expected(stencil, sins, n - 1, modes, constants) \
        if n > 1 else {o: sins[i] for i, o in pairs}
    sg = strip['ghost_lo']
    for side in ('low', 'high'):
      box = _slices([l - a for l, a in zip(rim[side][0], sg)],
                    [h - a for h, a in zip(rim[side][1], sg)])
      for o in stencil.output_names:
        parts.append(delta(cur[o][box], prev[o][box]))
        acc = norms.oracle(cur[o][box], prev[o][box], acc)
  return fold(parts), acc


# -- device runs ----------------------------------------------------------------

def extended(stencil, ins, info, modes, constants):
  """{input: padded array}: `ins` extended by the frame of `info`."""
  lo, hi = info['ghost_lo'], info['ghost_hi']
  cst = borders.constants_of(stencil, constants)
  out = dict(ins)
  for n in stencil.input_names:
    out[n] = periodic.wrap_pad(ins[n], lo, hi) if modes is None else \
        borders.pad(ins[n], lo, hi, modes, cst[n])
  return out


class Run:
  """The padded entries of one handle on device copies of extended inputs:
  `plain`, `residual` and `norms` runs of `iterate` iterations, each into
  outputs of its own; everything freed on exit."""

  def __init__(self, prog, handle, ins, modes=None, constants=None):
    from soda_amd import runtime
    self.prog, self.handle, self.st = prog, handle, prog.stencil
    self.info = handle.info()
    self.start = extended(self.st, ins, self.info, modes, constants)
    self.shape = self.start[self.st.input_names[0]].shape
    assert self.shape == tuple(self.info['padded'][::-1])
    self.dev = periodic.Device(prog)
    self.d_in = [self.dev.upload(self.start[n]) for n in self.st.input_names] \
        + [self.dev.upload(np.ascontiguousarray(ins[p.name]).reshape(-1))
           for p in self.st.param_stmts]
    self.res = self.dev.alloc(32)
    self.acc = self.dev.alloc(ctypes.sizeof(runtime.NormsStruct))

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.dev.__exit__(*exc)

  def _outs(self):
    cells = int(np.prod(self.shape))
    return [self.dev.alloc(cells * np.dtype(t.np_name).itemsize)
            for t in self.st.output_types]

  def _fetch(self, ptrs):
    return {n: self.dev.download(p, self.shape, np.dtype(t.np_name))
            for n, p, t in zip(self.st.output_names, ptrs,
                               self.st.output_types)}

  def inputs_now(self):
    return {n: self.dev.download(p, self.shape, self.start[n].dtype)
            for n, p in zip(self.st.input_names, self.d_in)}

  def plain(self, iterate):
    outs = self._outs()
    self.handle.run_padded(outs, self.d_in, iterate)
    return self._fetch(outs)

  def residual(self, iterate):
    """(padded outputs, Residual)."""
    outs = self._outs()
    self.dev.write(self.res, np.full(32, 0xA5, np.uint8))
    self.handle.run_padded(outs, self.d_in, iterate, residual=self.res)
    return self._fetch(outs), self.prog.residual(self.res)

  def norms(self, iterate):
    """(padded outputs, NormsStruct)."""
    outs = self._outs()
    self.dev.write(self.acc, np.full(840, 0xA5, np.uint8))
    self.handle.run_padded(outs, self.d_in, iterate, norms=self.acc)
    return self._fetch(outs), self.prog.norms().fetch(self.acc)

  def interior(self, padded):
    return {o: np.ascontiguousarray(periodic.interior(a, self.info))
            for o, a in padded.items()}
