"""Residual of a run's last iteration (LowerOptions.residual):
what the option means for a module, the generic `<app>_residual` kernel, and
the recurrence the library derives the counted cells from.

Over the last iteration of a run of N iterations every output `o` pairs with
the input `i` it replaces -- `zip(input_names, output_names)`, under `border:
preserve` that is `preserved_from` -- `cur` is `o` after N iterations, `prev`
that input as the last iteration saw it.  The marching kernels get twins
(march.py, names ending in `_rs`) that take the delta where they store; every
other family, and a marching depth without a twin, is served by the kernel
built here from two dense arrays per pair."""
import os
from typing import Dict, List, Tuple

from soda_amd import core, util

from soda_amd.codegen.hip.module import KernelDesc, Module

_HERE = os.path.dirname(os.path.abspath(__file__))
_RT_RESIDUAL_PATH = os.path.join(_HERE, '..', '..', 'csrc', 'soda_rt_residual.h')

TWIN_SUFFIX = '_rs'
# what a twin's head ends in, and the generic kernel's
RESIDUAL_ARGS = ('(soda_hip_kargs_t a, soda_hip_residual_t* soda_res, '
                 'soda_hip_resbox_t soda_box) {')
MAX_PAIRS = 8          # SODA_HIP_MAX_RES_PAIRS (include/soda_hip.h)
NONE = -(1 << 30)      # SODA_HIP_RES_NONE: this output does not depend on that input
RESIDUAL_BLOCK = 256


def residual_runtime_text() -> str:
  """The helpers of residual kernels (soda_rt_residual.h): pasted behind
  runtime_text() into modules lowered with LowerOptions.residual, and only
  those."""
  with open(_RT_RESIDUAL_PATH) as f:
    return f.read()


def residual_supported(stencil: core.Stencil) -> str:
  """'' if `residual` can be built for the program, else why not."""
  if len(stencil.input_names) != len(stencil.output_names) or \
      list(stencil.input_types) != list(stencil.output_types):
    return ('residual compares every output with the input it replaces: the '
            'program must be iterable (as many outputs as inputs, of the same '
            'types)')
  if len(stencil.output_names) > MAX_PAIRS:
    return 'residual handles up to %d input / output pairs' % MAX_PAIRS
  return ''


def pairs(stencil: core.Stencil) -> List[Tuple[str, str]]:
  """(input, output) of every pair, in slot order."""
  return list(zip(stencil.input_names, stencil.output_names))


def box_recurrence(stencil: core.Stencil) -> Dict[str, object]:
  """What the library needs to know the valid box of every output after any
  number of iterations (core.Stencil.valid_box) without the program text.
  One iteration maps the bounds of its inputs' windows to those of its
  outputs' (core.iteration_boxes); per dimension that map is

      lo(o) = min(base_lo(o), min over inputs i of dep_lo(o, i) + min(lo(i), 0))

  and the same with max for `hi`: taps only add constants, and a window
  always includes the loaded cell itself.  `base` is the map's value on
  inputs of window zero; `dep(o, i)` is found by moving input i's bound far
  out and reading how far the output's follows (NONE: it does not).
  `whole` (border: preserve): the box is the whole array."""
  dim = stencil.dim
  ins, outs = list(stencil.input_names), list(stencil.output_names)
  base = stencil.iteration_boxes()
  far = 1 << 20
  dep_lo = [[[NONE] * 4 for _ in ins] for _ in outs]
  dep_hi = [[[NONE] * 4 for _ in ins] for _ in outs]
  for k, i in enumerate(ins):
    moved = stencil.iteration_boxes(
        {i: ((-far,) * dim, (far,) * dim)})
    for j, o in enumerate(outs):
      for d in range(dim):
        if moved[o][0][d] < -far // 2:
          dep_lo[j][k][d] = moved[o][0][d] + far
        if moved[o][1][d] > far // 2:
          dep_hi[j][k][d] = moved[o][1][d] - far
  return dict(
      whole=bool(stencil.preserve_border),
      base_lo=[list(base[o][0]) + [0] * (4 - dim) for o in outs],
      base_hi=[list(base[o][1]) + [0] * (4 - dim) for o in outs],
      dep_lo=dep_lo, dep_hi=dep_hi)


def window_after(rec: Dict[str, object], dim: int, iterate: int):
  """The recurrence run `iterate` times, as the library runs it: [(lo, hi)]
  per output, bounds relative to the program inputs (core.window_bounds)."""
  n = len(rec['base_lo'])
  lo = [[0] * dim for _ in range(n)]
  hi = [[0] * dim for _ in range(n)]
  for _ in range(iterate):
    nlo = [list(rec['base_lo'][o][:dim]) for o in range(n)]
    nhi = [list(rec['base_hi'][o][:dim]) for o in range(n)]
    for o in range(n):
      for i in range(n):
        for d in range(dim):
          if rec['dep_lo'][o][i][d] != NONE:
            nlo[o][d] = min(nlo[o][d], rec['dep_lo'][o][i][d] + min(lo[i][d], 0))
          if rec['dep_hi'][o][i][d] != NONE:
            nhi[o][d] = max(nhi[o][d], rec['dep_hi'][o][i][d] + max(hi[i][d], 0))
    lo, hi = nlo, nhi
  return [(tuple(l), tuple(h)) for l, h in zip(lo, hi)]


def add_residual_kernel(mod: Module) -> int:
  """Adds `<app>_residual`: dense `cur` (the output slots) and `prev` (the
  input slots) of every pair, the cells of `soda_box` counted.  A thread
  reads fragments of `vec` cells -- the widest cells-per-lane of the module's
  kernels, so up to 16 bytes, aligned by the device entry contract, and rows
  are a whole number of them.  A block owns one segment of 256 fragments of a
  row and strides over the rows of arrays of 1 to 4 dimensions (no division
  per fragment: the library launches a whole number of rows' worth of
  blocks), and ends in the reduction tail of every residual kernel."""
  st = mod.stencil
  table = st.symbol_table
  vec = 1
  for k in mod.kernels:
    vec = max(vec, int((k.tune or {}).get('vec') or 1))
  name = '%s_residual' % st.app_name
  seg = RESIDUAL_BLOCK * vec
  L = ['// residual of the last iteration over dense arrays: %d pair(s), %d '
       'cells per thread and row' % (len(pairs(st)), vec),
       '// grid: (segments of %d cells a row has) x (rows in flight); block b '
       'takes segment b %% nx of rows b / nx, b / nx + gridDim.x / nx, ...' % seg,
       'extern "C" __global__ void __launch_bounds__(%d) %s%s' %
       (RESIDUAL_BLOCK, name, RESIDUAL_ARGS),
       '  soda_res_lane_t soda_acc;',
       '  soda_res_init(soda_acc);',
       '  const unsigned nx = ((unsigned)a.extent[0] + %du) / %du;' %
       (seg - 1, seg),
       '  const unsigned xc = blockIdx.x % nx, r0 = blockIdx.x / nx, '
       'rstep = gridDim.x / nx;',
       '  const int x = (int)((xc * %du + threadIdx.x) * %du);' %
       (RESIDUAL_BLOCK, vec),
       '  // (a row is a whole number of fragments: in or out as a whole)',
       '  const bool x_in = x < a.extent[0];',
       '  unsigned rows = 1u;',
       '  for (int d = 1; d < %d; ++d) rows *= (unsigned)a.extent[d];' % st.dim,
       '  for (unsigned row = r0; row < rows; row += rstep) {']
  if st.dim > 1:
    L.append('    unsigned rest = row;')
  for d in range(1, st.dim):
    if d < st.dim - 1:
      L.append('    const int q%d = (int)(rest %% (unsigned)a.extent[%d]); rest '
               '/= (unsigned)a.extent[%d];' % (d, d, d))
    else:
      L.append('    const int q%d = (int)rest;' % d)
  L += ['    const int64_t c = (int64_t)row * a.extent[0] + x;',
        '    if (x_in) {']
  for p, (i, o) in enumerate(pairs(st)):
    ct = table[o].c_type
    rows = ' && '.join('q%d >= soda_box.lo[%d][%d] && q%d < soda_box.hi[%d][%d]'
                       % (d, p, d, d, p, d) for d in range(1, st.dim)) or 'true'
    L += ['      {  // %s against %s' % (o, i),
          '        %s cur[%d], prev[%d];' % (ct, vec, vec),
          '        soda_load_frag<%s, %d, false>(cur, (const %s*)a.buf[%d] + c);'
          % (ct, vec, ct, mod.slot[o]),
          '        soda_load_frag<%s, %d, false>(prev, (const %s*)a.buf[%d] + c);'
          % (ct, vec, ct, mod.slot[i]),
          '        const bool rows_ok = %s;' % rows,
          '        _Pragma("unroll") for (int e = 0; e < %d; ++e)' % vec,
          '          soda_res_add(soda_acc, cur[e], prev[e], rows_ok && x + e >= '
          'soda_box.lo[%d][0] && x + e < soda_box.hi[%d][0]);' % (p, p),
          '      }']
  L += ['    }',
        '  }',
        '  soda_res_flush(soda_acc, soda_res);',
        '}']
  desc = KernelDesc(name, (RESIDUAL_BLOCK, 1, 1),
                    (RESIDUAL_BLOCK * vec,) + (1,) * (st.dim - 1),
                    note='residual V%d' % vec, tune=dict(vec=vec))
  mod.kernels.append(desc)
  mod.chunks.append('\n'.join(L) + '\n')
  mod.residual_kernel = len(mod.kernels) - 1
  # ... and the kernel that zeroes the struct at the head of a residual run,
  # on the run's own stream: a kernel node like the passes behind it, so a
  # captured call zeroes at every replay (a 32-byte memset node did not: see
  # DESIGN.md 4.9)
  zero = '%s_residual_zero' % st.app_name
  mod.kernels.append(KernelDesc(zero, (64, 1, 1), (64,) + (1,) * (st.dim - 1),
                                note='residual: zero the struct'))
  mod.chunks.append('\n'.join([
      'extern "C" __global__ void __launch_bounds__(64) %s(soda_hip_residual_t* '
      'soda_res) {' % zero,
      '  if (threadIdx.x < 4u) ((unsigned long long*)soda_res)[threadIdx.x] = '
      '0ull;',
      '}']) + '\n')
  mod.residual_zero_kernel = len(mod.kernels) - 1
  return mod.residual_kernel


def check_options(stencil: core.Stencil, batch: bool, banks) -> None:
  """SemanticError, naming the option, for what `residual` is refused with."""
  why = residual_supported(stencil)
  if why:
    raise util.SemanticError('residual: %s' % why)
  if batch:
    raise util.SemanticError(
        'residual: not together with `batch` (a residual per item of a batch '
        'is a reduction of its own)')
  if banks:
    raise util.SemanticError(
        'residual: not together with `banks` (the wire format\'s banked '
        'tensors are not dense arrays to compare)')
