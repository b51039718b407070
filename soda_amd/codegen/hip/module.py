"""What every kernel family of the HIP backend shares: the device runtime text,
kernel / pass descriptors and the Module a lowering fills (see lower.py)."""
import os
from typing import Dict, List, Optional, Sequence

from soda_amd import core, util

_HERE = os.path.dirname(os.path.abspath(__file__))
_RT_PATH = os.path.join(_HERE, '..', '..', 'csrc', 'soda_rt.h')
_RT_BANKED_PATH = os.path.join(_HERE, '..', '..', 'csrc', 'soda_rt_banked.h')
_RT_BATCH_PATH = os.path.join(_HERE, '..', '..', 'csrc', 'soda_rt_batch.h')
_COORDS = util.COORDS_IN_ORIG



def runtime_text() -> str:
  with open(_RT_PATH) as f:
    return f.read()


def banked_runtime_text() -> str:
  """The helpers of the banked form (soda_rt_banked.h): pasted behind
  runtime_text() into modules that address banks themselves, and only those."""
  with open(_RT_BANKED_PATH) as f:
    return f.read()


def batch_runtime_text() -> str:
  """The helpers of batched kernels (soda_rt_batch.h): pasted behind
  runtime_text() into modules lowered with LowerOptions.batch, and only those."""
  with open(_RT_BATCH_PATH) as f:
    return f.read()


# what every generated kernel's head ends in, and a batched kernel's instead
_KERNEL_ARGS = '(soda_hip_kargs_t a) {'
_BATCH_SUFFIX = '_bt'

# slots of soda_hip_kargs_t.buf a banked module may use: the last one stays
# the debug slot
BANKED_MAX_SLOTS = 15


class KernelDesc:
  """Mirror of soda_hip_kernel_desc_t."""

  def __init__(self, name: str, block: Sequence[int], tile: Sequence[int],
               lds_bytes: int = 0, note: str = '',
               tune: Optional[dict] = None):
    self.name = name
    self.block = tuple(block) + (1,) * (3 - len(block))
    self.tile = tuple(tile) + (1,) * (util.MAX_DIM - len(tile))
    self.lds_bytes = lds_bytes
    self.note = note
    # marching kernels: what the host needs to size the chunk length at load
    # time (axis, waves of a block along it, pipeline warm-up, fixed or not)
    self.tune = tune
    # LowerOptions.residual: index of the kernel's twin (the same kernel, with
    # the residual of the last fused iteration taken where it stores), or -1
    self.twin = -1


class PassDesc:
  """Mirror of soda_hip_pass_desc_t (kernel indices are into Module.kernels)."""

  def __init__(self, fused_iters: int, kernels: Sequence[int], kind: str,
               traffic_model: Optional[dict] = None):
    self.fused_iters = fused_iters
    self.kernels = list(kernels)
    self.kind = kind
    self.traffic_model = traffic_model or {}


class Module:
  """HIP source text + plan for one program at one vector width."""

  def __init__(self, stencil: core.Stencil,
               banks: Optional[Dict[str, int]] = None, batch: bool = False,
               residual: bool = False):
    self.stencil = stencil
    # LowerOptions.residual: the module also holds `<app>_residual` (its index
    # in `kernels`; residual.py) and the twins of its marching kernels
    self.residual = bool(residual)
    self.residual_kernel = -1
    self.residual_zero_kernel = -1
    # LowerOptions.batch: every kernel is emitted in its batched form
    # (add_kernel)
    self.batch = bool(batch)
    if self.batch and banks:
      raise util.SemanticError(
          'batch: the wire format has no batch, `banks` cannot be combined '
          'with it')
    self.chunks: List[str] = []
    self.kernels: List[KernelDesc] = []
    self.passes: List[PassDesc] = []
    # slots of soda_hip_kargs_t.buf: inputs, outputs, locals, param arrays
    names = list(stencil.input_names) + list(stencil.output_names) + list(
        stencil.local_names) + list(stencil.param_names)
    table = dict(stencil.symbol_table)
    table.update((p.name, p.haoda_type) for p in stencil.param_stmts)
    # the banked form of a wire stream's dense program: {input or output: NB},
    # such a tensor takes NB consecutive slots, one per bank
    self.banks = dict(banks or {})
    if not self.banks:
      self.slot = {n: i for i, n in enumerate(names)}
      self.elem_size = [table[n].size_in_bytes for n in names]
      return
    io = list(stencil.input_names) + list(stencil.output_names)
    for n, nb in self.banks.items():
      if n not in io or nb not in (2, 4):
        raise util.SemanticError(
            'banks: `%s` on %r banks: an input or output on 2 or 4' % (n, nb))
    self.slot, self.elem_size = {}, []
    for n in names:
      self.slot[n] = len(self.elem_size)
      self.elem_size += [table[n].size_in_bytes] * self.banks.get(n, 1)
    if len(self.elem_size) > BANKED_MAX_SLOTS:
      raise util.SemanticError(
          'banks: %d tensor slots (> %d)' % (len(self.elem_size),
                                             BANKED_MAX_SLOTS))

  def param_decls(self, stage: core.Stage) -> List[str]:
    """Kernel text: one pointer per param array `stage` reads."""
    ptable = self.stencil.param_table
    return ['  const %s* __restrict__ prm_%s = (const %s*)a.buf[%d];' %
            (ptable[p].haoda_type.c_type, p, ptable[p].haoda_type.c_type,
             self.slot[p]) for p in stage.params]

  def param_load(self, ref) -> Optional[str]:
    """C text of `name(i, j)` if `name` is a param array, else None."""
    ptable = self.stencil.param_table
    if ref.name not in ptable:
      return None
    return 'prm_%s[%d]' % (ref.name, self.stencil.param_index(
        ptable[ref.name], ref.idx))

  def param_var(self, v) -> str:
    """C text of a variable: a scalar param reads element 0."""
    if v.name in self.stencil.param_table and not v.idx:
      return 'prm_%s[0]' % v.name
    return v.text()

  def _batched(self, desc: KernelDesc, text: str) -> str:
    """The batched form of a kernel of any family (soda_rt_batch.h): the same
    text behind a head that takes blockIdx.y as the item and moves the slots
    of the inputs, outputs and locals -- not the param arrays' -- of a copy of
    the argument block by that many items.  The kernel's name, in `desc` too,
    gets the suffix `_bt`."""
    head = desc.name + _KERNEL_ARGS
    if text.count(head) != 1:
      raise util.InternalError('batch: kernel head of %s not found' % desc.name)
    st = self.stencil
    moved = list(st.input_names) + list(st.output_names) + list(st.local_names)
    lines = [desc.name + _BATCH_SUFFIX + '(soda_hip_kargs_t soda_a0) {',
             '  // batched: blockIdx.y is the item; the items of every tensor '
             'lie one behind the other',
             '  soda_hip_kargs_t a = soda_a0;',
             '  const int64_t soda_item = soda_batch_cells<%d>(soda_a0) * '
             '(int64_t)blockIdx.y;' % st.dim]
    for n in moved:
      lines.append('  a.buf[%d] = soda_batch_base<%d>(soda_a0.buf[%d], '
                   'soda_item);  // %s' %
                   (self.slot[n], self.elem_size[self.slot[n]], self.slot[n], n))
    desc.name += _BATCH_SUFFIX
    return text.replace(head, '\n'.join(lines))

  def add_kernel(self, desc: KernelDesc, text: str) -> int:
    if self.batch:
      text = self._batched(desc, text)
    self.kernels.append(desc)
    self.chunks.append(text)
    return len(self.kernels) - 1

  @property
  def source(self) -> str:
    head = ('// generated by soda_amd (sodac --hip-kernel) for `%s`; gfx950 only\n'
            % self.stencil.app_name)
    st = self.stencil
    types = [s.haoda_type for s in
             st.input_stmts + st.local_stmts + st.output_stmts]
    for s in st.local_stmts + st.output_stmts:
      types += [l.haoda_type for l in s.let if l.haoda_type is not None]
    text = ' '.join(str(s) for s in st.local_stmts + st.output_stmts)
    if all(t.width_in_bits <= 32 for t in types) and 'double' not in text \
        and 'int64' not in text:
      # no 64-bit arithmetic anywhere: fp32 lane shifts may fold into their
      # consumers (soda_rt.h, soda_lane_shift)
      head += '#define SODA_FOLD_F32_DPP 1\n'
    from soda_amd.codegen.hip import exact, residual
    return (head + runtime_text() +
            (banked_runtime_text() if self.banks else '') +
            (batch_runtime_text() if self.batch else '') +
            (residual.residual_runtime_text() if self.residual else '') +
            exact.helper_text(self.stencil) + '\n' + '\n'.join(self.chunks))

  def sorted_passes(self) -> List[PassDesc]:
    return sorted(self.passes, key=lambda p: -p.fused_iters)


def _check_native(stencil: core.Stencil) -> None:
  for stmt in (stencil.input_stmts + stencil.local_stmts + stencil.output_stmts
               + stencil.param_stmts):
    if not stmt.haoda_type.is_native:
      raise util.SemanticError(
          'the HIP backend runs 8/16/32/64-bit integers, float and double; '
          '`%s` is %s' % (stmt.name, stmt.haoda_type))
    for let in getattr(stmt, 'let', ()):
      if let.haoda_type is not None and not let.haoda_type.is_native:
        raise util.SemanticError('let `%s` has unsupported type %s' %
                                 (let.name, let.haoda_type))


