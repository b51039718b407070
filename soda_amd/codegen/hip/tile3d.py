"""`tile3d`: LDS-tiled 3-D kernels that fuse more than two iterations.

`march3d` keeps a tile of rows x planes per tensor per fused iteration in
REGISTERS: two iterations of heat3d already need 260 VGPRs
(march_schedule.py, MAX_FUSE_3D).  Here the planes live in LDS (3.5-D blocking):

  * a block of W waves owns a tile of TX x TY cells in (x, y) -- ghost cells
    included -- and marches along dimension 2 in chunks, one plane per step;
  * every tensor of the T-times chained program that somebody reads -- the
    inputs, every fused level's locals and outputs but the last level's -- keeps
    a ring of planes of the tile in LDS: as many planes as its consumers reach
    back along z, plus the one being written;
  * the levels are SKEWED: a stage computes, in step t, plane t - delay of its
    tensor from planes its parents finished in EARLIER steps (delay = the
    latest parent's delay + its highest tap along z + 1), so the plane a step
    writes is never one the step reads and ONE block barrier per step orders
    everything: what a step wrote is read from the next step on, and the slot
    the next step overwrites is the one whose last reader ran before the
    barrier;
  * lane l of a wave owns column x = l (+ 64 c for tiles wider than 64), a wave
    owns TY / W consecutive rows: a tap is one `ds_read_b32` whose address is
    the thread's own cell plus a CONSTANT -- consecutive lanes read consecutive
    banks (conflict-free whatever the pitch), taps shared by a thread's rows
    are read once -- and a result is one `ds_write_b32`;
  * a ring's planes carry guard rows / columns as wide as the taps reach, so no
    tap needs a bounds test: every thread computes every cell of its rows at
    every level, the cells of the ghost zone (whose taps reach the guards or
    a neighbour's territory) hold garbage nobody valid reads -- the
    recomputation rule of the marching kernels: the valid part of a tile
    shrinks by the program's reach per fused level, neighbouring tiles and
    chunks overlap by that much;
  * input plane t + 1 travels from global memory into registers while step t
    computes, and is filed into its ring at the top of step t + 1;
  * the last level's outputs go from registers to global memory, masked to
    the valid part of the tile, the grid and the chunk by the buffer
    addressing of soda_rt.h -- no wave ever leaves the step loop early.

The expression text is the one the other families emit (ir.c_expr), operands
replaced by LDS reads: with -ffp-contract=off the bits of the oracle.
"""
from typing import Dict, List, Optional, Tuple

from soda_amd import core, ir, util

from soda_amd.codegen.hip.module import KernelDesc, Module, PassDesc

LDS_MAX = 160 * 1024        # per block (MI355X_MICROARCH.md: per CU)
LDS_TWO_BLOCKS = LDS_MAX // 2
TILE_W = 64                 # cells along x (one per lane)
TILE_HEIGHTS = (32, 24, 16, 12, 8, 4)
CHUNK = 128                 # planes per block and launch
CELL_TYPES = ('float', 'int32', 'uint32')


def tile3d_supported(stencil: core.Stencil) -> Optional[str]:
  """None if the tile3d kernels can run the program, else why not."""
  if stencil.dim != 3:
    return 'tile3d needs a 3-dimensional program (this one has %d)' % \
        stencil.dim
  if stencil.preserve_border:
    return 'tile3d does not handle border: preserve'
  if stencil.param_stmts:
    return 'tile3d does not handle param arrays'
  if len(stencil.input_names) != len(stencil.output_names) or \
      list(stencil.input_types) != list(stencil.output_types):
    return ('tile3d fuses iterations: the program must be iterable (as many '
            'outputs as inputs, of the same types)')
  for name, t in stencil.symbol_table.items():
    if str(t) not in CELL_TYPES:
      return 'tile3d handles float, int32 and uint32 cells; `%s` is %s' % (
          name, t)
  return None


class _Node:
  """A tensor of the T-times chained program."""

  def __init__(self, var: str, ctype: str, stage: Optional[core.Stage]):
    self.var = var
    self.ctype = ctype
    self.stage = stage                  # None: a program input
    self.parents: Dict[str, '_Node'] = {}
    self.delay = 0          # step t computes (files) plane t - delay
    self.margin = [[0, 0], [0, 0]]      # invalid cells low / high in x, y
    self.need = None        # planes (lo, hi), relative to an output plane,
    #                         that output plane depends on; None: dead
    self.store: Optional[str] = None    # last level: the output it is
    self.ring = 0           # planes in LDS (0: not kept)
    self.guard = [[0, 0], [0, 0]]       # guard cells low / high in x, y
    self.pitch = self.rows = self.plane = 0


def _chain(st: core.Stencil, T: int) -> List[_Node]:
  table = st.symbol_table
  nodes: List[_Node] = []
  env: Dict[str, _Node] = {}
  for name in st.input_names:
    env[name] = _Node('g_%s' % name, table[name].c_type, None)
    nodes.append(env[name])
  for it in range(T):
    for stage in st.ordered_stages:
      n = _Node('t%d_%s' % (it, stage.name), stage.haoda_type.c_type, stage)
      for pname in stage.taps:
        n.parents[pname] = env[pname]
      env[stage.name] = n
      nodes.append(n)
    if it == T - 1:
      for o in st.output_names:
        env[o].store = o
    else:
      env.update({i: env[o]
                  for i, o in zip(st.input_names, st.output_names)})
  # skewed delays and ghost margins, in chain order
  for n in nodes:
    if n.stage is None:
      continue
    delay = None
    for pname, p in n.parents.items():
      tlo, thi = n.stage.tap_bounds(pname)
      d = p.delay + thi[2] + 1
      delay = d if delay is None else max(delay, d)
      for a in (0, 1):
        n.margin[a][0] = max(n.margin[a][0], p.margin[a][0] + max(0, -tlo[a]))
        n.margin[a][1] = max(n.margin[a][1], p.margin[a][1] + max(0, thi[a]))
    n.delay = delay or 0
  # what the stored planes depend on, back to front
  for n in nodes:
    if n.store is not None:
      n.need = (0, 0)
  for n in reversed(nodes):
    if n.need is None or n.stage is None:
      continue
    for pname, p in n.parents.items():
      tlo, thi = n.stage.tap_bounds(pname)
      lo, hi = n.need[0] + tlo[2], n.need[1] + thi[2]
      p.need = (lo, hi) if p.need is None else (min(p.need[0], lo),
                                                max(p.need[1], hi))
  nodes = [n for n in nodes if n.need is not None]
  for n in nodes:
    if n.stage is None:
      continue
    for pname, p in n.parents.items():
      tlo, thi = n.stage.tap_bounds(pname)
      # planes from the one `p` writes this step back to the oldest `n` reads
      p.ring = max(p.ring, n.delay - tlo[2] - p.delay + 1)
      for a in (0, 1):
        p.guard[a][0] = max(p.guard[a][0], -tlo[a])
        p.guard[a][1] = max(p.guard[a][1], thi[a])
  return nodes


class _Tile3dKernel:

  def __init__(self, mod: Module, fused_iters: int, tile_w: Optional[int],
               tile_h: Optional[int], waves: Optional[int], chunk: int,
               nt_load: bool, nt_store: bool, xcd_swizzle: bool):
    self.mod, self.st, self.T = mod, mod.stencil, fused_iters
    why = tile3d_supported(self.st)
    if why:
      raise util.SemanticError('tile3d: %s' % why)
    if self.T < 1:
      raise util.SemanticError('tile3d: fusion depth %d' % self.T)
    self.TX = TILE_W if tile_w is None else int(tile_w)
    if self.TX < 64 or self.TX % 64:
      raise util.SemanticError('tile3d: the tile width is a multiple of 64 '
                               'cells (one column per lane), not %d' % self.TX)
    self.CX = self.TX // 64
    self.nodes = _chain(self.st, self.T)
    self.stored = [n for n in self.nodes if n.store is not None]
    self.mx = [max(n.margin[0][s] for n in self.stored) for s in (0, 1)]
    self.my = [max(n.margin[1][s] for n in self.stored) for s in (0, 1)]
    self.VX = self.TX - self.mx[0] - self.mx[1]
    if self.VX < 1:
      raise util.SemanticError(
          'tile3d: %d fused iterations reach %d+%d cells along x, a tile of '
          '%d cells has no valid part' % (self.T, self.mx[0], self.mx[1],
                                          self.TX))
    # tile height.  Asked for: taken (if its rings fit LDS at all).  Else the
    # tallest height whose rings leave room for two blocks per CU and whose
    # valid rows are at least a third of the tile (below that the ghost rows
    # cost more than the second block hides); else the tallest that fits.
    heights = (int(tile_h),) if tile_h is not None else TILE_HEIGHTS
    fits = [h for h in heights if h - self.my[0] - self.my[1] >= 1]
    if not fits:
      raise util.SemanticError(
          'tile3d: %d fused iterations reach %d+%d rows along y, a tile of %d '
          'rows has no valid part' % (self.T, self.my[0], self.my[1],
                                      max(heights)))
    sized = [(h, self._lds_bytes(h)) for h in fits]
    two = [h for h, b in sized if b <= LDS_TWO_BLOCKS and
           3 * (h - self.my[0] - self.my[1]) >= h]
    one = [h for h, b in sized if b <= LDS_MAX]
    if not one:
      raise util.SemanticError(
          'tile3d: the plane rings of %d fused iterations need %d bytes of '
          'LDS for the smallest tile (%d x %d cells); a block has %d' %
          (self.T, min(b for _, b in sized), self.TX,
           min(h for h, _ in sized), LDS_MAX))
    self.TY = max(two) if two else max(one)
    self.lds_bytes = self._lds_bytes(self.TY)
    self.VY = self.TY - self.my[0] - self.my[1]
    if waves is None:
      waves = max(w for w in (8, 4, 2, 1) if self.TY % w == 0)
    self.W = int(waves)
    if self.W < 1 or self.W > 16 or self.TY % self.W:
      raise util.SemanticError('tile3d: %d waves do not divide a tile of %d '
                               'rows (1 to 16 waves)' % (self.W, self.TY))
    self.RY = self.TY // self.W
    for n in self.nodes:
      n.pitch = n.guard[0][0] + self.TX + n.guard[0][1]
      n.rows = n.guard[1][0] + self.TY + n.guard[1][1]
      n.plane = n.pitch * n.rows
    self.chunk = int(chunk)
    self.nt_l = 'true' if nt_load else 'false'
    self.nt_s = 'true' if nt_store else 'false'
    self.xcd = xcd_swizzle
    self.inputs = [n for n in self.nodes if n.stage is None]
    # planes of the inputs a chunk's output planes depend on, relative to them
    self.m_lo = min([0] + [n.need[0] for n in self.inputs])
    self.m_hi = max([0] + [n.need[1] for n in self.inputs])
    # first step of a chunk: the earliest at which a plane somebody needs is
    # computed (an input's, unless a stage reads constants only)
    self.start = min(n.need[0] + n.delay for n in self.nodes)
    self.max_delay = max(n.delay for n in self.stored)
    self.warm = self.max_delay - self.start
    self.name = '%s_tile3d_T%d_X%d_Y%d_W%d%s%s' % (
        self.st.app_name, self.T, self.TX, self.TY, self.W,
        '_nts' if nt_store else '', '_ntl' if nt_load else '')
    self.L: List[str] = []
    self.w = self.L.append

  def _lds_bytes(self, h: int) -> int:
    return sum(4 * n.ring * (n.guard[0][0] + self.TX + n.guard[0][1]) *
               (n.guard[1][0] + h + n.guard[1][1])
               for n in self.nodes if n.ring)

  # -- emission ---------------------------------------------------------------
  def emit(self) -> PassDesc:
    w = self.w
    slot = self.mod.slot
    w('// tile3d: T=%d fused iteration(s); tile %d x %d cells (valid %d x %d, '
      'ghost %d+%d / %d+%d), %d waves x %d rows, chunks along dim 2' %
      (self.T, self.TX, self.TY, self.VX, self.VY, self.mx[0], self.mx[1],
       self.my[0], self.my[1], self.W, self.RY))
    w('// %d bytes of LDS; %d steps of warm-up per chunk; one barrier per step'
      % (self.lds_bytes, self.warm))
    for n in self.nodes:
      w('//   %-20s delay %2d  ring %2d planes of %2d x %3d  ghost %d+%d / '
        '%d+%d' % (n.var, n.delay, n.ring, n.rows, n.pitch, n.margin[0][0],
                   n.margin[0][1], n.margin[1][0], n.margin[1][1]))
    w('extern "C" __global__ void __launch_bounds__(%d) %s(soda_hip_kargs_t a) {'
      % (64 * self.W, self.name))
    for n in self.nodes:
      if n.ring:
        w('  __shared__ __attribute__((aligned(16))) %s rg_%s[%d];' %
          (n.ctype, n.var, n.ring * n.plane))
    w('  const int lane = (int)(threadIdx.x & 63u);')
    w('  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));')
    if self.xcd:
      w('  const unsigned nblk = gridDim.x;')
      w('  const unsigned bid = (nblk % 8u == 0u) ? (blockIdx.x % 8u) * (nblk / 8u)'
        ' + blockIdx.x / 8u : blockIdx.x;')
    else:
      w('  const unsigned bid = blockIdx.x;')
    w('  const int tile_x = (int)(bid % (unsigned)a.ntile[0]);')
    w('  const int tile_y = (int)((bid / (unsigned)a.ntile[0]) % '
      '(unsigned)a.ntile[1]);')
    w('  const int chunk_l = (int)(bid / ((unsigned)a.ntile[0] * '
      '(unsigned)a.ntile[1]));')
    w('  const int chunk = chunk_l + (chunk_l >= a.skip_from ? a.skip_count : 0);')
    w('  const int n0 = a.extent[0], n1 = a.extent[1], nm = a.extent[2];')
    w('  const int ly0 = wave * %d;                 // first tile row of the thread'
      % self.RY)
    w('  const int gx0 = tile_x * %d - %d + lane;    // its first column in the grid'
      % (self.VX, self.mx[0]))
    w('  const int gy0 = tile_y * %d - %d + ly0;' % (self.VY, self.my[0]))
    w('  const int chunk_len = a.tile[2];')
    w('  const int m_begin = chunk * chunk_len;')
    w('  const int m_end = min(m_begin + chunk_len, nm);')
    w('  const int in_end = min(nm, m_end + %d);  // last input plane needed + 1'
      % self.m_hi)
    w('  const int wlo = max(0, m_begin + (%d));' % self.m_lo)
    w('  const unsigned pitch_b = (unsigned)a.stride[2] * 4u;')
    w('  const unsigned pitch_yb = (unsigned)a.stride[1] * 4u;')
    # offsets: plane part + row part + column part, each in range or
    # SODA_OOB_X, so the sum is out of range as soon as one is (soda_rt.h)
    for c in range(self.CX):
      w('  const int gx_%d = gx0 + %d;' % (c, 64 * c))
      w('  const bool x_ok%d = gx_%d >= 0 && gx_%d < n0;' % (c, c, c))
      w('  const unsigned xb%d = x_ok%d ? (unsigned)gx_%d * 4u : SODA_OOB_X;' %
        (c, c, c))
      w('  const unsigned sxb%d = (x_ok%d && lane + %d >= %d && lane + %d < %d) ? '
        '(unsigned)gx_%d * 4u : SODA_OOB_X;' %
        (c, c, 64 * c, self.mx[0], 64 * c, self.TX - self.mx[1], c))
    for j in range(self.RY):
      w('  const bool y_ok%d = gy0 + %d >= 0 && gy0 + %d < n1;' % (j, j, j))
      w('  const unsigned yo%d = y_ok%d ? (unsigned)(gy0 + %d) * pitch_yb : '
        'SODA_OOB_X;' % (j, j, j))
      w('  const unsigned syo%d = (y_ok%d && ly0 + %d >= %d && ly0 + %d < %d) ? '
        '(unsigned)(gy0 + %d) * pitch_yb : SODA_OOB_X;' %
        (j, j, j, self.my[0], j, self.TY - self.my[1], j))
    for n in self.inputs:
      nme = n.var[2:]
      w('  const soda_rsrc_t r_%s = soda_make_rsrc((const %s*)a.buf[%d] + '
        '(int64_t)wlo * a.stride[2], (int64_t)(in_end - wlo) * a.stride[2] * 4);'
        % (nme, n.ctype, slot[nme]))
    for n in self.stored:
      w('  const soda_rsrc_t w_%s = soda_make_rsrc((%s*)a.buf[%d] + '
        '(int64_t)m_begin * a.stride[2], (int64_t)(m_end - m_begin) * '
        'a.stride[2] * 4);' % (n.store, n.ctype, slot[n.store]))
    for n in self.nodes:
      if n.ring:
        w('  const int o_%s = (%d + ly0) * %d + %d + lane;  // the thread\'s '
          'first cell in a plane' % (n.var, n.guard[1][0], n.pitch,
                                     n.guard[0][0]))
        w('  int b_%s = 0;                  // ring slot of the plane being '
          'written' % n.var)
    for n in self.inputs:
      w('  %s nx_%s[%d];' % (n.ctype, n.var, self.RY * self.CX))
    w('  int t = m_begin + (%d);' % self.start)
    w('  // (a block whose chunk lies beyond the grid runs no step at all)')
    w('  const int t_end = m_begin < nm ? m_end + %d : t;' % self.max_delay)
    self._emit_loads('t')
    w('  for (; t < t_end; ++t) {')
    # ring slots (times the plane size) of the planes this step reads
    ages: Dict[Tuple[str, int], None] = {}
    for n in self.nodes:
      if n.stage is None:
        continue
      for pname, p in n.parents.items():
        for off in n.stage.taps[pname]:
          ages[(p.var, n.delay - off[2] - p.delay)] = None
    by_var = {n.var: n for n in self.nodes}
    for (var, age) in sorted(ages):
      p = by_var[var]
      if not 1 <= age < p.ring:
        raise util.InternalError('tile3d: age %d of %s (ring %d)' %
                                 (age, var, p.ring))
      w('    const int q_%s_%d = (b_%s >= %d ? b_%s - %d : b_%s + %d) * %d;' %
        (var, age, var, age, var, age, var, p.ring - age, p.plane))
    for n in self.nodes:
      if n.ring:
        w('    const int q_%s_0 = b_%s * %d;' % (n.var, n.var, n.plane))
    w('    // input plane t: from the registers it travelled in to its ring')
    for n in self.inputs:
      if not n.ring:
        continue
      for j in range(self.RY):
        for c in range(self.CX):
          w('    rg_%s[q_%s_0 + o_%s + %d] = nx_%s[%d];' %
            (n.var, n.var, n.var, j * n.pitch + 64 * c, n.var,
             j * self.CX + c))
    w('    // plane t + 1 sets out while this step computes')
    self._emit_loads('t + 1', indent='    ')
    self.lds_reads = 0
    for n in self.nodes:
      if n.stage is not None:
        self._emit_stage(n)
    w('    soda_pipe_barrier();')
    for n in self.nodes:
      if n.ring:
        w('    b_%s = b_%s == %d ? 0 : b_%s + 1;' %
          (n.var, n.var, n.ring - 1, n.var))
    w('  }')
    w('}')
    return self._finish()

  def _emit_loads(self, t_expr: str, indent: str = '  ') -> None:
    w = self.w
    w('%s{' % indent)
    w('%s  const int tl = %s;' % (indent, t_expr))
    w('%s  const unsigned po = (tl >= wlo && tl < in_end) ? (unsigned)(tl - wlo) '
      '* pitch_b : SODA_OOB_X;' % indent)
    for n in self.inputs:
      for j in range(self.RY):
        for c in range(self.CX):
          w('%s  soda_buf_load_frag<%s, 1, %s>(*(%s(*)[1])&nx_%s[%d], r_%s, '
            'po + yo%d + xb%d);' % (indent, n.ctype, self.nt_l, n.ctype, n.var,
                                    j * self.CX + c, n.var[2:], j, c))
    w('%s}' % indent)

  def _emit_stage(self, n: _Node) -> None:
    w = self.w
    stage = n.stage
    w('    // %s: plane t - %d' % (n.var, n.delay))
    w('    %s v_%s[%d];' % (n.ctype, n.var, self.RY * self.CX))
    seen = set()
    for j in range(self.RY):
      for c in range(self.CX):

        def load(ref: ir.Ref, _j=j, _c=c) -> str:
          off = tuple(a - b for a, b in zip(ref.idx, stage.st_idx))
          p = n.parents[ref.name]
          age = n.delay - off[2] - p.delay
          if not all(-p.guard[d][0] <= off[d] <= p.guard[d][1]
                     for d in (0, 1)):
            raise util.InternalError('tile3d: tap %s of %s leaves the guard '
                                     'cells of %s' % (off, n.var, p.var))
          where = (_j + off[1]) * p.pitch + off[0] + 64 * _c
          seen.add((p.var, age, where))
          return 'rg_%s[q_%s_%d + o_%s + (%d)]' % (p.var, p.var, age, p.var,
                                                   where)

        dst = 'v_%s[%d]' % (n.var, j * self.CX + c)
        if stage.stmt.let:
          w('    {')
          for let in stage.stmt.let:
            w('      const %s %s = %s;' %
              (let.haoda_type.c_type, let.name,
               ir.c_expr(let.expr, load, self.mod.param_var)))
          w('      %s = (%s)(%s);' % (dst, n.ctype, ir.c_expr(
              stage.stmt.expr, load, self.mod.param_var)))
          w('    }')
        else:
          w('    %s = (%s)(%s);' % (dst, n.ctype, ir.c_expr(
              stage.stmt.expr, load, self.mod.param_var)))
    self.lds_reads += len(seen)
    if n.ring:
      for j in range(self.RY):
        for c in range(self.CX):
          w('    rg_%s[q_%s_0 + o_%s + %d] = v_%s[%d];' %
            (n.var, n.var, n.var, j * n.pitch + 64 * c, n.var,
             j * self.CX + c))
    if n.store is not None:
      w('    {')
      w('      const int m = t - (%d);' % n.delay)
      w('      const unsigned mo = (m >= m_begin && m < m_end) ? '
        '(unsigned)(m - m_begin) * pitch_b : SODA_OOB_X;')
      for j in range(self.RY):
        for c in range(self.CX):
          w('      soda_buf_store_frag<%s, 1, %s>(w_%s, mo + syo%d + sxb%d, '
            '*(const %s(*)[1])&v_%s[%d]);' %
            (n.ctype, self.nt_s, n.store, j, c, n.ctype, n.var,
             j * self.CX + c))
      w('    }')

  def _finish(self) -> PassDesc:
    redundancy = (self.TX * self.TY) / float(self.VX * self.VY)
    idx = self.mod.add_kernel(
        KernelDesc(self.name, (64 * self.W, 1, 1),
                   (self.VX, self.VY, self.chunk), lds_bytes=0,
                   note='tile3d T%d' % self.T,
                   # a block per tile, its residency set by LDS: the chunk rule
                   # of the register-marching kernels (waves per SIMD from the
                   # register count) does not apply, the length is fixed
                   tune=dict(axis=2, waves_along=1, waves_per_block=self.W,
                             warm=self.warm, fixed=True, pipe=1, vec=1,
                             # the launch-time model was fitted to the
                             # register-marching kernels (VALU issue against
                             # HBM); a step here is LDS traffic and a barrier,
                             # which it has no term for: the pass is left to
                             # the clock (soda_hip_program_calibrate)
                             unmodelled=True, step_ops=0.0, fused=self.T,
                             lane_redundancy=redundancy,
                             window_extra=self.m_hi - self.m_lo, max_elem=4,
                             tile3d=(self.TX, self.TY))),
        '\n'.join(self.L) + '\n')
    table = self.st.symbol_table
    io = sum(table[x].size_in_bytes
             for x in list(self.st.input_names) + list(self.st.output_names))
    p = PassDesc(self.T, [idx], 'tile3d',
                 dict(bytes_per_cell_min=io, lds_bytes=self.lds_bytes,
                      read_redundancy=redundancy *
                      (self.chunk + self.m_hi - self.m_lo) / float(self.chunk),
                      tile=(self.TX, self.TY), valid=(self.VX, self.VY),
                      waves=self.W, warm_steps=self.warm,
                      lds_reads_per_step=self.lds_reads,
                      blocks_per_cu=max(1, LDS_MAX // self.lds_bytes)))
    self.mod.passes.append(p)
    return p


def add_tile3d_pass(mod: Module, fused_iters: int, *,
                    tile_w: Optional[int] = None, tile_h: Optional[int] = None,
                    waves: Optional[int] = None, chunk: Optional[int] = None,
                    nt_load: bool = False, nt_store: bool = False,
                    xcd_swizzle: bool = True) -> PassDesc:
  """Adds one tile3d kernel (and its pass) that advances `fused_iters`
  iterations; raises SemanticError if the program is not one tile3d runs or
  its plane rings do not fit LDS at this depth.  `None` = the default: a tile
  of 64 cells by the height the rule in _Tile3dKernel picks, as many waves
  (8, 4, 2 or 1) as divide it, chunks of 128 planes."""
  return _Tile3dKernel(mod, fused_iters, tile_w, tile_h, waves,
                       chunk or CHUNK, nt_load, nt_store, xcd_swizzle).emit()
