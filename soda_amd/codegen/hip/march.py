"""`march2d` / `march3d`: register-window marching kernels (see lower.py for
the design; DESIGN.md section 4.1 for the measurements behind the choices).
This file holds the kernels' options (MarchConfig), their HIP text
(_MarchKernel) and the entry points; what a kernel is -- chain, geometry,
windows, warm-up -- is decided in march_schedule.py, before any text."""
from typing import Dict, List, Optional, Tuple

from soda_amd import core, ir, util

from soda_amd.codegen.hip.march_schedule import (  # noqa: F401
    MAX_FUSE_3D, MAX_FUSE_PRESERVE, MAX_SHIFT_TEMPS, MAX_UNROLL, MIRROR_PREFETCH,
    REG_BUDGET, Schedule, _build_chain, _choose_unroll, _Node,
    bank_fragment_map, march_supported)
from soda_amd.codegen.hip.module import KernelDesc, Module, PassDesc

# ---------------------------------------------------------------------------
# march: register-window marching along the last (streamed) dimension
# ---------------------------------------------------------------------------

LDS_PER_CU = 160 * 1024     # MI355X_MICROARCH.md


# how a row is shifted by one lane (MarchConfig.lane_shift) -> its tag in the
# kernel name
LANE_SHIFTS = {'dpp': '', 'mixh': '_mixh'}


class MarchConfig:

  def __init__(self, *, fused_iters: int = 1, vec: int = 4, chunk_rows: int = 64,
               prefetch: int = 2, waves_x: int = 1, waves_y: int = 1,
               nt_store: bool = False, nt_load: bool = True,
               xcd_swizzle: bool = True, edge_loads: bool = True,
               tile_rows: int = 6, lane_shift: str = 'dpp',
               min_waves: int = 0, occupancy: int = 0,
               pipe: int = 1, pipe_rows: int = 4, stamps: bool = False,
               peel: int = -1, align_lanes: int = 1, xshare: int = 0,
               xwindow: bool = True, slide: bool = True,
               xshare_block: int = 0,
               banks: Optional[Dict[str, int]] = None,
               bank_lead: Optional[Dict[str, int]] = None,
               residual: bool = False):
    # the kernel's twin (LowerOptions.residual): same chain, same stores, and
    # on the last fused level every output is also a consumer of the input it
    # replaces, at offset 0; the delta is taken where the plane is stored,
    # under the store's own predicate (_emit_store).  Name: the plain
    # kernel's + `_rs`
    self.residual = bool(residual)
    # the banked form of a wire stream's dense program: {input or output: NB}.
    # Such a tensor is not one dense array but NB banks, stream element k in
    # bank k % NB at index k / NB; the kernel addresses every bank through a
    # resource of its own and (de)interleaves in registers (soda_rt_banked.h,
    # bank_fragment_map).  The tensor takes NB consecutive a.buf[] slots.
    # `bank_lead`: {input: elements}, the delay of the reference host that the
    # kernel undoes by starting lead / NB elements into every bank; dense
    # element k + lead of such an input is read as zero from
    # a.reserved[0] (the stream's length) on.
    self.banks = dict(banks or {})
    self.bank_lead = {n: int(v) for n, v in (bank_lead or {}).items() if v}
    # integer window reductions along dimension 0 evaluated for all cells of
    # a lane jointly (_xwindow_body); integer sums along the streamed
    # dimension as sliding sums
    self.xwindow = xwindow
    self.slide = slide
    # x-halos shared through LDS: a block of `xshare` waves covers the WHOLE
    # row (extent[0] <= xshare * 64 * vec, checked at launch), every wave a
    # strip of 64 fully valid lanes; the one cell a fused iteration needs from
    # the neighbouring strip's intermediate results is handed over through LDS
    # (lanes 0 and 63 write their end cells, one barrier per row step, the
    # neighbour reads them into the register DPP shifts take their `old`
    # operand from -- the mechanism edge loads use for the program inputs).
    # Without it a T = 2 strip of heat3d has 62 valid lanes = 248 cells and a
    # 512-cell row needs THREE waves, the third nearly idle.
    self.xshare = int(xshare)
    # segmented x-halo sharing: a block of `xshare_block` waves side by side
    # covers a SEGMENT of the row, S = (64 * xshare_block - lanes_lo -
    # lanes_hi) * vec cells of it stored.  Between the block's waves the end
    # cells change hands exactly as above; the segment's two outer sides have
    # no neighbour in the block, read the cell that stays zero and lose a
    # fused iteration's x-reach per level, as an overlapping strip does, so
    # neighbouring blocks overlap by lanes_lo + lanes_hi lanes.  Halo lanes
    # are lanes_lo + lanes_hi of 64 * xshare_block instead of every 64; any
    # row length runs, none is needed at build time.  Wins over `xshare`.
    self.xshare_block = int(xshare_block)
    # valid lanes of a strip rounded down to a multiple of this (extra halo
    # lanes on the high side): 4 makes a strip's rows start and end on 64-byte
    # boundaries.  Pays where rows are written with non-temporal stores -- a
    # 63-lane strip's 1008-byte rows end in partial lines that go to memory
    # twice (blur 16384^2: 225 -> 202 us at 60 lanes) -- and not with plain
    # stores, which L2 merges (jacobi2d T = 4 / 8 / 12: no gain, slower)
    self.align_lanes = max(1, int(align_lanes))
    # the pipeline warm-up of a chunk as straight-line code in front of the
    # loop, WITHOUT the stages whose rows cannot reach an output row of the
    # chunk yet (fused iteration l first matters 2l row steps into the chunk:
    # T = 12 computes 156 of its first 288 stage-rows for nothing otherwise)
    # (in whole trips of the unrolled loop; -1: all the warm-up, 0: none.  The
    # last trips are nearly full row steps, save little and can cost registers
    # -- T = 12: 159 VGPRs with 2 of its 4 trips peeled, 231 with all four --
    # so runtime.select_peel picks the count per kernel from compiled code)
    self.peel = int(peel)
    # diagnostics: every wave records s_memtime at entry and exit and where it
    # ran (tools/timeline.py)
    self.stamps = stamps
    # row steps per barrier of a stage-pipelined block (power of two): the
    # waves synchronise once per `pipe_rows` rows through a ring of twice
    # that many slots
    self.pipe_rows = pipe_rows if pipe > 1 else 1
    # stage-pipelined blocks: the fused iterations are split over `pipe` waves
    # of a block; wave w runs iterations [w*T/pipe, (w+1)*T/pipe) of the SAME
    # strip and chunk one tick behind wave w-1, rows travel through a 2-slot
    # LDS ring, one barrier per tick.  Fewer registers per wave (more waves per
    # SIMD) and `pipe` times longer chunks for the same number of waves (the
    # 2T-row warm-up is paid per block, not per wave).
    self.pipe = pipe
    # cap the waves resident per SIMD (0 = whatever the registers allow) by
    # giving every block an LDS allocation it never touches: 3 waves per SIMD
    # issue VALU work slower than 2 or 4 (tools/valubench.py)
    self.occupancy = occupancy
    # ask the register allocator for at least this many waves per SIMD
    # (amdgpu_waves_per_eu); 0 = let it use what it wants
    self.min_waves = min_waves
    # how a row is shifted by one lane: 'dpp' (wave_shr/shl fused into the
    # consuming add) or 'mixh' (down through DPP, up through a ds_swizzle
    # rotate; the wave holds two independent 32-lane half strips, each with its
    # own halo lanes)
    self.lane_shift = lane_shift
    self.fused_iters = fused_iters
    self.vec = vec
    self.chunk_rows = chunk_rows  # cells one wave marches over (last dim)
    self.prefetch = prefetch
    self.waves_x = waves_x
    self.waves_y = waves_y
    self.nt_store = nt_store      # non-temporal stores of the output rows
    self.nt_load = nt_load        # non-temporal loads of the input rows
    self.xcd_swizzle = xcd_swizzle  # neighbouring tiles on one XCD (one L2)
    self.edge_loads = edge_loads  # halo cells of the inputs fetched by the
    #                               strip's edge lanes instead of overlap
    self.tile_rows = tile_rows    # 3-D: output rows (dim 1) per wave
    self.chunk_fixed = False      # True: the host must not re-size the chunk

  def key(self) -> str:
    # chunk_rows is a launch-time value, not part of the code.  Every name
    # carries `_buf` (buffer addressing, once optional): the names key
    # profiles/traffic.json
    return ''.join((
        'T%d_V%d_P%d_W%dx%d_R%d' % (self.fused_iters, self.vec, self.prefetch,
                                    self.waves_x, self.waves_y, self.tile_rows),
        '_nts' if self.nt_store else '', '_ntl' if self.nt_load else '',
        '_xcd' if self.xcd_swizzle else '', '_edge' if self.edge_loads else '',
        LANE_SHIFTS[self.lane_shift],
        '_mw%d' % self.min_waves if self.min_waves else '',
        '_occ%d' % self.occupancy if self.occupancy else '',
        '_buf',
        '_pipe%dx%d' % (self.pipe, self.pipe_rows) if self.pipe > 1 else '',
        '_st' if self.stamps else '',
        '_k%d' % self.peel if self.peel >= 0 else '',
        '_al%d' % self.align_lanes if self.align_lanes > 1 else '',
        '_xs%d' % self.xshare if self.xshare and not self.xshare_block
        else '',
        '_xb%d' % self.xshare_block if self.xshare_block else '',
        '_bk_' + '_'.join('%sx%d' % (n, nb) + (
            'l%d' % self.bank_lead[n] if n in self.bank_lead else '')
                         for n, nb in sorted(self.banks.items()))
        if self.banks else ''))


def default_vec(stencil: core.Stencil) -> int:
  """16 bytes per lane per row for the widest tensor."""
  widest = max(t.size_in_bytes for t in stencil.symbol_table.values())
  return max(1, 16 // widest)


def edge_cell_banks(i: int, vec: int, nb: int) -> Tuple[int, int]:
  """Banks of the i-th halo cell left of a strip (cell -1 - i relative to the
  strip's first) and right of it (cell vec + i relative to the first cell of
  the strip's LAST lane): strips and lanes start on bank-group boundaries, so
  both are constants of the kernel."""
  if nb < 1 or vec % nb:
    raise util.SemanticError('banks: %d cells per lane, %d banks' % (vec, nb))
  return (-1 - i) % nb, (vec + i) % nb


class _Tick:
  """What the stages of one row step share while its text is written (one is
  also made for the set-up of a sliding sum in front of the loop)."""

  def __init__(self, k: int, mark: int):
    self.k = k            # slot phase of the step
    # lane-shifted operands of the step, shared by its stages:
    # (tensor, slot, row, cell, lanes) -> the copy's name
    self.shifted: Dict[Tuple[str, int, int, int, int], str] = {}
    self.wide: Dict[str, str] = {}   # one-byte cells widened in this step
    # index into the line list at which the previous stage's block of this
    # step begins: early shifts are put in front of it
    self.mark = mark
    # of the stage being written: the lines in front of its statements, and
    # the shifts that may be issued a stage ahead
    self.pre: List[str] = []
    self.early: List[str] = []


class _MarchKernel:
  """The HIP text of one marching kernel: spells the Schedule `s`, decides
  nothing (`emit`)."""

  def __init__(self, mod: Module, cfg: MarchConfig):
    self.mod, self.cfg = mod, cfg
    self.s = Schedule(mod.stencil, cfg, mod.banks, mod.slot)
    self.L: List[str] = []
    self.w = self.L.append
    self.shift_temps = 0    # lane-shifted copies alive within one tick

  @staticmethod
  def _reg(n: _Node, slot: int, row: int) -> str:
    """The register fragment that holds row `row` of the plane in `slot`."""
    return '%s_s%d_r%d' % (n.var, slot, row)

  def _load_row(self, es: int, j: int) -> str:
    """Row offset of a load of `es`-byte cells (declared by _emit_loads)."""
    return 'ro%d' % es if self.s.dim == 2 else 'ro%d_%d' % (es, j)

  def _store_row(self, es: int, j: int) -> str:
    """Offset of a lane's fragment of row `j` of the plane being stored."""
    if self.s.dim == 3:
      return ('(m_ok ? (unsigned)(m - m_begin) * pitch_b%d : SODA_OOB_X) + '
              'yo%d_%d + sxb%d' % (es, es, j, es))
    return ('(m_ok ? (unsigned)(m - m_begin) * pitch_b%d : SODA_OOB_ROW) '
            '+ sxb%d' % (es, es))

  # -- emission ---------------------------------------------------------------
  def emit(self) -> PassDesc:
    s = self.s
    self._emit_header()
    self._emit_addressing()
    for wv in range(s.W):
      self._emit_wave(wv)
    if self.cfg.stamps:
      self.w('  if (lane == 0) {')
      self.w('    unsigned long long* d = (unsigned long long*)a.buf[15] + '
             '4ull * ((unsigned long long)blockIdx.x * %d + wave);' % s.waves)
      self.w('    d[0] = soda_t0;')
      self.w('    d[1] = __builtin_amdgcn_s_memtime();')
      self.w('    d[2] = __builtin_amdgcn_s_getreg(63492);   // HW_REG_HW_ID')
      self.w('    d[3] = __builtin_amdgcn_s_getreg(63508);   // HW_REG_XCC_ID')
      self.w('  }')
    if self.cfg.residual:
      # one wave reduction and lane 0's atomics, at the end of the kernel
      self.w('  soda_res_flush(soda_acc, soda_res);')
    self.w('}')
    self._check_emitted()
    return self._register(*self._launch_model())

  def _emit_header(self) -> None:
    s, cfg = self.s, self.cfg
    self.w('// %s: T=%d fused iteration(s), %d cells/lane, chunks of %d along dim %d,'
      ' prefetch %d, unroll %d' % (s.kind, s.T, s.V, cfg.chunk_rows, s.ax, s.PF,
                                   s.U))
    self.w('// strip: %d lanes valid of 64 (halo %d+%d cells, edge loads %d+%d); '
      'pipeline depth %d' % (s.strip_lanes, s.margin_lo, s.margin_hi,
                             s.edge[0], s.edge[1], s.warm))
    if s.seg:
      self.w('// segment: %d waves side by side store %d cells; x-halos shared '
             'through LDS between them, %d+%d halo lanes at the outer sides' %
             (s.xs, s.seg_cells, s.lanes_lo, s.lanes_hi))
    for nme, nb in sorted(s.banks.items()):
      self.w('// banked: %s on %d banks (a.buf[%d..%d]), cell j of a fragment = '
             'element j / %d of bank j %% %d%s' %
             (nme, nb, self.mod.slot[nme], self.mod.slot[nme] + nb - 1, nb, nb,
              ', read %d elements on' % cfg.bank_lead[nme]
              if nme in cfg.bank_lead else ''))
    if s.dim == 3:
      self.w('// tile: %d rows held in registers for %d output rows (halo %d+%d)' %
        (s.rows_in, s.tile_rows, s.rhalo_lo, s.rhalo_hi))
    for n in s.nodes:
      self.w('//   %-24s delay %2d  window %2d (slots %2d)  margin %d/%d  rows %d/%d' %
        (n.var, n.delay, n.window, n.slots, n.margin[0], n.margin[1],
         n.rmargin[0], n.rmargin[1]))
    self.w('extern "C" __global__ void __launch_bounds__(%d) %s%s%s'
      % (s.block, '__attribute__((amdgpu_waves_per_eu(%d, %d))) ' %
         (cfg.min_waves, max(cfg.min_waves, 8))
         if cfg.min_waves else '', s.name,
         '(soda_hip_kargs_t a, soda_hip_residual_t* soda_res, '
         'soda_hip_resbox_t soda_box) {' if cfg.residual else
         '(soda_hip_kargs_t a) {'))
    if cfg.residual:
      self.w('  soda_res_lane_t soda_acc;  // this lane\'s share of the residual')
      self.w('  soda_res_init(soda_acc);')
    if cfg.stamps:
      self.w('  const unsigned long long soda_t0 = __builtin_amdgcn_s_memtime();')
    self.w('  const int lane = (int)(threadIdx.x & 63u);')
    self.w('  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));')
    if cfg.xcd_swizzle:
      # blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous
      # run of tiles so halo rows/columns shared by neighbours hit one L2
      # (speed only; any placement is correct)
      self.w('  const unsigned nblk = gridDim.x;')
      self.w('  const unsigned bid = (nblk % 8u == 0u) ? (blockIdx.x % 8u) * (nblk / 8u)'
        ' + blockIdx.x / 8u : blockIdx.x;')
    else:
      self.w('  const unsigned bid = blockIdx.x;')
    self.w('  const int tile_x = (int)(bid % (unsigned)a.ntile[0]);')
    if s.dim == 2:
      self.w('  const int tile_l = (int)(bid / (unsigned)a.ntile[0]);')
      self.w('  const int tile_m = tile_l + (tile_l >= a.skip_from ? a.skip_count : 0);')
      if s.xs:           # the block's waves cover the row side by side
        self.w('  const int strip = wave;')
        self.w('  const int chunk = tile_m;')
      elif s.W > 1:      # all waves of the block share the strip and the chunk
        self.w('  const int strip = tile_x;')
        self.w('  const int chunk = tile_m;')
      else:
        self.w('  const int strip = tile_x * %d + wave %% %d;' % (s.wx, s.wx))
        self.w('  const int chunk = tile_m * %d + wave / %d;' % (cfg.waves_y, s.wx))
      self.w('  const int n0 = a.extent[0], nm = a.extent[1];')
    else:
      self.w('  const int tile_y = (int)((bid / (unsigned)a.ntile[0]) % '
        '(unsigned)a.ntile[1]);')
      self.w('  const int chunk_l = (int)(bid / ((unsigned)a.ntile[0] * '
        '(unsigned)a.ntile[1]));')
      self.w('  const int chunk = chunk_l + (chunk_l >= a.skip_from ? a.skip_count : 0);')
      self.w('  const int strip = %s;' % ('wave' if s.xs else 'tile_x'))
      self.w('  const int n0 = a.extent[0], n1 = a.extent[1], nm = a.extent[2];')
      self.w('  const int y0 = tile_y * %d - %d;  // first row held' %
        (s.tile_rows, s.rhalo_lo))
      self.w('  const int64_t pitch_y = a.stride[1];')
    if s.seg:
      # wave `strip` of the block's segment: 64 lanes right of its neighbour's
      self.w('  const int sub = lane;')
      self.w('  const int x0 = tile_x * %d + (strip * 64 + lane - %d) * %d;' %
        (s.seg_cells, s.lanes_lo, s.V))
    elif s.group == 64:
      self.w('  const int sub = lane;')
      self.w('  const int x0 = strip * %d + (lane - %d) * %d;' %
        (s.strip_cells, s.lanes_lo, s.V))
    else:     # two half strips side by side, each with its own halo lanes
      self.w('  const int sub = lane & %d;' % (s.group - 1))
      self.w('  const int x0 = strip * %d + (lane >> 5) * %d + (sub - %d) * %d;'
        % (s.strip_cells, s.group_lanes * s.V, s.lanes_lo, s.V))
    # chunk length is a launch-time value (kernel descriptor tile / waves): the
    # host sizes it so the grid fills the GPU in whole rounds of waves
    self.w('  const int chunk_len = a.tile[%d] / %d;' %
      (s.ax, cfg.waves_y if s.dim == 2 else 1))
    self.w('  const int m_begin = chunk * chunk_len;')
    self.w('  const int m_end = min(m_begin + chunk_len, nm);')
    if s.xs:
      # every wave of the block takes part in the barriers, whatever its strip
      self.w('  if (m_begin >= nm) return;  // block-uniform')
    else:
      self.w('  if (m_begin >= nm || strip * %d >= n0) return;  // wave-uniform' %
        s.strip_cells)
    self.w('  const bool lane_ok = x0 >= 0 && x0 + %d <= n0;' % s.V)
    if s.seg:
      # the halo lanes are the first of the first wave and the last of the last
      self.w('  const bool store_ok = lane_ok && (strip > 0 || sub >= %d) && '
             '(strip < %d || sub < %d);' %
             (s.lanes_lo, s.xs - 1, 64 - s.lanes_hi))
    else:
      self.w('  const bool store_ok = lane_ok && sub >= %d && sub < %d;' %
        (s.lanes_lo, s.group - s.lanes_hi))
    self.w('  const int64_t pitch = a.stride[%d];' % s.ax)
    # (read by nothing: the buffer offsets below address every tensor; the
    # line stays so that the generated kernels keep their exact text)
    self.w('  const int64_t x0c = lane_ok ? (int64_t)x0 : 0;')

  def _emit_addressing(self) -> None:
    s, cfg = self.s, self.cfg
    # vector memory through buffer resources with out-of-range offsets instead
    # of `if (row_ok)` branches: straight-line loop body, exact s_waitcnt
    # counts.  Every tensor is addressed through a window that starts at the
    # first plane this wave touches; see soda_rt.h for the offset encoding
    self.w('  const int in_end = min(nm, m_end + %d);  // last input plane needed + 1'
      % s.m_hi)
    self.w('  const int wlo = max(0, m_begin + (%d));' % s.m_lo)
    for es in sorted(set(s.esz.values())):
      self.w('  const unsigned xb%d = lane_ok ? (unsigned)x0 * %du : SODA_OOB_X;' %
        (es, es))
      self.w('  const unsigned sxb%d = store_ok ? (unsigned)x0 * %du : SODA_OOB_X;' %
        (es, es))
      self.w('  const unsigned pitch_b%d = (unsigned)pitch * %du;' % (es, es))
      if s.dim == 3:
        self.w('  const unsigned pitch_yb%d = (unsigned)pitch_y * %du;' % (es, es))
        for j in range(s.rows_in):
          self.w('  const unsigned yo%d_%d = (y0 + %d >= 0 && y0 + %d < n1) ? '
                 '(unsigned)(y0 + %d) * pitch_yb%d : SODA_OOB_X;' %
                 (es, j, j, j, j, es))
    for nme, n in s.inputs.items():
      if nme in s.banks:
        # every bank's window: 1 / NB of the dense window, from 1 / NB of its
        # first element on (NB divides the row pitch and the lead: the library
        # admits no other stream).  A delayed input ends `lead` elements
        # early: what lies beyond the stream reads as zero.  The clipped end,
        # element n - lead, is a fragment boundary (stream.banked_tensors
        # offers a delayed input only where V divides the lead and the
        # stream's length n), so no access straddles it: every fragment is
        # wholly inside the window or wholly dropped, as `unwire_` zeroes
        nb, lead = s.banks[nme], cfg.bank_lead.get(nme, 0)
        size = '(int64_t)(in_end - wlo) * pitch'
        if lead:
          self.w('  const int64_t left_%s = (int64_t)a.reserved[0] - %d - '
                 '(int64_t)wlo * pitch;  // elements of the stream from wlo on'
                 % (nme, lead))
          size = '(%s < left_%s ? %s : left_%s)' % (size, nme, size, nme)
        for b in range(nb):
          self.w('  const soda_rsrc_t r_%s_b%d = soda_make_rsrc_bank<%d>((const '
                 '%s*)a.buf[%d] + ((int64_t)wlo * pitch + %d) / %d, %s * %d);' %
                 (nme, b, nb, n.ctype, self.mod.slot[nme] + b, lead, nb, size,
                  s.esz[nme]))
        continue
      self.w('  const soda_rsrc_t r_%s = soda_make_rsrc((const %s*)a.buf[%d] + '
        '(int64_t)wlo * pitch, (int64_t)(in_end - wlo) * pitch * %d);' %
        (nme, n.ctype, self.mod.slot[nme], s.esz[nme]))
    for o, n in s.outputs.items():
      if o in s.banks:
        nb = s.banks[o]
        for b in range(nb):
          self.w('  const soda_rsrc_t w_%s_b%d = soda_make_rsrc_bank<%d>((%s*)'
                 'a.buf[%d] + ((int64_t)m_begin * pitch) / %d, (int64_t)(m_end - '
                 'm_begin) * pitch * %d);' %
                 (o, b, nb, n.ctype, self.mod.slot[o] + b, nb, s.esz[o]))
        continue
      self.w('  const soda_rsrc_t w_%s = soda_make_rsrc((%s*)a.buf[%d] + '
        '(int64_t)m_begin * pitch, (int64_t)(m_end - m_begin) * pitch * %d);' %
        (o, n.ctype, self.mod.slot[o], s.esz[o]))
    if cfg.residual:
      # the cells of a lane that count: those its stores land (store_ok; a
      # lane is wholly inside the row or wholly outside) inside the pair's box
      for p, o in enumerate(s.st.output_names):
        for e in range(s.V):
          self.w('  const bool rsx%d_%d = store_ok && x0 + %d >= soda_box.lo[%d][0] '
                 '&& x0 + %d < soda_box.hi[%d][0];' % (p, e, e, p, e, p))
    if s.xs or s.n_edge:
      self.w('  const bool edge_lane = lane == 0 || lane == 63;')
    if s.xs_nodes:    # (none: no tap leaves its column, nothing to share)
      for n in s.xs_nodes:
        # [parity of the row step][wave][0: its first cell, 1: its last][row],
        # then one cell that stays zero (what lies beyond the row's ends)
        self.w('  __shared__ %s soda_xs_%s[%d];' %
               (n.ctype, n.var, 2 * s.xs_stride + 1))
      self.w('  if (threadIdx.x == 0) {')
      for n in s.xs_nodes:
        self.w('    soda_xs_%s[%d] = (%s)0;' % (n.var, 2 * s.xs_stride, n.ctype))
      self.w('  }')
      self.w('  soda_pipe_barrier();')
      # writing: lane 0 files its first cell, lane 63 its last
      self.w('  const int xs_wr = (wave * 2 + (lane == 0 ? 0 : 1)) * %d;' %
             s.xs_rows)
      # reading: lane r takes row r's cell from the strip on the left (its last
      # cell), lane 32 + r from the strip on the right (its first cell); lanes
      # without a neighbour or a row read the zero cell
      self.w('  const int xs_nb = lane < 32 ? wave - 1 : wave + 1;')
      self.w('  const int xs_rd = (xs_nb >= 0 && xs_nb < %d && (lane & 31) < %d) ? '
             '(xs_nb * 2 + (lane < 32 ? 1 : 0)) * %d + (lane & 31) : %d;' %
             (s.xs, s.xs_rows, s.xs_rows, 2 * s.xs_stride))
    if s.n_edge:
      # lane 0 fetches the cells left of the strip, lane 63 those right of it;
      # DPP hands them to the shifted reads through the `old` operand
      for i in range(s.n_edge):
        self.w('  const int ex%d = lane == 0 ? x0 - %d : x0 + %d;' %
          (i, 1 + i, s.V + i))
        self.w('  const bool edge_ok%d = edge_lane && ex%d >= 0 && ex%d < n0;' %
          (i, i, i))
        for es in sorted({s.esz[nme] for nme in s.inputs}):
          self.w('  const unsigned exb%d_%d = edge_ok%d ? (unsigned)ex%d * %du : '
            'SODA_OOB_X;' % (i, es, i, i, es))

    if s.st.preserve_border:
      # border: preserve -- which of a lane's cells lie outside the columns one
      # iteration can compute (the same for every fused iteration)
      for o in s.st.output_names:
        wlo, whi = s.st.interior_bounds(o)
        for e in range(s.V):
          self.w('  const bool keepx_%s_%d = !(a.origin[0] + x0 + %d >= %d && '
                 'a.origin[0] + x0 + %d < a.gextent[0] - %d);'
                 % (o, e, e, max(0, -wlo[0]), e, max(0, whi[0])))
    declared = set()
    for stage in s.st.ordered_stages:      # `param` arrays: plain pointers
      for line in self.mod.param_decls(stage):
        if line not in declared:
          declared.add(line)
          self.w(line)
    for n in s.nodes:
      if n.to_lds:     # written at tick t, read by the next wave at tick t + R
        self.w('  __shared__ %s soda_ring_%s[%d][%d][%d];' % (
            n.ctype, n.var, 2 * s.R, s.rows_in, 64 * s.V))

  def _emit_decls(self, wv: int) -> None:
    s = self.s
    for n in s.nodes:
      if n.owner != wv:
        continue
      if id(n) in s.slide:
        for j in s.rows_of(n):
          self.w('  int xa_%s_r%d[%d];' % (n.var, j, s.V))
          self.w('  soda_zero_frag<int, %d>(xa_%s_r%d);' % (s.V, n.var, j))
      for slot in range(n.slots):
        for j in s.rows_of(n):
          reg = self._reg(n, slot, j)
          self.w('  %s %s[%d];' % (n.ctype, reg, s.V))
          self.w('  soda_zero_frag<%s, %d>(%s);' % (n.ctype, s.V, reg))
          if n.is_input and s.n_edge:
            self.w('  %s %s_e[%d];' % (n.ctype, reg, s.n_edge))
            self.w('  soda_zero_frag<%s, %d>(%s_e);' % (n.ctype, s.n_edge, reg))
        if n.xs:
          # halo cells of the plane in slot s: lane r / 32 + r holds row r's
          # left / right neighbour cell
          self.w('  %s hv_%s_s%d = (%s)0;' % (n.ctype, n.var, slot, n.ctype))

  def _emit_loads(self, k: int, t_expr: str, pin: bool = False) -> None:
    """Issues the loads of input plane t (tick phase k).  `pin`: the step is
    straight-line code (peeled warm-up); its loads take their lane offset
    from an opaque copy made here, or the compiler hoists the loads of ALL
    peeled steps to the top of the kernel (T = 12: 229 instead of 159
    VGPRs)."""
    s = self.s
    self.w('      const int t = %s;' % t_expr)
    self.w('      const bool plane_ok = t >= 0 && t < in_end;')
    if pin:
      for es in sorted({s.esz[nme] for nme in s.inputs}):
        self.w('      unsigned xb%dp = xb%d; asm volatile("" : "+v"(xb%dp));'
               % (es, es, es))
    pinned = 'p' if pin else ''
    for es in sorted({s.esz[nme] for nme in s.inputs}):
      if s.dim == 2:
        self.w('      const unsigned ro%d = plane_ok ? (unsigned)(t - wlo) * '
          'pitch_b%d : SODA_OOB_ROW;' % (es, es))
      else:
        # plane part + row part (loop-invariant, emitted once) + lane
        # part, each either in range or 2^30: the sum is out of range as
        # soon as one of them is, and cannot wrap (soda_rt.h)
        self.w('      const unsigned po%d = plane_ok ? (unsigned)(t - wlo) * '
          'pitch_b%d : SODA_OOB_X;' % (es, es))
        for j in sorted({j for n in s.inputs.values() for j in s.rows_of(n)}):
          self.w('      const unsigned ro%d_%d = po%d + yo%d_%d;' %
                 (es, j, es, es, j))
    for nme, n in s.inputs.items():
      slot = s.slot_of(n, k, 0)
      for j in s.rows_of(n):
        es = s.esz[nme]
        ro = self._load_row(es, j)
        reg = self._reg(n, slot, j)
        if nme in s.banks:
          nb = s.banks[nme]
          self.w('      soda_buf_load_frag_banked<%s, %d, %d, %s>(%s, %s + '
                 'xb%d%s, %s);' %
                 (n.ctype, s.V, nb, s.nt_l, reg, ro, es, pinned,
                  ', '.join('r_%s_b%d' % (nme, b) for b in range(nb))))
          for i in range(s.n_edge):
            # lane 0's cell and lane 63's lie in different banks as a rule:
            # one load each, the other lanes' offsets out of range
            left, right = edge_cell_banks(i, s.V, nb)
            self.w('      { %s e1[1], e2[1]; soda_buf_load_cell_banked<%s, %d>('
                   'e1, r_%s_b%d, lane == 0 ? %s + exb%d_%d : SODA_OOB_X); '
                   'soda_buf_load_cell_banked<%s, %d>(e2, r_%s_b%d, lane == 0 '
                   '? SODA_OOB_X : %s + exb%d_%d); %s_e[%d] = lane == 0 ? '
                   'e1[0] : e2[0]; }' %
                   (n.ctype, n.ctype, nb, nme, left, ro, i, es,
                    n.ctype, nb, nme, right, ro, i, es, reg, i))
          continue
        self.w('      soda_buf_load_frag<%s, %d, %s>(%s, r_%s, %s + xb%d%s);' %
          (n.ctype, s.V, s.nt_l, reg, nme, ro, es, pinned))
        for i in range(s.n_edge):
          self.w('      { %s e1[1]; soda_buf_load_frag<%s, 1, false>(e1, r_%s, %s + '
            'exb%d_%d); %s_e[%d] = e1[0]; }' %
            (n.ctype, n.ctype, nme, ro, i, es, reg, i))

  def _emit_wave(self, wv: int) -> None:
    """The tick loop of one wave of the block (the only one unless the
    block is stage-pipelined)."""
    s = self.s
    if s.W > 1:
      self.w('  if (wave == %d) {  // iterations %d..%d of the chain' %
             (wv, wv * (s.T // s.W), (wv + 1) * (s.T // s.W) - 1))
    self._emit_decls(wv)
    # The first `lead` ticks of a chunk only fill the prefetch queue: nothing a
    # stage could compute then reaches an output plane (every stage lags its
    # inputs by at least the prefetch depth), so they are peeled into a
    # load-only prologue whose slot phases continue into tick 0 of the loop.
    self.w('  int tau = m_begin + (%d);' % (s.m_lo + s.lead))
    if wv == 0:
      for i in range(s.lead):
        self.w('    {  // prologue: loads of plane tau - %d' % (s.lead - i))
        self._emit_loads((i - s.lead) % s.U, 'tau - %d' % (s.lead - i))
        self.w('    }')
    self.w('  const int tau_end = m_end + %d;' % s.max_delay)
    if s.peeled:
      self.w('  {  // warm-up: %d row steps, stages enter as their rows start '
             'to matter' % s.peeled)
      for i in range(s.peeled):
        self._emit_tick(wv, i % s.U, step=i)
      self.w('  }')
      self.w('  tau += %d;' % s.peeled)
    for n in s.nodes:
      if id(n) in s.slide and n.owner == wv and not (
          s.peeled and s.stage_needed(n, s.peeled - 1)):
        # the stage's first step is the loop's first: set its accumulator up
        self.w('  {  // sliding sum of %s: the rows its window holds now' % n.var)
        self.w('    const int t = tau;')
        self._emit_stage(n, _Tick(0, len(self.L)), slide_init='only')
        self.w('  }')
    self.w('  for (; tau < tau_end; tau += %d) {' % s.U)
    for k in range(s.U):
      self._emit_tick(wv, k)
    self.w('  }')
    if s.W > 1:
      self.w('  }')

  def _emit_tick(self, wv: int, k: int, step: Optional[int] = None) -> None:
    """One row step at slot phase k; `step` = its number within the peeled
    warm-up (None: a step of the loop)."""
    s = self.s
    at = k if step is None else step
    self.w('    {  // tick %d of %d' % (k, s.U))

    if s.W > 1 and k % s.R == 0:
      self.w('      soda_pipe_barrier();')
    if wv == 0:
      self._emit_loads(k, 'tau + %d' % at, pin=step is not None)
    else:
      self.w('      const int t = tau + %d;' % at)
    for n in s.nodes:
      if n.mirror_of is not None and n.owner == wv:
        # the plane the previous wave wrote R ticks (one barrier) ago
        for j in s.rows_of(n):
          self.w('      soda_load_frag<%s, %d, false>(%s, &soda_ring_%s'
                 '[(t + %d) & %d][%d][lane * %d]);' %
                 (n.ctype, s.V, self._reg(n, s.slot_of(n, k, 0), j),
                  n.mirror_of.var, s.R, 2 * s.R - 1, j, s.V))
    # 2. compute every tensor's new plane
    tick = _Tick(k, len(self.L))
    # (tensor, slot) whose end cells change hands at the end of this step: the
    # planes computed in it, and the input plane whose load it is first to use
    fresh_xs: List[Tuple[_Node, int]] = []
    if s.xs and wv == 0:
      for n in s.inputs.values():
        if n.xs:
          fresh_xs.append((n, s.slot_of(n, k, s.PF)))
      # the neighbours' end cells of the planes handed over at the end of the
      # previous step: one LDS read per tensor, row r in lanes r and 32 + r
      # (stale or unwritten values reach only planes no output depends on)
      for n in s.nodes:
        if not n.xs:
          continue
        slot = s.slot_of(n, k - 1, s.PF if n.is_input else 0)
        self.w('      hv_%s_s%d = soda_xs_%s[xs_rd < %d ? xs_rd + ((t - 1) & 1) * %d '
               ': xs_rd];' % (n.var, slot, n.var, 2 * s.xs_stride,
                              s.xs_stride))
    for n in s.nodes:
      if n.stage is not None and n.owner == wv:
        if step is not None and not s.stage_needed(n, step):
          continue
        first = step is not None and (step == 0 or
                                      not s.stage_needed(n, step - 1))
        self._emit_stage(n, tick, slide_init='first' if first else None)
        if n.xs:
          fresh_xs.append((n, s.slot_of(n, k, 0)))
    self.shift_temps = max(self.shift_temps, len(tick.shifted))
    if fresh_xs:
      # x-halo hand-over of the planes computed (first read, for an input) in
      # this step: lanes 0 and 63 put their end cells into LDS; the barrier
      # also keeps the next write of this parity behind every wave's reads
      self.w('      if (edge_lane) {')
      for n, slot in fresh_xs:
        for jj, j in enumerate(s.rows_of(n)):
          reg = self._reg(n, slot, j)
          self.w('        soda_xs_%s[xs_wr + (t & 1) * %d + %d] = lane == 0 ? %s[0] '
                 ': %s[%d];' % (n.var, s.xs_stride, jj, reg, reg, s.V - 1))
      self.w('      }')
      self.w('      soda_pipe_barrier();')
    self.w('    }')

  # -- one tensor's new plane ---------------------------------------------------
  def _operand(self, tick: _Tick, n: _Node, pname: str, off: Tuple[int, ...],
               j: int, e: int) -> str:
    """The text of cell `e` + off[0] of row `j` (+ off[1]) of the plane of
    parent `pname` that stage `n` taps at `off`; lane-shifted copies and
    widened bytes are declared in `tick.pre` / `tick.early`, once per step."""
    s = self.s
    p = n.parents[pname]
    age = n.delay - off[s.ax] - p.fill_delay
    slot = s.slot_of(p, tick.k, age)
    row = j + (off[1] if s.dim == 3 else 0)
    if row < p.rmargin[0] or row >= s.rows_in - p.rmargin[1]:
      raise util.InternalError('march: row %d of %s is not held' %
                               (row, p.var))
    reg = self._reg(p, slot, row)
    c = e + off[0]
    lane_off, sub = c // s.V, c % s.V
    src = '%s[%d]' % (reg, sub)
    # one-byte cells enter an expression as the int C promotes them to, with
    # the value range hidden from the compiler (soda_rt.h soda_wide: hipcc's
    # packed-byte instruction selection is wrong in places), once per cell
    # and tick
    byte = p.ctype in ('uint8_t', 'int8_t')

    def wide(text: str, tag: str) -> str:
      if not byte:
        return text
      if tag not in tick.wide:
        tick.wide[tag] = 'w%d_%s' % (len(tick.wide), tag)
        tick.pre.append('      const int %s = soda_wide(%s);' %
                        (tick.wide[tag], text))
      return tick.wide[tag]

    if lane_off == 0:
      return wide(src, '%s_e%d' % (reg, sub))
    key = (p.var, slot, row, sub, lane_off)
    if key not in tick.shifted:
      tmp = 'sh_%s_e%d_%s%d' % (reg, sub, 'm' if lane_off < 0 else 'p',
                                abs(lane_off))
      if (p.is_input and s.n_edge) or p.xs:
        if abs(lane_off) != 1:
          raise util.InternalError('march: edge loads reach one lane')
        # cell index relative to the strip end, served by the edge lane
        ei = (-c - 1) if lane_off < 0 else (c - s.V)
        if p.xs:
          # broadcast from the halo vector of the plane (a scalar register)
          rr = row - p.rmargin[0] + (0 if lane_off < 0 else 32)
          old = ('soda_bcast(hv_%s_s%d, %d)' % (p.var, slot, rr)
                 if ei == 0 else '(%s)0' % p.ctype)
        else:
          old = '%s_e[%d]' % (reg, ei) if 0 <= ei < s.n_edge else \
              '(%s)0' % p.ctype
        expr = ('soda_lane_dn_or(%s, %s)' if lane_off < 0 else
                'soda_lane_up_or(%s, %s)') % (src, old)
      elif s.use_mix and lane_off > 0:
        expr = src
        for _ in range(lane_off):
          expr = 'soda_lane_up32(%s)' % expr
      else:
        expr = src
        for _ in range(abs(lane_off)):
          expr = ('soda_lane_dn(%s)' if lane_off < 0 else
                  'soda_lane_up(%s)') % expr
      line = '      const %s %s = %s;' % (p.ctype, tmp, expr)
      # a shift of a row produced in an EARLIER tick can be issued ahead
      # of the previous stage's arithmetic (latency hidden behind it)
      early = s.use_mix and lane_off > 0 and (
          p.is_input or age > 0) and not (p.is_input and s.n_edge) \
          and not p.xs
      (tick.early if early else tick.pre).append(line)
      tick.shifted[key] = tmp
    return wide(tick.shifted[key], tick.shifted[key])

  def _emit_stage(self, n: _Node, tick: _Tick,
                  slide_init: Optional[str] = None) -> None:
    """One tensor's new plane in the row step `tick`: lane-shifted operands
    first (shared by the stages of a tick), then one statement per cell.
    `slide_init` (sliding sums only): 'first' -- this is the stage's first
    step, set the accumulator up in front of it; 'only' -- emit nothing but
    that set-up (the first step is the loop's first)."""
    s = self.s
    tick.pre, tick.early = [], []
    dst_slot = s.slot_of(n, tick.k, 0)
    if id(n) in s.slide:
      body = self._slide_body(n, tick, dst_slot, slide_init)
      if slide_init == 'only':
        self.L.extend(tick.early)     # (shifts on the LDS pipe: nothing to hide behind here)
        self.L.extend(tick.pre)
        self.L.extend(body)
        return
    elif id(n) in s.xwin:
      body = self._xwindow_body(n, tick, dst_slot)
    else:
      body = self._statement_body(n, tick, dst_slot)
    if tick.early:
      # place them in front of the previous stage's block of this tick.
      # (The compiler sinks each to one stage's arithmetic ahead of its use,
      # one swizzle in flight at a time.  Round 4 pinned all 13 of a T=13 step
      # at the head of the step behind a scheduling barrier -- 13 in flight,
      # 162 VGPRs, bit-exact -- and gained nothing: T12 145-146 us either way,
      # T13 170 against 156-161, profiles/r04_early_*.json.  The swizzles'
      # latency is not what the step waits for.)
      self.L[tick.mark:tick.mark] = tick.early
    if n.keep is not None:
      body += self._keep_body(n, tick, dst_slot)
    tick.mark = len(self.L)
    self.L.extend(tick.pre)
    self.L.extend(body)
    self._emit_own_registers(n, dst_slot)
    self._emit_to_lds(n, dst_slot)
    if n.store_slot is not None:
      self._emit_store(n, n.stage.name, dst_slot, tick.k)

  def _slide_body(self, n: _Node, tick: _Tick, dst_slot: int,
                  slide_init: Optional[str]) -> List[str]:
    """A sliding sum along the streamed dimension (Schedule.slide)."""
    s = self.s
    pname, off, taps = s.slide[id(n)]
    body: List[str] = []
    for j in s.rows_of(n):
      acc = 'xa_%s_r%d' % (n.var, j)
      for e in range(s.V):
        def tap(i, _j=j, _e=e):
          o = list(off)
          o[s.ax] = off[s.ax] + i
          return '(int)%s' % self._operand(tick, n, pname, tuple(o), _j, _e)
        if slide_init:
          body.append('      %s[%d] = %s;' % (acc, e, ' + '.join(
              tap(i) for i in range(taps - 1))))
        if slide_init != 'only':
          body.append('      %s[%d] += %s;' % (acc, e, tap(taps - 1)))
          body.append('      %s[%d] = (%s)%s[%d];' %
                      (self._reg(n, dst_slot, j), e, n.ctype, acc, e))
          body.append('      %s[%d] -= %s;' % (acc, e, tap(0)))
    return body

  def _xwindow_body(self, n: _Node, tick: _Tick, dst_slot: int) -> List[str]:
    """A window of `taps` cells along dimension 0 (Schedule.xwin), for the V
    cells of a lane at once: the V + taps - 1 cells the lane's windows cover
    are brought into the lane ONCE (whole fragments of the lanes to the right:
    ~ (taps - 1) lane moves instead of a move per tap per cell), then

      +        out[0] = the first window, out[e + 1] = out[e] + in[e + taps]
               - in[e]: taps - 1 + 2 (V - 1) operations for V cells, in int32
               (exact: the values are narrower than 32 bits, windows.py);
      min/max  in blocks of b = min(V, taps) cells: the windows of a block
               share the middle cells in[e0+b-1 .. e0+taps-1]; suffix
               reductions of in[e0 .. e0+b-2] and prefix reductions of
               in[e0+taps .. e0+taps+b-2] complete them: ~ taps + 3 b
               operations per block.  (One block only when V <= taps; with
               more cells per lane than taps -- uint8: 16 -- no cell is common
               to all V windows.)

    Integer arithmetic in any order gives the same bits as the statement's
    left-to-right text; the statement's cast is applied per cell as before."""
    s = self.s
    op, pname, off, taps = s.xwin[id(n)]
    V = s.V
    body: List[str] = []
    for j in s.rows_of(n):
      tag = '%s_k%d_r%d' % (n.var, dst_slot, j)
      cells = []
      for i in range(V + taps - 1):
        o = list(off)
        o[0] = off[0] + i
        cells.append(self._operand(tick, n, pname, tuple(o), j, 0))
      dst = ['%s[%d]' % (self._reg(n, dst_slot, j), e) for e in range(V)]
      body.append('      {')
      if op == '+':
        body.append('        int xw_%s = %s;' % (tag, ' + '.join(
            '(int)%s' % c for c in cells[:taps])))
        body.append('        %s = (%s)xw_%s;' % (dst[0], n.ctype, tag))
        for e in range(1, V):
          body.append('        xw_%s = xw_%s + (int)%s - (int)%s;' %
                      (tag, tag, cells[e + taps - 1], cells[e - 1]))
          body.append('        %s = (%s)xw_%s;' % (dst[e], n.ctype, tag))
      else:
        fn = 'SODA_MIN' if op == 'min' else 'SODA_MAX'
        pt = s.st.symbol_table[pname].c_type
        # blocks of at most `taps` cells: the windows of cells e0 .. e0+b-1
        # all contain in[e0+b-1 .. e0+taps-1] (b <= taps, so never empty)
        for blk, e0 in enumerate(range(0, V, taps)):
          b = min(taps, V - e0)
          lo, hi = e0 + b - 1, e0 + taps - 1
          btag = '%s_b%d' % (tag, blk)
          mid = '(%s)%s' % (pt, cells[lo])
          for c in cells[lo + 1:hi + 1]:
            mid = '%s((%s)%s, %s)' % (fn, pt, c, mid)
          body.append('        const %s xm_%s = %s;' % (pt, btag, mid))
          # suffix reductions of the cells below the middle block ...
          suf = {}
          prev = None
          for i in range(lo - 1, e0 - 1, -1):
            name = 'xs_%s_%d' % (btag, i)
            expr = '(%s)%s' % (pt, cells[i]) if prev is None else \
                '%s((%s)%s, %s)' % (fn, pt, cells[i], prev)
            body.append('        const %s %s = %s;' % (pt, name, expr))
            suf[i] = prev = name
          # ... and prefix reductions of the cells above it
          pre = {}
          prev = None
          for i in range(hi + 1, e0 + b + taps - 1):
            name = 'xp_%s_%d' % (btag, i)
            expr = '(%s)%s' % (pt, cells[i]) if prev is None else \
                '%s(%s, (%s)%s)' % (fn, prev, pt, cells[i])
            body.append('        const %s %s = %s;' % (pt, name, expr))
            pre[i] = prev = name
          for e in range(e0, e0 + b):
            parts = ['xm_%s' % btag]
            if e < lo:
              parts.append(suf[e])
            if e + taps - 1 > hi:
              parts.append(pre[e + taps - 1])
            expr = parts[0]
            for q in parts[1:]:
              expr = '%s(%s, %s)' % (fn, expr, q)
            body.append('        %s = (%s)(%s);' % (dst[e], n.ctype, expr))
      body.append('      }')
    return body

  def _statement_body(self, n: _Node, tick: _Tick, dst_slot: int) -> List[str]:
    """The stage's statement as written, once per cell (with its `let`s)."""
    s = self.s
    stage = n.stage
    body: List[str] = []
    for j in s.rows_of(n):
      for e in range(s.V):

        def load(ref: ir.Ref, _e=e, _j=j) -> str:
          prm = self.mod.param_load(ref)
          if prm is not None:
            return prm
          off = tuple(a - b for a, b in zip(ref.idx, stage.st_idx))
          return self._operand(tick, n, ref.name, off, _j, _e)

        dst = '%s[%d]' % (self._reg(n, dst_slot, j), e)
        if stage.stmt.let:
          body.append('      {')
          for let in stage.stmt.let:
            body.append('        const %s %s = %s;' %
                        (let.haoda_type.c_type, let.name,
                         ir.c_expr(let.expr, load, self.mod.param_var)))
          body.append('        %s = (%s)(%s);' %
                      (dst, n.ctype, ir.c_expr(stage.stmt.expr, load,
                                               self.mod.param_var)))
          body.append('      }')
        else:
          body.append('      %s = (%s)(%s);' %
                      (dst, n.ctype, ir.c_expr(stage.stmt.expr, load,
                                               self.mod.param_var)))
    return body

  def _keep_body(self, n: _Node, tick: _Tick, dst_slot: int) -> List[str]:
    """border: preserve -- cells one iteration cannot compute keep the value
    of the input this output replaces (same cell, previous iteration)."""
    s = self.s
    wlo, whi = s.st.interior_bounds(n.stage.name)
    zero = (0,) * s.dim
    body = ['      {']
    body.append('        const int mk = a.origin[%d] + t - %d;  // global plane'
                % (s.ax, n.delay))
    body.append('        const bool keep_m = !(mk >= %d && mk < a.gextent[%d] - '
                '%d);' % (max(0, -wlo[s.ax]), s.ax, max(0, whi[s.ax])))
    for j in s.rows_of(n):
      keep_row = 'keep_m'
      if s.dim == 3:
        body.append('        const bool keep_r%d = keep_m || !(a.origin[1] + '
                    'y0 + %d >= %d && a.origin[1] + y0 + %d < a.gextent[1] - '
                    '%d);' % (j, j, max(0, -wlo[1]), j, max(0, whi[1])))
        keep_row = 'keep_r%d' % j
      for e in range(s.V):
        dst = '%s[%d]' % (self._reg(n, dst_slot, j), e)
        body.append('        %s = (%s || keepx_%s_%d) ? %s : %s;' %
                    (dst, keep_row, n.stage.name, e,
                     self._operand(tick, n, n.keep, zero, j, e), dst))
    body.append('      }')
    return body

  def _emit_own_registers(self, n: _Node, dst_slot: int) -> None:
    s = self.s
    if s.st.symbol_table[n.stage.name].size_in_bytes == 1:
      # every cell of a one-byte tensor through a register of its own: left to
      # itself the compiler packs the cells of a row into one register, and one
      # of its instruction-selection combines on that form is wrong on gfx950
      # (ROCm 7.2: a min whose operands come out of the packed register picked
      # the wrong side in one cell of one unrolled step of a fused kernel --
      # tools/fuzz_scan.py options, seed 613; exact with the pass that selects
      # instructions run unoptimised)
      for j in s.rows_of(n):
        self.w('      soda_own_register<%s, %d>(%s);' %
               (n.ctype, s.V, self._reg(n, dst_slot, j)))

  def _emit_to_lds(self, n: _Node, dst_slot: int) -> None:
    s = self.s
    if n.to_lds:   # hand the new plane to the next wave of the block
      for j in s.rows_of(n):
        self.w('      soda_store_frag<%s, %d, false>(&soda_ring_%s[t & %d][%d]'
               '[lane * %d], %s);' %
               (n.ctype, s.V, n.var, 2 * s.R - 1, j, s.V,
                self._reg(n, dst_slot, j)))

  def _emit_store(self, n: _Node, oname: str, dst_slot: int, k: int) -> None:
    """Stores the new plane of a last-iteration output (rows and lanes that
    are not this wave's to write are dropped by the addressing).  A twin also
    takes the plane's share of the residual: per cell, the decision the
    addressing makes implicitly -- the plane is one of the chunk's (m_ok), the
    row one of the tile's and of the grid's, the lane one that stores
    (store_ok, in rsx) -- as a boolean, and inside the pair's box.  Chunks,
    tiles and the storing lanes of strips partition the grid, so a cell
    counts once whatever overlaps the wave computes."""
    s = self.s
    es = s.esz[oname]
    self.w('      {')
    self.w('        const int m = t - %d;' % n.delay)
    self.w('        const bool m_ok = m >= m_begin && m < m_end;')
    if n.prev is not None:
      pair = s.st.output_names.index(oname)
      prev = n.parents[n.prev]
      pslot = s.slot_of(prev, k, n.delay - prev.fill_delay)
      self.w('        const bool rs_m = m_ok && m >= soda_box.lo[%d][%d] && m < '
             'soda_box.hi[%d][%d];' % (pair, s.ax, pair, s.ax))
      for j in s.store_rows(n):
        if j < prev.rmargin[0] or j >= s.rows_in - prev.rmargin[1]:
          raise util.InternalError('march: row %d of %s is not held' %
                                   (j, prev.var))
        row = 'rs_m'
        if s.dim == 3:
          # (the box lies inside the grid: a row in it is a row that exists)
          self.w('        const bool rs_r%d = rs_m && y0 + %d >= soda_box.lo[%d][1] '
                 '&& y0 + %d < soda_box.hi[%d][1];' % (j, j, pair, j, pair))
          row = 'rs_r%d' % j
        for e in range(s.V):
          self.w('        soda_res_add(soda_acc, %s[%d], %s[%d], '
                 '%s && rsx%d_%d);' % (self._reg(n, dst_slot, j), e,
                                      self._reg(prev, pslot, j), e, row, pair,
                                      e))
    for j in s.store_rows(n):
      reg = self._reg(n, dst_slot, j)
      if oname in s.banks:
        nb = s.banks[oname]
        self.w('        soda_buf_store_frag_banked<%s, %d, %d, %s>(%s, %s, %s);' %
               (n.ctype, s.V, nb, s.nt_s, self._store_row(es, j), reg,
                ', '.join('w_%s_b%d' % (oname, b) for b in range(nb))))
        continue
      self.w('        soda_buf_store_frag<%s, %d, %s>(w_%s, %s, %s);' %
             (n.ctype, s.V, s.nt_s, oname, self._store_row(es, j), reg))
    self.w('      }')

  # -- after the text -----------------------------------------------------------
  def _check_emitted(self) -> None:
    """The one refusal that counts what emission produced."""
    if self.shift_temps > MAX_SHIFT_TEMPS:
      raise util.SemanticError(
          'march: %d lane-shifted operands per row step (> %d); the taps reach '
          'too far along dim 0 for %d cells per lane' %
          (self.shift_temps, MAX_SHIFT_TEMPS, self.s.V))

  def _launch_model(self):
    """(step_ops, warm_saved, tile, lds_rings, lds_pad) of the launch-time
    model (include/soda_hip.h, soda_hip_kernel_desc_t): vector instructions
    one row step of the busiest wave issues, the part of the warm-up the
    peeled steps skip, in row steps, the tile a block covers and its LDS."""
    s, cfg = self.s, self.cfg
    stages = [n for n in s.nodes if n.stage is not None]
    per_wave = []
    for wv in range(s.W):
      ops = 0.0
      for n in stages:
        if n.owner != wv:
          continue
        cost = sum(ir.op_count(l.expr) for l in n.stage.stmt.let) + \
            ir.op_count(n.stage.stmt.expr) + 0.5
        wide = 2.0 if n.ctype in ('double', 'int64_t', 'uint64_t') else 1.0
        ops += cost * wide * s.V * len(s.rows_of(n))
      per_wave.append(ops + 8.0)
    step_ops = max(per_wave)
    saved = sum(1 for i in range(s.peeled) for n in stages
                if not s.stage_needed(n, i)) / float(max(1, len(stages)))
    if s.dim == 2:
      tile = (s.strip_cells * (s.xs or s.wx), cfg.chunk_rows * cfg.waves_y)
    else:
      tile = (s.strip_cells * (s.xs or 1), s.tile_rows, cfg.chunk_rows)
    if s.seg:
      tile = (s.seg_cells,) + tile[1:]
    # the rings a stage-pipelined block declares (the cells x-halo sharing
    # hands over are a few hundred bytes more, not counted: `lds_rings`)
    table = s.st.symbol_table
    lds_rings = sum(
        2 * s.R * s.rows_in * 64 * s.V *
        table[n.key[1] if n.key[0] == 'in' else n.key[0]].size_in_bytes
        for n in s.nodes if n.to_lds)
    lds_pad = 0
    if cfg.occupancy:
      blocks_per_cu = max(1, 4 * cfg.occupancy // s.waves)
      # smallest allocation of which blocks_per_cu + 1 no longer fit -- of
      # which the block's own rings are a part: the pad is what is missing
      # beside them (on top of them, 64 KiB beside the 24 KiB of jacobi2d
      # T = 12 pipe 4 x 4 asked for 88 KiB a block where 81 KiB were meant; an
      # MI355X accepts such a launch -- 160 KiB a block -- and ran it right)
      need = (LDS_PER_CU // (blocks_per_cu + 1)) // 1024 * 1024 + 1024
      lds_pad = min(65536, max(0, need - lds_rings))
    return step_ops, saved, tile, lds_rings, lds_pad

  def _register(self, step_ops: float, saved: float, tile, lds_rings: int,
                lds_pad: int) -> PassDesc:
    """Adds the kernel and its pass to the module."""
    s, cfg = self.s, self.cfg
    est_regs = s.est_regs + self.shift_temps
    idx = self.mod.add_kernel(
        KernelDesc(s.name, (s.block, 1, 1), tile, lds_bytes=lds_pad,
                   note='%s %s' % (s.kind, cfg.key()),
                   tune=dict(axis=s.ax, waves_along=cfg.waves_y if s.dim == 2 else 1,
                             waves_per_block=s.waves, warm=s.warm,
                             fixed=cfg.chunk_fixed, occupancy=cfg.occupancy,
                             lds_rings=lds_rings, lds_pad=lds_pad,
                             pipe=s.W, vec=s.V, step_ops=step_ops,
                             lane_shift=cfg.lane_shift,
                             warm_saved=saved,
                             lane_redundancy=s.lane_redundancy,
                             peel_trips=s.peeled // s.U,
                             unroll=s.U, tile_rows=s.tile_rows,
                             peel_trips_max=s.peel_trips_max,
                             fused=s.T,
                             window_extra=s.m_hi - s.m_lo,
                             max_elem=max(s.esz.values()),
                             max_extent0=0 if s.seg else
                             s.strip_cells * s.xs)),
        '\n'.join(self.L) + '\n')
    table = s.st.symbol_table
    bytes_in = sum(table[i].size_in_bytes for i in s.st.input_names)
    bytes_out = sum(table[o].size_in_bytes for o in s.st.output_names)
    redundancy = s.lane_redundancy * (
        (cfg.chunk_rows + s.warm) / float(cfg.chunk_rows)) * (
            s.rows_in / float(s.tile_rows))
    p = PassDesc(
        s.T, [idx], s.kind,
        dict(bytes_per_cell_min=bytes_in + bytes_out,
             read_redundancy=redundancy, strip_cells=s.strip_cells, warm_rows=s.warm,
             unroll=s.U, edge=s.edge, rows_in=s.rows_in, tile_rows=s.tile_rows,
             est_window_regs=est_regs))
    self.mod.passes.append(p)
    return p


def add_march_twin(mod: Module, cfg: MarchConfig) -> Optional[int]:
  """Adds the residual twin of the marching kernel `cfg` built last (a kernel,
  not a pass: the library launches it in place of its plain kernel) and names
  it in that kernel's descriptor; None, and nothing added, where the form has
  no twin or the extra window does not fit."""
  import copy
  plain = '%s_march%dd_%s' % (mod.stencil.app_name, mod.stencil.dim, cfg.key())
  owner = [k for k in mod.kernels if k.name == plain]
  if len(owner) != 1:
    raise util.InternalError('march: no kernel %s to build a twin of' % plain)
  twin_cfg = copy.copy(cfg)
  twin_cfg.residual = True
  keep = (len(mod.kernels), len(mod.passes), len(mod.chunks))
  try:
    p = _MarchKernel(mod, twin_cfg).emit()
  except util.SemanticError:
    del mod.kernels[keep[0]:], mod.passes[keep[1]:], mod.chunks[keep[2]:]
    return None
  mod.passes.remove(p)
  owner[0].twin = p.kernels[0]
  mod.kernels[p.kernels[0]].tune['twin_of'] = plain
  mod.kernels[p.kernels[0]].tune['est_window_regs'] = \
      p.traffic_model['est_window_regs']
  return p.kernels[0]


def add_march_pass(mod: Module, cfg: MarchConfig) -> PassDesc:
  """Adds one marching kernel (and its pass) for `cfg.fused_iters` iterations;
  raises SemanticError if the program or the shape does not fit."""
  return _MarchKernel(mod, cfg).emit()
