"""The schedule of a marching kernel (`march2d` / `march3d`): what the kernel
IS -- the T-times unrolled stage chain, the strip and tile geometry, the
register windows, the warm-up -- as data, built by named steps before any text
exists.  march.py spells it in HIP and only reads it; nothing here writes
text, and nothing there decides geometry."""
from typing import Callable, Dict, List, Optional, Tuple

from soda_amd import core, util

MAX_UNROLL = 24        # tallest register window (planes) a marching wave holds
MAX_FUSE_PRESERVE = 8      # deepest temporal blocking under `border: preserve`
MAX_FUSE_3D = 2            # deepest temporal blocking of the 3-D kernels
MAX_SHIFT_TEMPS = 64       # lane-shifted operand copies per row step
REG_BUDGET = 160           # estimated VGPRs (windows + shifted copies) a shape may need

MIRROR_PREFETCH = 1         # ticks between a mirror's LDS read and its first use


class _Node:
  """A tensor of the T-times unrolled chain."""

  def __init__(self, key, ctype: str, stage: Optional[core.Stage], it: int):
    self.key = key              # ('in', name) or (stage name, iteration)
    self.ctype = ctype
    self.stage = stage          # None for a global input
    self.it = it
    self.parents: Dict[str, '_Node'] = {}   # DSL name -> node
    self.delay = 0              # ticks between issue of input plane t and plane t here
    self.first_use = None       # age of the youngest plane any child reads
    self.window = 1             # planes (rows in 2-D) kept
    self.slots = 1              # window padded to a divisor of the unroll
    self.margin = [0, 0]        # invalid cells at the low/high end of a strip
    self.rmargin = [0, 0]       # 3-D: invalid rows at the low/high end of a tile
    self.store_slot: Optional[int] = None   # plan slot if stored to memory
    # stage-pipelined blocks: the wave that owns (computes / loads) the tensor;
    # a `mirror` is the copy a wave keeps of a tensor the previous wave of the
    # block produces, filled from the LDS ring one tick after its production
    self.owner = 0
    self.mirror_of: Optional['_Node'] = None
    self.to_lds = False         # some wave mirrors this tensor
    # border: preserve -- DSL name of the input whose value this output keeps
    # on cells one iteration cannot compute (it is then also a parent, tapped
    # at offset 0)
    self.keep: Optional[str] = None
    # residual twins: DSL name of the input this output of the LAST fused
    # iteration replaces -- a parent tapped at offset 0, like `keep` (and the
    # same tensor where both are set), for |cur - prev| where it is stored
    self.prev: Optional[str] = None
    # x-halo sharing: the strip's neighbours hand this tensor's end cells over
    # through LDS (one register per row slot holds them, like edge loads)
    self.xs = False
    # segmented x-halo sharing: invalid cells at the two OUTER ends of the
    # block's segment, the sides no wave of the block hands cells over to
    # (`margin` then describes the sides between the block's waves)
    self.omargin = [0, 0]

  def tap_bounds(self, pname: str):
    """Bounds of the taps on parent `pname`, the offset-0 tap of a preserved
    border included."""
    dim = len(self.stage.st_idx)
    if pname in self.stage.taps:
      lo, hi = self.stage.tap_bounds(pname)
    else:
      lo, hi = (0,) * dim, (0,) * dim
    if pname == self.keep or pname == self.prev:
      lo = tuple(min(0, v) for v in lo)
      hi = tuple(max(0, v) for v in hi)
    return lo, hi

  @property
  def is_input(self) -> bool:
    return self.stage is None and self.mirror_of is None

  @property
  def fill_delay(self) -> int:
    """Ticks between the issue of input plane t and the tick at which plane t
    of THIS tensor is put into its register slot (loaded, read from LDS or
    computed).  Loads are put in flight `delay` ticks before they are used."""
    if self.mirror_of is not None:
      return self.delay - MIRROR_PREFETCH
    return 0 if self.stage is None else self.delay

  @property
  def var(self) -> str:
    if self.mirror_of is not None:
      return 'm%d_%s' % (self.owner, self.mirror_of.var)
    if self.stage is None:
      return 'g_%s' % self.key[1]
    return 't%d_%s' % (self.it, self.stage.name)


def bank_fragment_map(vec: int, nb: int) -> List[Tuple[int, int]]:
  """(bank, element of the lane's piece of that bank) of every cell of a
  fragment of `vec` cells that starts on a bank-group boundary (`nb` divides
  its first stream element): stream element k is bank k % nb, index k / nb.
  A restatement, for the record and for the CPU test against numpy's strided
  views, of what soda_buf_load_frag_banked / _store_frag_banked
  (csrc/soda_rt_banked.h: `dst[j * NB + b] = part[j]`) do in registers: the
  generator calls it only to refuse a `vec` that is no whole number of bank
  groups and emits no code from it, so the helpers themselves are guarded by
  the GPU cases of tests/test_wire_banked.py, not by this function."""
  if nb < 1 or vec % nb:
    raise util.SemanticError(
        'banks: %d cells per lane are no whole number of groups of %d banks' %
        (vec, nb))
  return [(j % nb, j // nb) for j in range(vec)]


def march_supported(stencil: core.Stencil) -> Optional[str]:
  """None if the marching kernels can run the program, else why not."""
  if stencil.dim not in (2, 3):
    return 'the marching kernels need a 2- or 3-dimensional program'
  return None


def _build_chain(st: core.Stencil, T: int, pf: int, edge: Tuple[int, int],
                 pipe: int = 1, pipe_rows: int = 1, xshare: bool = False,
                 residual: bool = False):
  """The tensors of T chained iterations with their schedule (delay in ticks
  behind the load of the input plane, window of planes kept, invalid margins).
  `pipe` > 1 splits the iterations evenly over that many waves of a block:
  a tensor consumed by the next wave gets a mirror there (see _Node)."""
  dim = st.dim
  ax = dim - 1                         # march axis
  table = st.symbol_table
  per_wave = T // pipe
  nodes: List[_Node] = []
  inputs = {}
  for name in st.input_names:
    n = _Node(('in', name), table[name].c_type, None, -1)
    n.delay = pf
    n.margin = [-edge[0], -edge[1]]    # edge lanes fetch that many halo cells
    n.omargin = [-edge[0], -edge[1]]
    inputs[name] = n
    nodes.append(n)
  cur_inputs = dict(inputs)
  last_outputs = {}
  for it in range(T):
    owner = it // per_wave if pipe > 1 else 0
    env = {}
    for name, src in cur_inputs.items():
      if src.owner != owner:
        m = _Node(('mirror', src.key, owner), src.ctype, None, it)
        m.mirror_of = src
        m.owner = owner
        src.to_lds = True
        nodes.append(m)
        src = m
      env[name] = src
    for stage in st.ordered_stages:
      n = _Node((stage.name, it), stage.haoda_type.c_type, stage, it)
      n.owner = owner
      for parent in stage.taps:
        n.parents[parent] = env[parent]
      if st.preserve_border and stage.is_output:
        n.keep = st.preserved_from(stage.name)
        n.parents.setdefault(n.keep, env[n.keep])
      if residual and it == T - 1 and stage.is_output:
        # (under `border: preserve` the window is there already: `keep`)
        n.prev = st.input_names[st.output_names.index(stage.name)]
        n.parents.setdefault(n.prev, env[n.prev])
      env[stage.name] = n
      nodes.append(n)
    last_outputs = {o: env[o] for o in st.output_names}
    if it < T - 1:
      cur_inputs = {i: env[o] for i, o in zip(st.input_names, st.output_names)}
  def share(n: _Node) -> None:
    """x-halo sharing: if some consumer taps `n` off-centre along dim 0, the
    neighbouring strips hand its end cells over (one valid cell per side)."""
    reach = 0
    for c in nodes:
      if c.stage is None or c.mirror_of is not None:
        continue
      for pname, p in c.parents.items():
        if p is not n:
          continue
        tlo, thi = c.tap_bounds(pname)
        reach = max(reach, -tlo[0], thi[0])
        if tlo[0] < 0 or thi[0] > 0:
          # the halo cells of a plane arrive at the END of the row step that
          # computes it (or first reads it, for an input): taps off-centre in
          # x must not touch the newest plane the consumer reads
          newest = max(off[ax] for off in c.stage.taps.get(pname, ())
                       if off[0] != 0)
          if newest >= thi[ax]:
            raise util.SemanticError(
                'march: x-halo sharing needs a row step between a plane and '
                'its off-centre taps (%s reads %s)' % (c.var, n.var))
    if reach:
      # (`margin`: the sides a neighbouring strip of the block serves.  The
      # outer sides of a segment -- `omargin` -- have no neighbour and may
      # well be invalid: they are the overlap with the next block)
      if reach > 1 or n.margin[0] > 0 or n.margin[1] > 0:
        raise util.SemanticError(
            'march: x-halo sharing hands over one valid cell per side')
      n.xs = True
      n.margin = [n.margin[0] - 1, n.margin[1] - 1]

  if xshare:
    for n in inputs.values():
      share(n)
  # delays and margins, in chain order
  for n in nodes:
    if n.mirror_of is not None:
      src = n.mirror_of
      # read `pipe_rows` ticks (one barrier period) after it was written, used
      # MIRROR_PREFETCH ticks after that
      n.delay = src.delay + pipe_rows + MIRROR_PREFETCH
      n.margin = list(src.margin)
      n.omargin = list(src.omargin)
      n.rmargin = list(src.rmargin)
      continue
    if n.stage is None:
      continue
    delay = None
    margin = [0, 0]
    # (kept for every chain: without sharing nothing lowers `margin` and the
    # two are equal; only a segmented kernel reads `omargin`)
    omargin = [0, 0]
    rmargin = [0, 0]
    for pname, p in n.parents.items():
      tlo, thi = n.tap_bounds(pname)
      d = p.delay + thi[ax]
      delay = d if delay is None else max(delay, d)
      margin[0] = max(margin[0], p.margin[0] + max(0, -tlo[0]))
      margin[1] = max(margin[1], p.margin[1] + max(0, thi[0]))
      omargin[0] = max(omargin[0], p.omargin[0] + max(0, -tlo[0]))
      omargin[1] = max(omargin[1], p.omargin[1] + max(0, thi[0]))
      if dim == 3:
        rmargin[0] = max(rmargin[0], p.rmargin[0] + max(0, -tlo[1]))
        rmargin[1] = max(rmargin[1], p.rmargin[1] + max(0, thi[1]))
    n.delay = delay if delay is not None else 0
    n.margin = margin
    n.omargin = omargin
    n.rmargin = rmargin
    if xshare:
      share(n)
  # windows: a parent keeps planes from its newest (age 0) to the oldest any
  # child still reads
  for n in nodes:
    if n.stage is None:
      continue
    for pname, p in n.parents.items():
      tlo, thi = n.tap_bounds(pname)
      p.window = max(p.window, n.delay - tlo[ax] - p.fill_delay + 1)
      # the youngest plane of the parent any child reads (an input plane is
      # first touched that many ticks after its load was issued)
      first = n.delay - thi[ax] - p.fill_delay
      p.first_use = first if p.first_use is None else min(p.first_use, first)
  return nodes, inputs, last_outputs


def _choose_unroll(nodes: List[_Node], regs_per_plane: int,
                   multiple_of: int = 1) -> Optional[int]:
  max_w = max(n.window for n in nodes)
  best = None
  for u in range(max_w, MAX_UNROLL + 1):
    if u % multiple_of:
      continue
    divisors = [d for d in range(1, u + 1) if u % d == 0]
    pad = 0
    for n in nodes:
      slots = min(d for d in divisors if d >= n.window)
      pad += slots - n.window
    cost = pad * regs_per_plane + 2 * u
    if best is None or cost < best[0]:
      best = (cost, u)
  return None if best is None else best[1]


def _walk_back(nodes: List[_Node], seeds: Dict[int, object],
               push: Callable, merge: Callable) -> Dict[int, object]:
  """What every tensor of the chain is needed for, told backwards from the
  outputs: {id(node): value, None where no output depends on the tensor}.
  `seeds` holds the outputs' values.  In reverse chain order a tensor that has
  a value hands it on -- a mirror to its source as it is (the same planes,
  held by another wave), a stage to every parent as `push(value, tap lo, tap
  hi)` -- and a tensor told twice keeps `merge(old, new)`.  (A mirror stands
  behind every other consumer of its source in the chain, so its source has
  heard nothing yet when the mirror speaks.)"""
  got: Dict[int, object] = {id(n): None for n in nodes}
  got.update(seeds)
  for n in reversed(nodes):
    value = got[id(n)]
    if value is None:
      continue
    if n.mirror_of is not None:
      told = [(n.mirror_of, value)]
    elif n.stage is None:
      continue
    else:
      told = [(p, push(value, *n.tap_bounds(pname)))
              for pname, p in n.parents.items()]
    for p, new in told:
      cur = got[id(p)]
      got[id(p)] = new if cur is None else merge(cur, new)
  return got


class Schedule:
  """One marching kernel as data.  `cfg` is a march.MarchConfig; `banks` and
  `slot` are the module's bank counts and buffer slots.  The constructor calls
  the steps below in order; every refusal a shape can meet before its text is
  written is raised by one of them."""

  def __init__(self, st: core.Stencil, cfg, banks: Dict[str, int],
               slot: Dict[str, int]):
    self.st, self.cfg = st, cfg
    self._check_config(banks)
    self.edge, chain, halo = self._edge_cells()
    self.nodes, self.inputs, self.outputs = chain
    self.out_nodes = list(self.outputs.values())
    self._strip_geometry(halo)
    self._tile_rows()
    self._unroll_and_slots()
    self._estimate_registers()
    for o, n in self.outputs.items():
      n.store_slot = slot[o]
    self._first_planes()
    self._warm_up()
    self._name_and_block()
    self._tables()

  # -- the steps ---------------------------------------------------------------
  def _check_config(self, module_banks: Dict[str, int]) -> None:
    """Every refusal that needs only the program, the config and the module's
    bank slots; sets what the config alone decides."""
    st, cfg = self.st, self.cfg
    why = march_supported(st)
    if why:
      raise util.SemanticError('march: %s' % why)
    self.dim = st.dim
    self.ax = self.dim - 1
    self.T, self.V, self.PF = cfg.fused_iters, cfg.vec, cfg.prefetch
    if self.T > 1 and len(st.input_names) != len(st.output_names):
      raise util.SemanticError('march: cannot fuse iterations of a program '
                               'whose inputs and outputs differ in number')
    # lanes that form one strip: the whole wave, or each 32-lane half
    self.group = 32 if cfg.lane_shift == 'mixh' else 64
    # one wave per strip: the block is not several strips or chunks wide
    self.one_wave = cfg.waves_x * cfg.waves_y == 1
    self.W = cfg.pipe
    if self.W > 1 and (self.T % self.W or not self.one_wave):
      raise util.SemanticError(
          'march: %d pipelined waves need a fusion depth that is a multiple '
          'of it and one strip per block' % self.W)
    self.R = cfg.pipe_rows if self.W > 1 else 1
    self.banks = cfg.banks
    for nme, nb in self.banks.items():
      if module_banks.get(nme) != nb:
        raise util.InternalError('march: banks of `%s` and the module\'s slots '
                                 'differ' % nme)
      if self.W > 1:
        raise util.SemanticError(
            'march: stage-pipelined blocks read and write dense arrays')
      bank_fragment_map(self.V, nb)       # NB | V, or refused
    for nme in cfg.bank_lead:
      if nme not in self.banks or nme not in st.input_names or \
          cfg.bank_lead[nme] % self.banks[nme] or cfg.bank_lead[nme] < 0:
        raise util.SemanticError(
            'march: bank_lead of `%s`: a banked input, a multiple of its bank '
            'count' % nme)
    if self.R & (self.R - 1):
      raise util.SemanticError('march: rows per barrier must be a power of two')
    self.xs = cfg.xshare
    # segmented sharing: the block's waves cover a segment, not the row
    self.seg = bool(cfg.xshare_block)
    if self.seg:
      if not 2 <= cfg.xshare_block <= 16:
        raise util.SemanticError(
            'march: xshare_block = %d: 2 to 16 waves share a segment of a row'
            % cfg.xshare_block)
      self.xs = cfg.xshare_block
    if self.xs:
      if self.W > 1 or cfg.lane_shift != 'dpp' or not self.one_wave:
        raise util.SemanticError(
            'march: x-halo sharing needs DPP shifts and one wave per strip')
      if not 1 <= self.xs <= 16:
        raise util.SemanticError('march: 1 to 16 waves can share a row')
      if self.dim == 3 and cfg.tile_rows > 24:
        raise util.SemanticError('march: x-halo sharing holds a row per lane')
    if cfg.residual and (self.W > 1 or self.seg or self.banks or
                         not self.one_wave):
      raise util.SemanticError(
          'march: no residual twin of stage-pipelined blocks, segmented '
          'x-halo sharing, several waves per block or banked tensors')

  def _chain(self, edge: Tuple[int, int]):
    return _build_chain(self.st, self.T, self.PF, edge, self.W, self.R,
                        bool(self.xs), self.cfg.residual)

  def _halo_lanes(self, margin: Tuple[int, int]) -> Tuple[int, int]:
    return -(-margin[0] // self.V), -(-margin[1] // self.V)

  def _edge_cells(self):
    """(edge, chain, halo): the halo cells of the program inputs that the
    strip's edge lanes fetch with separate narrow loads (so a 1-iteration
    strip keeps all 64 lanes valid and its rows start on a 64*V-cell
    boundary), the chain built with them, and the halo cells (low, high) of a
    strip of that chain's outputs."""
    st, cfg = self.st, self.cfg
    edge = (0, 0)
    # (the edge cells enter through DPP's `old` operand; a stage-pipelined
    # block does without, and under x-halo sharing the inputs' halo cells
    # travel through LDS as well)
    if cfg.edge_loads and cfg.lane_shift == 'dpp' and self.W == 1 and \
        not self.xs:
      lo = hi = 0
      for stage in st.ordered_stages:
        for pname in stage.taps:
          if pname in st.input_names:
            tlo, thi = stage.tap_bounds(pname)
            lo, hi = max(lo, -tlo[0]), max(hi, thi[0])
      if max(lo, hi) <= min(self.V, 2):
        edge = (lo, hi)
    chain = self._chain(edge)
    outs = list(chain[2].values())
    halo = (max(0, max(n.margin[0] for n in outs)),
            max(0, max(n.margin[1] for n in outs)))
    if self.seg:     # the halo lanes of a segment are those of its outer sides
      halo = (max(0, max(n.omargin[0] for n in outs)),
              max(0, max(n.omargin[1] for n in outs)))
    if edge != (0, 0):
      # edge loads only pay when they save a halo lane.  The chain to compare
      # with is the plain one: one wave and no sharing, which is all a kernel
      # with edge cells can be, and without a twin's offset-0 parents, as it
      # always was built -- a twin's own margins stay out of the comparison.
      # Where the lanes are the same the kernel is the plain chain's, but
      # `halo`, the cells the header names, stays the first chain's.
      plain = _build_chain(st, self.T, self.PF, (0, 0), self.W, self.R)[2]
      p_halo = (max(n.margin[0] for n in plain.values()),
                max(n.margin[1] for n in plain.values()))
      if self._halo_lanes(p_halo) == self._halo_lanes(halo):
        edge = (0, 0)
        chain = self._chain(edge)
    return edge, chain, halo

  def _strip_geometry(self, halo: Tuple[int, int]) -> None:
    """Halo lanes of a strip (outer sides of a segment), the spare lanes
    `align_lanes` gives up, the cells a strip and a segment store."""
    cfg = self.cfg
    self.margin_lo, self.margin_hi = halo
    self.lanes_lo, self.lanes_hi = self._halo_lanes(halo)
    if cfg.align_lanes > 1 and self.group == 64:
      spare = (64 - self.lanes_lo - self.lanes_hi) % cfg.align_lanes
      if self.lanes_lo + self.lanes_hi + spare < 16:
        self.lanes_hi += spare
    if self.lanes_lo + self.lanes_hi >= self.group // 2:
      raise util.SemanticError('march: halo of %d+%d cells is too wide for a '
                               '%d-lane strip at %d cells per lane' %
                               (self.margin_lo, self.margin_hi, self.group,
                                self.V))
    self.group_lanes = self.group - self.lanes_lo - self.lanes_hi
    self.strip_lanes = self.group_lanes * (64 // self.group)
    self.strip_cells = self.strip_lanes * self.V
    # segmented sharing: cells a block stores, lanes of a block per lane that
    # stores
    self.seg_cells = (64 * self.xs - self.lanes_lo - self.lanes_hi) * self.V
    self.lane_redundancy = 64.0 / self.strip_lanes
    if self.seg:
      self.lane_redundancy = 64.0 * self.xs * self.V / self.seg_cells

  def _tile_rows(self) -> None:
    """3-D: rows (dim 1) of a tile held in registers."""
    if self.dim == 3:
      self.rhalo_lo = max(n.rmargin[0] for n in self.out_nodes)
      self.rhalo_hi = max(n.rmargin[1] for n in self.out_nodes)
      self.rows_in = self.cfg.tile_rows + self.rhalo_lo + self.rhalo_hi
    else:
      self.rhalo_lo = self.rhalo_hi = 0
      self.rows_in = 1
    self.tile_rows = self.rows_in - self.rhalo_lo - self.rhalo_hi

  def _unroll_and_slots(self) -> None:
    self.U = _choose_unroll(self.nodes, self.V * self.rows_in, self.R)
    if self.U is None:
      raise util.SemanticError(
          'march: a tensor needs a window of %d planes (> %d)' %
          (max(n.window for n in self.nodes), MAX_UNROLL))
    for n in self.nodes:
      n.slots = min(d for d in range(1, self.U + 1)
                    if self.U % d == 0 and d >= n.window)

  def _estimate_registers(self) -> None:
    """Rows (3-D) of every tensor that some output row of the tile depends on:
    the generator emits all rows a tensor can hold, the compiler drops the
    statements nobody reads -- the estimate must not count them (denoise3d:
    10 stages, most of them needed on the 2-4 output rows only)."""
    rows = (lambda lo, hi: (lo[1], hi[1])) if self.dim == 3 else \
        (lambda lo, hi: (0, 0))
    need = _walk_back(
        self.nodes,
        {id(n): (self.rhalo_lo, self.rows_in - self.rhalo_hi)
         for n in self.out_nodes},
        lambda v, tlo, thi: (v[0] + rows(tlo, thi)[0], v[1] + rows(tlo, thi)[1]),
        lambda old, new: (min(old[0], new[0]), max(old[1], new[1])))

    def rows_needed(n: _Node) -> int:
      if need[id(n)] is None:
        return 0
      lo = max(need[id(n)][0], n.rmargin[0])
      hi = min(need[id(n)][1], self.rows_in - n.rmargin[1])
      return max(0, hi - lo)

    self.est_regs = max(
        sum(n.slots * self.V * rows_needed(n)
            for n in self.nodes if n.owner == wv) for wv in range(self.W))
    if self.est_regs > 400:
      raise util.SemanticError(
          'march: the register windows need about %d VGPRs per lane' % self.est_regs)

  def _first_planes(self) -> None:
    """Lowest plane of every tensor (relative to the chunk's first output
    plane) that some output plane of the chunk depends on: before that,
    computing the tensor is wasted pipeline warm-up."""
    self.back_lo = _walk_back(
        self.nodes, {id(n): 0 for n in self.out_nodes},
        lambda v, tlo, thi: v + tlo[self.ax], min)

  def _warm_up(self) -> None:
    self.max_delay = max(n.delay for n in self.out_nodes)
    bounds = self.st.window_bounds(self.T)
    self.m_lo = min(0, min(bounds[o][0][self.ax] for o in self.st.output_names))
    self.m_hi = max(0, max(bounds[o][1][self.ax] for o in self.st.output_names))
    # load-only ticks at the head of a chunk (branch-free: buffer addressing).
    # A stage that lags the loads by d computes, in the first `lead` <= d ticks,
    # only planes below every plane the chunk needs; a stage without inputs
    # (a constant) has d = 0 and forbids the peeling.
    self.lead = min([self.PF] + [n.delay for n in self.nodes if n.stage is not None])
    # compute ticks before a chunk's first output
    self.warm = self.max_delay - self.m_lo - self.lead

    # peeled warm-up: row steps in front of the loop (a whole number of loop
    # trips, so the register slots line up) in which a stage is emitted only
    # from the step on at which its rows start to matter
    self.peeled = 0
    self.peel_trips_max = 0
    if self.W == 1:
      steps = -(-self.warm // self.U) * self.U
      stages = [n for n in self.nodes if n.stage is not None]
      skipped = sum(1 for i in range(steps) for n in stages
                    if not self.stage_needed(n, i))
      if skipped * 4 >= steps * len(stages):
        self.peel_trips_max = steps // self.U
        trips = self.peel_trips_max if self.cfg.peel < 0 else min(
            self.cfg.peel, self.peel_trips_max)
        self.peeled = trips * self.U

  def _name_and_block(self) -> None:
    cfg = self.cfg
    self.kind = 'march%dd' % self.dim
    self.name = '%s_%s_%s' % (self.st.app_name, self.kind, cfg.key())
    if cfg.residual:
      self.name += '_rs'
    self.waves = cfg.waves_x * cfg.waves_y if self.dim == 2 else 1
    self.wx = cfg.waves_x if self.dim == 2 else 1
    if self.W > 1:
      self.waves = self.W
    if self.xs:
      self.waves = self.xs
    self.block = 64 * self.waves

  def _tables(self) -> None:
    """What the text looks up per tensor: cell sizes, edge cells, the rows
    x-halo sharing hands over, the window reductions."""
    cfg = self.cfg
    table = self.st.symbol_table
    self.esz = {nme: table[nme].size_in_bytes
                for nme in list(self.inputs) + list(self.outputs)}
    self.n_edge = max(self.edge)
    self.xs_nodes = [n for n in self.nodes if n.xs]
    self.xs_rows = self.xs_stride = 0
    if self.xs_nodes:    # (none: no tap leaves its column, nothing to share)
      self.xs_rows = max(len(self.rows_of(n)) for n in self.xs_nodes)
      if self.xs_rows > 32:
        raise util.SemanticError('march: x-halo sharing holds a row per lane')
      self.xs_stride = self.xs * 2 * self.xs_rows
    # 'mixh': the two shift directions on two different pipes -- down through
    # DPP (vector ALU), up through ds_swizzle (the LDS crossbar, shared by the
    # four SIMDs of a CU) -- on 32-lane half strips
    self.use_mix = cfg.lane_shift == 'mixh'
    # Integer sums over a run of taps along the STREAMED dimension as a sliding
    # sum: an int32 accumulator per cell that lives across row steps,
    #     acc += newest row;  result = cast(acc);  acc -= oldest row
    # -- 2 operations per cell whatever the window (xcorr: 19 rows), no
    # auxiliary tensors.  State that survives row steps: the stage must run in
    # EVERY step from its first on (it does: a stage is never dropped again
    # once the peeled warm-up has started it) and the accumulator is set up
    # right before that first step from the rows the window holds then.
    # Exact: integers narrower than 32 bits (optimization/windows.py).
    # {id(node): (parent, offset of the first tap, taps)}
    self.slide: Dict[int, Tuple[str, Tuple[int, ...], int]] = {}
    # integer window reductions along dimension 0, all cells of a lane jointly:
    # {id(node): (op, parent, first offset relative to the cell, taps)} where
    # the stage is an association-free reduction over a contiguous run of
    # dimension-0 taps of one tensor (optimization/windows.py states when it
    # is)
    self.xwin: Dict[int, Tuple[str, str, Tuple[int, ...], int]] = {}
    if cfg.xwindow:
      from soda_amd.optimization import windows
      table = dict(self.st.symbol_table)
      for n in self.nodes:
        if n.stage is None or n.mirror_of is not None or n.keep is not None:
          continue
        m = windows._match(n.stage.stmt, table)
        if m is None:
          continue
        off = tuple(a - b for a, b in zip(m[5], n.stage.st_idx))
        if m[0] == '+' and m[2] == self.ax and cfg.slide and self.W == 1:
          self.slide[id(n)] = (m[1], off, m[4])
        elif m[2] == 0:
          self.xwin[id(n)] = (m[0], m[1], off, m[4])
    self.nt_l = 'true' if cfg.nt_load else 'false'
    self.nt_s = 'true' if cfg.nt_store else 'false'

  # -- what the steps and the text ask of it -----------------------------------
  def rows_of(self, n: _Node):
    return range(n.rmargin[0], self.rows_in - n.rmargin[1])

  def store_rows(self, n: _Node):
    return range(max(n.rmargin[0], self.rhalo_lo),
                 self.rows_in - max(n.rmargin[1], self.rhalo_hi))

  def stage_needed(self, n: _Node, step: int) -> bool:
    """Does the plane `n` computes `step` row steps into a chunk (counted from
    the first step of the loop) reach any output plane of the chunk?"""
    lo = self.back_lo[id(n)]
    if lo is None:
      return False
    return self.m_lo + self.lead + step >= lo + n.delay

  @staticmethod
  def slot_of(n: _Node, k: int, age: int) -> int:
    return (k - age) % n.slots
