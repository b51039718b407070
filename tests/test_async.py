"""The device entries on a live stream: ordering, scratch, graphs.

include/soda_hip.h promises that soda_hip_run_device* and
soda_hip_stream_run_device are asynchronous on `stream` ("Streams, scratch,
graphs").  Every other GPU test calls them on the idle default stream and
synchronises the host before it looks at a byte: that pins WHAT the kernels
compute, not WHEN AND WHERE the library enqueues them.  Here

  A/B  every kernel family runs through the late-fill harness
       (tests/asyncrun.py): enqueued on a side stream ahead of its inputs,
       its outputs copied out and poisoned again behind it on that stream;
  C    calls run back to back on one handle while its scratch regrows, two
       handles run on two streams, one handle moves between streams;
  D    runs are captured into a graph (torch.cuda.graph) and replayed; a call
       whose scratch would have to grow during capture is refused and leaves
       the capture valid.

Programs, grids and references are those of tests/test_device_entry.py (the
smallest with two strips, three chunks and a ragged tail; oracle finite on the
compared box), every comparison is bit for bit against the C oracle
(values.same_bits), programs are built with calibrate=False (an
auto-calibrating first run synchronises the stream by design).  A replay after
regrowth is NOT tested: the graph then holds freed addresses
(include/soda_hip.h)."""
import functools
import re

import numpy as np
import pytest

from conftest import soda_path
import asyncrun
import values
import test_device_entry as de
import test_values as tv

pytestmark = pytest.mark.gpu

SEED = de.SEED


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------

def _order(stencil):
  """Names in the order of a call's `inputs`: input tensors, param arrays."""
  return list(stencil.input_names) + [p.name for p in stencil.param_stmts]


def _out_like(stencil, extent, batch=None, tag=''):
  shape = tuple(extent[::-1])
  if batch:
    shape = (batch,) + shape
  return {tag + o: (shape, np.dtype(t.np_name))
          for o, t in zip(stencil.output_names, stencil.output_types)}


@functools.lru_cache(maxsize=None)
def _poison_oracle(stencil, extent, iterate=None):
  like = values.edge_inputs(stencil, extent, 0, de._kind(stencil))
  ins = {n: asyncrun.poison_like(a) for n, a in like.items()}
  return tv._readonly(tv._oracle(stencil).run(ins, iterate=iterate))


def _poison_differs(stencil, extent, want, iterate=None, whole=False):
  """The oracle of the poison is not the oracle of the inputs, on every
  output: a run that read poison cannot pass."""
  bad = _poison_oracle(stencil, extent, iterate)
  for o, idx in tv._boxes(stencil, extent, iterate, whole):
    assert not values.same_bits(bad[o][idx], want[o][idx]).all(), o


def _late(prog, stencil, extent, ins, what, iterate=None, batch=None,
          late2=None, **run_kw):
  """One run_device call through the harness; {output: array}."""
  real = {n: ins[n] for n in _order(stencil)}
  if batch:
    run_kw['batch'] = batch

  def enqueue(run):
    prog.run_device(run.outs(), run.ins(), extent, iterate, stream=run.ptr,
                    **{k: (v(run) if callable(v) else v)
                       for k, v in run_kw.items()})
  return asyncrun.late_fill(what, real, _out_like(stencil, extent, batch),
                            enqueue, late2=late2)


def _kept_rows_same(stencil, extent, got, want, keep, iterate=None):
  for o in stencil.output_names:
    lo, hi = stencil.valid_box(extent, o, iterate)
    box = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
    k0, k1 = max(keep[0], lo[-1]) - lo[-1], min(keep[1], hi[-1]) - lo[-1]
    assert k1 > k0
    same = values.same_bits(got[o][box][k0:k1], want[o][box][k0:k1])
    assert same.all(), '%s: %d kept cells differ' % (o, int((~same).sum()))


# ---------------------------------------------------------------------------
# B. every family ahead of its inputs
# ---------------------------------------------------------------------------

NAMED = ['jacobi2d_T13', 'jacobi2d_pipe4', 'coupled2d', 'direct_blur_vfull',
         'conv2d', 'heat3d', 'heat3d_xshare', 'heat3d_xb2', 'heat3d_tile3d',
         'jacobi2d_preserve_auto', 'heat3d_preserve_direct']


@pytest.mark.parametrize('name', NAMED)
def test_named_cases_ahead_of_their_inputs(built, name):
  """Marching 2-D with multi-pass ping-pong (T13 + remainder passes, pipe4,
  two outputs), a two-kernel pass with its local in scratch, late param
  arrays, marching 3-D in its three forms, tile3d, `border: preserve` through
  `auto` and `direct`."""
  stencil, kw, extent, build_for = de._setup(name, probe=True)
  whole = bool(stencil.preserve_border)
  ins, want = de._reference(stencil, extent, SEED)
  assert de._finite(stencil, extent, want, whole=whole)
  _poison_differs(stencil, extent, want, whole=whole)
  with de._program(stencil, build_for, **kw) as prog:
    assert de.CASES[name][4] in tv._deepest(prog.module).name
    de._deepest_is_scheduled(prog, extent, stencil.iterate)
    got = _late(prog, stencil, extent, ins, name)
    launches = prog.last_launches()[0]
    if name == 'jacobi2d_T13':
      sched = prog.schedule(extent, stencil.iterate)
      assert sched.get(13) == 1 and len(sched) >= 2, sched
    if name == 'direct_blur_vfull':
      # two kernels, the local between them in the program's scratch
      assert launches >= 2 and prog.scratch()[0] > 0
    if name == 'conv2d':
      assert stencil.param_stmts
  tv._assert_same(stencil, extent, got, want, name, whole=whole)


@pytest.mark.parametrize('name,kind', [('wideint', 'full'),
                                       ('widefloat', 'positive')])
def test_ldswin_ahead_of_its_inputs(built, name, kind):
  stencil, extent, ins, want = de._ldswin_setup(name, kind)
  assert de._finite(stencil, extent, want)
  _poison_differs(stencil, extent, want)
  with de._program(stencil, extent, strategy='ldswin') as prog:
    k, = prog.module.kernels
    assert 'ldswin' in k.name
    got = _late(prog, stencil, extent, ins, 'ldswin %s' % name)
  tv._assert_same(stencil, extent, got, want, name)


@pytest.mark.parametrize('name', sorted(de.KEEP))
def test_keep_runs_ahead_of_their_inputs(built, name):
  """Three passes or more, trimmed to a cone: the passes before the last
  alternate between the program's two sets of temporaries."""
  soda, extent, iterate, fuse, keep = de.KEEP[name]
  stencil = de._keep_stencil(name)
  ins, want = de._reference(stencil, extent, SEED)
  assert de._finite(stencil, extent, want)
  _poison_differs(stencil, extent, want)
  with de._program(stencil, extent, fuse=fuse) as prog:
    de._deepest_is_scheduled(prog, extent, iterate)
    assert sum(prog.schedule(extent, iterate).values()) >= 3
    got = _late(prog, stencil, extent, ins, 'keep %s' % name, iterate,
                keep=keep)
    assert prog.last_rows() < prog.last_launches()[0] * extent[-1]
    cells = int(np.prod(extent)) * 4
    # temps and temps2 of the one output
    assert prog.scratch()[0] >= 2 * cells
  _kept_rows_same(stencil, extent, got, want, keep)


BATCHED = ['jacobi2d_T13', 'heat3d']


@functools.lru_cache(maxsize=None)
def _batch_reference(name, batch):
  """({input: [batch, ...]}, [oracle outputs per item])."""
  stencil, kw, extent, _ = de._setup(name, probe=True)
  items = [de._reference(stencil, extent, SEED + i) for i in range(batch)]
  ins = {n: np.stack([item[0][n] for item in items])
         for n in stencil.input_names}
  return tv._readonly(ins), [item[1] for item in items]


def _assert_items(stencil, extent, got, wants, what):
  for i, want in enumerate(wants):
    tv._assert_same(stencil, extent, {o: got[o][i] for o in got}, want,
                    '%s, item %d' % (what, i))


@pytest.mark.parametrize('name', BATCHED)
def test_batched_runs_ahead_of_their_inputs(built, name):
  stencil, kw, extent, build_for = de._setup(name, probe=True)
  ins, wants = _batch_reference(name, 3)
  for want in wants:
    assert de._finite(stencil, extent, want)
    _poison_differs(stencil, extent, want)
  with de._program(stencil, build_for, batch=True, **kw) as prog:
    got = _late(prog, stencil, extent, ins, 'batch of %s' % name, batch=3)
    assert prog.last_launches()[0] == \
        sum(prog.schedule(extent, stencil.iterate, 3).values())
  _assert_items(stencil, extent, got, wants, name)


SPLIT = dict(extent=(512, 300), iterate=9, fuse=(4,), ghost=12)


@pytest.mark.parametrize('order', ['inorder', 'side'])
def test_a_split_pass_ahead_of_its_inputs_and_its_ghosts(built, monkeypatch,
                                                         order):
  """One slab run with both events: the ghost rows are filled on a second
  stream behind a longer delay, `ghosts_ready` fires behind them.  In both
  launch orders of a split pass; with SODA_HIP_SPLIT=side the boundary chunks
  run on the program's own stream, which the call joins to the caller's."""
  from soda_amd import core, runtime
  monkeypatch.setenv('SODA_HIP_SPLIT', order)
  extent, iterate, ghost = SPLIT['extent'], SPLIT['iterate'], SPLIT['ghost']
  stencil = core.from_file(soda_path('jacobi2d.soda'), iterate=iterate)
  keep = (ghost, extent[1] - ghost)
  ins, want = de._reference(stencil, extent, SEED)
  assert de._finite(stencil, extent, want)
  _poison_differs(stencil, extent, want)
  sendable = runtime.Event()
  with de._program(stencil, extent, fuse=SPLIT['fuse']) as prog:
    got = _late(prog, stencil, extent, ins, 'split pass, %s' % order, iterate,
                late2={'t1': (ghost, ghost)}, keep=keep,
                ghosts=(ghost, ghost), sends=(ghost, ghost),
                ghosts_ready=lambda run: run.ghosts_ready,
                sendable=sendable.handle())
    assert prog.last_split() > 0
  _kept_rows_same(stencil, extent, got, want, keep)


# ---- the wire stream object -----------------------------------------------------

def _wire_stencil(name, in_decl=None, out_decl=None):
  from soda_amd import core
  text = open(soda_path(name)).read()
  if in_decl:
    text = re.sub(r'input dram [^\n]*', in_decl, text)
  if out_decl:
    text = re.sub(r'output dram [\d.]+ \w+:', out_decl, text)
  return core.from_text(text)


def _two_banks():
  import test_wire_banked as twb
  return twb._program('jacobi2d.soda', 2, 2, None)


# name -> (stencil, extent, StreamProgram keywords, last_mode): the dense, the
# linear and the two-bank case of tests/test_hip_parity.py STREAM_CASES (the
# last runs the unwire_ / wire_ copy passes and fills its staging array), the
# first banked case of tests/test_wire_banked.py GPU_CASES
WIRE = {
    'dense': (lambda: _wire_stencil('blur.soda',
                                    'input dram 0 uint16: input(2048, *)'),
              (2048, 20), dict(dense=True), 'dense'),
    'linear': (lambda: _wire_stencil('jacobi2d.soda'), (32, 12),
               dict(dense=False), 'linear'),
    'two_banks': (lambda: _wire_stencil('jacobi2d.soda',
                                        'input dram 0.1 float: t1(32, *)',
                                        'output dram 2.3 float:'),
                  (32, 12), dict(dense=True), 'dense'),
    'banked': (_two_banks, (32, 45), dict(dense=True, banked=True), 'banked'),
}


class _Wire:
  """A WIRE case: its banks, the reference kernel's banks, a stream object
  that never calibrates."""

  def __init__(self, name):
    from oracle import frt_layout
    from soda_amd import stream
    make, self.extent, self.kw, self.mode = WIRE[name]
    self.stencil = st = make()
    self.layout = stream.WireLayout(st, self.extent)
    self.shapes = frt_layout.alloc(self.layout, st.output_names)
    self.prog = None

  def banks(self, seed):
    """({'name/bank': array} of the inputs, {output: gathered reference})."""
    import test_wire_banked as twb
    from oracle import frt_layout
    st = self.stencil
    in_banks = frt_layout.scatter(self.layout,
                                  twb._inputs(st, self.extent, seed))
    real = {'%s/%d' % (n, b): bank for n in st.input_names
            for b, bank in enumerate(in_banks[n])}
    return real, self.gathered(
        frt_layout.kernel_on_streams(self.layout, in_banks))

  def gathered(self, out_banks):
    from oracle import frt_layout
    st = self.stencil
    got = {o: np.zeros(tuple(self.extent[::-1]), np.dtype(t.np_name))
           for o, t in zip(st.output_names, st.output_types)}
    frt_layout.gather(self.layout, out_banks, got)
    return got

  def out_like(self):
    return {'%s/%d' % (o, b): (bank.shape, bank.dtype)
            for o in self.stencil.output_names
            for b, bank in enumerate(self.shapes[o])}

  def open(self):
    from soda_amd import runtime, stream
    self.prog = stream.StreamProgram(self.stencil, **self.kw)
    for h in self.prog._programs.values():
      runtime.check(runtime.library().soda_hip_program_set_auto_calibrate(h, 0),
                    'set_auto_calibrate')
    return self.prog

  def close(self):
    if self.prog is not None:
      self.prog.close()

  def call(self, out_ptrs, in_ptrs, stream):
    """out_ptrs / in_ptrs: addresses in the order of out_like() / banks()."""
    st, outs, ins = self.stencil, iter(out_ptrs), iter(in_ptrs)
    nb = self.layout.bank_count
    self.prog.run_banked_device(
        {o: [next(outs) for _ in range(nb[o])] for o in st.output_names},
        {n: [next(ins) for _ in range(nb[n])] for n in st.input_names},
        self.layout.cycle_count, stream=stream)

  def split(self, flat):
    """{'name/bank': array} -> {output: [banks]}."""
    return {o: [flat['%s/%d' % (o, b)] for b in range(len(self.shapes[o]))]
            for o in self.stencil.output_names}

  def poison_differs(self, ref):
    from oracle import frt_layout
    st = self.stencil
    like = frt_layout.scatter(self.layout, {
        n: np.zeros(tuple(self.extent[::-1]), np.dtype(t.np_name))
        for n, t in zip(st.input_names, st.input_types)})
    bad = self.gathered(frt_layout.kernel_on_streams(self.layout, {
        n: [asyncrun.poison_like(b) for b in like[n]] for n in like}))
    for o in ref:
      assert not values.same_bits(bad[o], ref[o]).all(), o

  def assert_same(self, flat, ref, what):
    got = self.gathered(self.split(flat))
    for o in ref:
      same = values.same_bits(got[o], ref[o])
      assert ref[o].any() and same.all(), \
          '%s, output %s: %d cells differ' % (what, o, int((~same).sum()))


@pytest.mark.parametrize('name', sorted(WIRE))
def test_the_wire_stream_object_ahead_of_its_banks(built, name):
  """soda_hip_stream_run_device: un-interleave, program, re-interleave, all on
  the caller's stream.  What the host gathers is the reference kernel's, and
  every byte of the output banks -- beyond what the host gathers too -- is what
  a plain run on an idle GPU leaves.  The default stream is kept busy
  meanwhile: work that strayed there would come late.

  (What this does NOT catch: the fill of a new staging array sent to the
  default stream.  The array is 4 elements longer than the dense view of
  `two_banks`, and only those reach the caller's banks unwritten by the
  program; on new device memory they read as zeros with or without the fill.
  Tried once, see the commit message.)"""
  import torch
  case = _Wire(name)
  real, ref = case.banks(5)
  case.poison_differs(ref)
  try:
    # a plain run first, on a stream object of its own: the banks byte by byte
    case.open()
    plain = asyncrun.LateFill(real, case.out_like())
    for n, t in plain._ins.items():
      t.copy_(plain._real[n])
    torch.cuda.synchronize()
    case.call(plain.outs(), plain.ins(), 0)
    torch.cuda.synchronize()
    assert case.prog.last_mode == case.mode
    plain_banks = {n: t.cpu().numpy() for n, t in plain._outs.items()}
    case.close()
    # ... then ahead of its banks, on a fresh one
    case.open()
    run = asyncrun.LateFill(real, case.out_like())
    torch.cuda._sleep(int(3 * asyncrun.DELAY_MS * asyncrun.cycles_per_ms()))
    run.arm()
    asyncrun.timed('wire %s' % name,
                   lambda: case.call(run.outs(), run.ins(), run.ptr))
    run.ahead()
    run.collect()
    got = run.results()
    assert case.prog.last_mode == case.mode
  finally:
    case.close()
  case.assert_same(got, ref, name)
  for n in got:
    assert (got[n].view(np.uint8).reshape(-1) == plain_banks[n]).all(), \
        'bank %s differs from a plain run beyond what the host gathers' % n


# ---------------------------------------------------------------------------
# C. back-to-back calls, regrowth, two handles, two streams
# ---------------------------------------------------------------------------

def _several(name):
  """(stencil, LowerOptions keywords, (A, B < A, C > A)) of
  test_device_entry.SEVERAL."""
  return de._several_stencil(name), de.SEVERAL[name][2], de.SEVERAL[name][3]


def test_scratch_regrows_under_queued_calls(built):
  """One handle, one stream, no host synchronisation in between: the small
  extent with one iteration (no scratch) and with three passes (temporaries),
  a larger one (they regrow), the largest with a `keep=` run of three passes
  (they regrow again, their partners appear), the small one again.  The first call is enqueued ahead
  of its inputs; a call that regrows scratch waits for the device by contract
  (include/soda_hip.h), so from the second call on the delay has passed -- but
  nothing orders the host against the stream except that wait, and every call
  has its own outputs, compared at the end."""
  stencil, kw, (a, b, c) = _several('jacobi2d')
  keep = (10, c[1] - 10)
  calls = [(b, 1, None), (b, 9, None), (a, 9, None), (c, 9, keep),
           (b, 6, None)]
  real, out_like, wants = {}, {}, []
  for i, (extent, iterate, _) in enumerate(calls):
    ins, want = de._reference(stencil, extent, SEED, iterate)
    assert de._finite(stencil, extent, want, iterate)
    _poison_differs(stencil, extent, want, iterate)
    real['%d/t1' % i] = ins['t1']
    out_like.update(_out_like(stencil, extent, tag='%d/' % i))
    wants.append(want)
  with de._program(stencil, None, **kw) as prog:
    for extent, iterate, _ in calls[1:]:
      assert sum(prog.schedule(extent, iterate).values()) >= 3
    run = asyncrun.LateFill(real, out_like).arm()
    seen = []
    for i, (extent, iterate, kp) in enumerate(calls):
      prog.run_device(run.outs(['%d/t0' % i]), run.ins(['%d/t1' % i]), extent,
                      iterate, stream=run.ptr,
                      **({'keep': kp} if kp else {}))
      if i == 0:
        run.ahead()
      seen.append(prog.scratch())
    run.collect()
    got = run.results()
  # (bytes, buffers replaced so far): none; the temporary of B; of A, which
  # replaces it; of C, which replaces that, and its partner; the same
  cells = {e: int(np.prod(e)) * 4 for e in (a, b, c)}
  assert seen == [(0, 0), (cells[b], 0), (cells[a], 1), (2 * cells[c], 2),
                  (2 * cells[c], 2)], seen
  for i, (extent, iterate, kp) in enumerate(calls):
    one = {'t0': got['%d/t0' % i]}
    if kp:
      _kept_rows_same(stencil, extent, one, wants[i], kp, iterate)
    else:
      tv._assert_same(stencil, extent, one, wants[i], 'call %d' % i, iterate)


def test_scratch_regrows_twice_under_queued_batches(built):
  """A batched handle: batch 1, then 4, then 2, extents small, larger, small.
  Its temporaries are allocated by the first call and replaced by the second
  and by the third while the earlier ones are still queued."""
  stencil, kw, _ = _several('heat3d')
  a, b = (264, 11, 14), (132, 9, 14)
  calls = [(b, 3, 1), (b, 3, 4), (a, 3, 2), (b, 3, 2)]
  real, out_like, wants = {}, {}, []
  for i, (extent, iterate, batch) in enumerate(calls):
    items = [de._reference(stencil, extent, SEED + j, iterate)
             for j in range(batch)]
    for _, want in items:
      assert de._finite(stencil, extent, want, iterate)
      _poison_differs(stencil, extent, want, iterate)
    real['%d/in' % i] = np.stack([item[0]['in'] for item in items])
    out_like.update(_out_like(stencil, extent, batch, tag='%d/' % i))
    wants.append([item[1] for item in items])
  with de._program(stencil, None, batch=True, **kw) as prog:
    for extent, iterate, batch in calls:
      assert sum(prog.schedule(extent, iterate, batch).values()) >= 2
    run = asyncrun.LateFill(real, out_like).arm()
    seen = []
    for i, (extent, iterate, batch) in enumerate(calls):
      prog.run_device(run.outs(['%d/out' % i]), run.ins(['%d/in' % i]), extent,
                      iterate, stream=run.ptr, batch=batch)
      if i == 0:
        run.ahead()
      seen.append(prog.scratch())
    run.collect()
    got = run.results()
  cells = {e: int(np.prod(e)) * 4 for e in (a, b)}
  assert cells[a] * 2 > cells[b] * 4
  assert seen == [(cells[b], 0), (4 * cells[b], 1), (2 * cells[a], 2),
                  (2 * cells[a], 2)], seen
  for i, (extent, iterate, batch) in enumerate(calls):
    for j in range(batch):
      tv._assert_same(stencil, extent, {'out': got['%d/out' % i][j]},
                      wants[i][j], 'call %d, item %d' % (i, j), iterate)


def test_two_handles_on_two_streams(built):
  """Their enqueues interleaved, each behind its own delay: independent, and
  both right."""
  cases = []
  for name in ('jacobi2d_T13', 'heat3d'):
    stencil, kw, extent, build_for = de._setup(name, probe=True)
    ins, want = de._reference(stencil, extent, SEED)
    cases.append((name, stencil, kw, extent, build_for, ins, want))
  progs = [de._program(c[1], c[4], **c[2]) for c in cases]
  try:
    runs = [asyncrun.LateFill({n: c[5][n] for n in _order(c[1])},
                              _out_like(c[1], c[3]), delay=d)
            for c, d in zip(cases, (1.0, 1.5))]
    # twice each, alternating: the second run of a handle goes through the
    # same temporaries behind the first, into outputs of its own
    outs2 = [asyncrun.LateFill({}, _out_like(c[1], c[3]), stream=r.stream)
             for c, r in zip(cases, runs)]
    for run in runs:
      run.arm()
    for rnd in range(2):
      for c, prog, run, second in zip(cases, progs, runs, outs2):
        prog.run_device((run if rnd == 0 else second).outs(), run.ins(), c[3],
                        stream=run.ptr)
    for run in runs:
      run.ahead()
    for run, second in zip(runs, outs2):
      second.checked = True
      second.collect()
      run.collect()
    got = [(run.results(), second.results())
           for run, second in zip(runs, outs2)]
  finally:
    for prog in progs:
      prog.close()
  for c, (first, second) in zip(cases, got):
    tv._assert_same(c[1], c[3], first, c[6], c[0])
    tv._assert_same(c[1], c[3], second, c[6], c[0] + ', again')


def test_one_handle_on_one_stream_then_another(built):
  """The header: one handle is one queue of work, the caller orders calls on
  different streams.  The call on S2 is ordered behind the call on S1 by an
  event; both share the handle's temporaries; both are right."""
  import torch
  stencil, kw, extent, build_for = de._setup('jacobi2d_T13', probe=True)
  ins, want = de._reference(stencil, extent, SEED)
  ins2, want2 = de._reference(stencil, extent, SEED + 1)
  with de._program(stencil, build_for, **kw) as prog:
    first = asyncrun.LateFill({'t1': ins['t1']}, _out_like(stencil, extent))
    second = asyncrun.LateFill({'t1': ins2['t1']}, _out_like(stencil, extent),
                               delay=0.5)
    first.arm()
    second.arm()
    prog.run_device(first.outs(), first.ins(), extent, stream=first.ptr)
    done = torch.cuda.Event()
    done.record(first.stream)
    second.stream.wait_event(done)
    prog.run_device(second.outs(), second.ins(), extent, stream=second.ptr)
    first.ahead()
    second.checked = True        # (its own fill is the shorter one)
    first.collect()
    second.collect()
    got, got2 = first.results(), second.results()
  tv._assert_same(stencil, extent, got, want, 'on S1')
  tv._assert_same(stencil, extent, got2, want2, 'on S2')


# ---------------------------------------------------------------------------
# D. graph capture
# ---------------------------------------------------------------------------

class _Tensors:
  """Device tensors of one run_device call, refilled per seed."""

  def __init__(self, names, out_like):
    self.names, self.out_like = list(names), out_like
    self.ins, self.outs = {}, {}

  def fill(self, ins):
    import torch
    for n in self.names:
      src = asyncrun._bytes(ins[n])
      if n not in self.ins:
        self.ins[n] = src
      else:
        self.ins[n].copy_(src)
    for n, (s, d) in self.out_like.items():
      src = asyncrun._bytes(asyncrun.poison_like(np.empty(s, d)))
      if n not in self.outs:
        self.outs[n] = src
      else:
        self.outs[n].copy_(src)
    torch.cuda.synchronize()

  def in_ptrs(self):
    return [self.ins[n].data_ptr() for n in self.names]

  def out_ptrs(self):
    return [t.data_ptr() for t in self.outs.values()]

  def read(self):
    import torch
    torch.cuda.synchronize()
    return {n: self.outs[n].cpu().numpy().view(d).reshape(s)
            for n, (s, d) in self.out_like.items()}


GRAPH = ['jacobi2d_T13', 'heat3d', 'heat3d_tile3d', 'ldswin',
         'batch of jacobi2d_T13']


def _graph_case(name):
  """(stencil, program keywords, extent, extent built for, batch,
  seed -> (inputs, [oracle per item]))."""
  if name == 'ldswin':
    stencil, extent, _, _ = de._ldswin_setup('widefloat', 'positive')

    def reference(seed):
      ins = {n: np.abs(a) for n, a in
             de._reference(stencil, extent, seed)[0].items()}
      return ins, [tv._oracle(stencil).run(ins)]
    return stencil, dict(strategy='ldswin'), extent, extent, None, reference
  batch = 3 if name.startswith('batch of ') else None
  base = name.replace('batch of ', '')
  stencil, kw, extent, build_for = de._setup(base, probe=True)

  def reference(seed):
    if not batch:
      ins, want = de._reference(stencil, extent, seed)
      return ins, [want]
    items = [de._reference(stencil, extent, seed + 100 * j)
             for j in range(batch)]
    ins = {n: np.stack([item[0][n] for item in items])
           for n in stencil.input_names}
    return ins, [item[1] for item in items]
  if batch:
    kw = dict(kw, batch=True)
  return stencil, kw, extent, build_for, batch, reference


def _assert_seed(stencil, extent, batch, got, wants, what):
  if batch:
    _assert_items(stencil, extent, got, wants, what)
  else:
    tv._assert_same(stencil, extent, got, wants[0], what)


@pytest.mark.parametrize('name', GRAPH)
def test_warm_capture_replay(built, name):
  """The recipe of the header: one eager run (scratch exists), capture one
  run_device call, replay it three times on new inputs; an eager call that
  fits the scratch between two replays leaves the graph working."""
  import torch
  stencil, kw, extent, build_for, batch, reference = _graph_case(name)
  run_kw = dict(batch=batch) if batch else {}
  S = torch.cuda.Stream()
  t = _Tensors(_order(stencil), _out_like(stencil, extent, batch))
  with de._program(stencil, build_for, **kw) as prog:
    ins, wants = reference(SEED)
    t.fill(ins)
    prog.run_device(t.out_ptrs(), t.in_ptrs(), extent, stream=S.cuda_stream,
                    **run_kw)
    S.synchronize()
    _assert_seed(stencil, extent, batch, t.read(), wants, name + ', eager')
    warm = prog.scratch()
    g = torch.cuda.CUDAGraph()
    t.fill(ins)
    with torch.cuda.graph(g, stream=S):
      prog.run_device(t.out_ptrs(), t.in_ptrs(), extent, stream=S.cuda_stream,
                      **run_kw)
    # capture records, it does not run
    assert all((a.view(np.uint8) == asyncrun.poison_like(a).view(np.uint8)).all()
               for a in t.read().values())
    for k, seed in enumerate((SEED + 1, SEED + 2, SEED + 3)):
      ins, wants = reference(seed)
      for want in wants:
        assert de._finite(stencil, extent, want,
                          whole=bool(stencil.preserve_border))
      t.fill(ins)
      g.replay()
      _assert_seed(stencil, extent, batch, t.read(), wants,
                   '%s, replay %d' % (name, k))
      if k == 0:
        # an eager call between two replays
        ins, wants = reference(SEED + 7)
        t.fill(ins)
        prog.run_device(t.out_ptrs(), t.in_ptrs(), extent,
                        stream=torch.cuda.current_stream().cuda_stream,
                        **run_kw)
        _assert_seed(stencil, extent, batch, t.read(), wants,
                     name + ', eager between replays')
    assert prog.scratch() == warm
    torch.cuda.synchronize()
    del g


def _wire_tensors(case, real):
  t = _Tensors(list(real), case.out_like())
  t.fill(real)
  return t


@pytest.mark.parametrize('name', sorted(WIRE))
def test_warm_capture_replay_of_a_dense_wire_stream(built, name):
  """Every form a call's route takes -- dense view, linear, copy kernels
  around the dense view, banked -- captured warm and replayed."""
  import torch
  case = _Wire(name)
  S = torch.cuda.Stream()
  try:
    case.open()
    real, ref = case.banks(5)
    t = _wire_tensors(case, real)
    case.call(t.out_ptrs(), t.in_ptrs(), S.cuda_stream)
    S.synchronize()
    case.assert_same(t.read(), ref, 'eager')
    g = torch.cuda.CUDAGraph()
    t.fill(real)
    with torch.cuda.graph(g, stream=S):
      case.call(t.out_ptrs(), t.in_ptrs(), S.cuda_stream)
    for seed in (6, 7, 8):
      real, ref = case.banks(seed)
      t.fill(real)
      g.replay()
      case.assert_same(t.read(), ref, 'replay, seed %d' % seed)
    assert case.prog.last_mode == case.mode
    torch.cuda.synchronize()
    del g
  finally:
    case.close()


def test_capture_never_calibrates(built):
  """A handle that calibrates by itself: an eager run on the larger extent
  times that extent (and leaves scratch large enough for the smaller one); the
  FIRST run on the smaller extent, captured, is scheduled by the model and
  replays right."""
  import torch
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  stencil, kw, (a, b, c) = _several('jacobi2d')
  S = torch.cuda.Stream()
  with runtime.Program(stencil, lower.LowerOptions(**kw)) as prog:
    ins, want = de._reference(stencil, a, SEED, 9)
    big = _Tensors(['t1'], _out_like(stencil, a))
    big.fill(ins)
    prog.run_device(big.out_ptrs(), big.in_ptrs(), a, 9, stream=S.cuda_stream)
    tv._assert_same(stencil, a, big.read(), want, 'eager', 9)
    assert prog.pass_times(a)[1] is True
    assert prog.pass_times(b)[1] is False
    modelled = prog.schedule(b, 6)
    ins, want = de._reference(stencil, b, SEED, 6)
    small = _Tensors(['t1'], _out_like(stencil, b))
    small.fill(ins)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
      prog.run_device(small.out_ptrs(), small.in_ptrs(), b, 6,
                      stream=S.cuda_stream)
    assert prog.pass_times(b)[1] is False
    assert prog.schedule(b, 6) == modelled
    g.replay()
    tv._assert_same(stencil, b, small.read(), want, 'replay', 6)
    del g


def _assert_refused(err):
  text = str(err.value)
  assert 'captured into a graph' in text and 'once eagerly' in text, text
  assert text.endswith('nothing was launched'), text


def test_growth_is_refused_under_capture(built):
  """A cold handle that needs temporaries, on a capturing stream: refused
  before anything is allocated or launched, and the capture stays valid -- the
  call of a warm handle that follows in the same capture is recorded and
  replays right."""
  import torch
  from soda_amd import util
  stencil, kw, extent, build_for = de._setup('jacobi2d_T13', probe=True)
  ins, want = de._reference(stencil, extent, SEED)
  ins2, want2 = de._reference(stencil, extent, SEED + 1)
  S = torch.cuda.Stream()
  t = _Tensors(['t1'], _out_like(stencil, extent))
  cold_t = _Tensors(['t1'], _out_like(stencil, extent))
  with de._program(stencil, build_for, **kw) as warm, \
      de._program(stencil, build_for, **kw) as cold:
    t.fill(ins)
    cold_t.fill(ins)
    warm.run_device(t.out_ptrs(), t.in_ptrs(), extent, stream=S.cuda_stream)
    S.synchronize()
    assert warm.scratch()[0] > 0 and cold.scratch() == (0, 0)
    g = torch.cuda.CUDAGraph()
    t.fill(ins2)
    with torch.cuda.graph(g, stream=S):
      with pytest.raises(util.BackendError) as err:
        cold.run_device(cold_t.out_ptrs(), cold_t.in_ptrs(), extent,
                        stream=S.cuda_stream)
      warm.run_device(t.out_ptrs(), t.in_ptrs(), extent, stream=S.cuda_stream)
    _assert_refused(err)
    assert cold.scratch() == (0, 0)
    g.replay()
    tv._assert_same(stencil, extent, t.read(), want2, 'replay')
    # the refused call left its outputs alone
    assert all((a.view(np.uint8) == asyncrun.poison_like(a).view(np.uint8)).all()
               for a in cold_t.read().values())
    # ... and the handle works: eagerly it allocates and runs
    cold.run_device(cold_t.out_ptrs(), cold_t.in_ptrs(), extent,
                    stream=S.cuda_stream)
    S.synchronize()
    tv._assert_same(stencil, extent, cold_t.read(), want, 'cold, eager')
    del g


def test_growth_of_a_wire_stream_is_refused_under_capture(built):
  """soda_hip_stream_run_device allocates its staging arrays between its
  launches; whether it has to is found out before the first of them."""
  import torch
  from soda_amd import util
  warm, cold = _Wire('two_banks'), _Wire('two_banks')
  S = torch.cuda.Stream()
  try:
    warm.open()
    cold.open()
    real, ref = warm.banks(5)
    real2, ref2 = warm.banks(6)
    t, cold_t = _wire_tensors(warm, real), _wire_tensors(cold, real)
    warm.call(t.out_ptrs(), t.in_ptrs(), S.cuda_stream)
    S.synchronize()
    g = torch.cuda.CUDAGraph()
    t.fill(real2)
    with torch.cuda.graph(g, stream=S):
      with pytest.raises(util.BackendError) as err:
        cold.call(cold_t.out_ptrs(), cold_t.in_ptrs(), S.cuda_stream)
      warm.call(t.out_ptrs(), t.in_ptrs(), S.cuda_stream)
    _assert_refused(err)
    g.replay()
    warm.assert_same(t.read(), ref2, 'replay')
    assert all((a.view(np.uint8) == asyncrun.poison_like(a).view(np.uint8)).all()
               for a in cold_t.read().values())
    cold.call(cold_t.out_ptrs(), cold_t.in_ptrs(), S.cuda_stream)
    S.synchronize()
    cold.assert_same(cold_t.read(), ref, 'cold, eager')
    del g
  finally:
    warm.close()
    cold.close()


# ---------------------------------------------------------------------------
# the delay (last: it looks at every enqueue above)
# ---------------------------------------------------------------------------

def test_the_delay_covers_ten_enqueues(built):
  """DELAY_MS against the slowest enqueue of this session (of the whole module
  where the whole module ran, which is how the number was chosen)."""
  stencil, kw, extent, build_for = de._setup('jacobi2d_T13', probe=True)
  ins, want = de._reference(stencil, extent, SEED)
  with de._program(stencil, build_for, **kw) as prog:     # cold: it allocates
    got = _late(prog, stencil, extent, ins, 'a cold handle')
  tv._assert_same(stencil, extent, got, want, 'a cold handle')
  stats = asyncrun.STATS
  print('torch.cuda._sleep: %.0f cycles per ms; slowest enqueue: %.3f ms (%s); '
        'delay: %.0f ms' % (asyncrun.cycles_per_ms(), stats['enqueue_ms'],
                            stats['slowest'], asyncrun.DELAY_MS))
  assert 10 * stats['enqueue_ms'] <= asyncrun.DELAY_MS <= 500
