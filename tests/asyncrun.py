"""The late-fill harness of tests/test_async.py: library calls enqueued on a
live stream AHEAD of their inputs.

Every other GPU test hands the library the idle default stream and
synchronises the host before it looks at a byte, so a launch that strays to
another stream, or a side stream that is never joined, cannot fail there.
Here a call runs on a fresh `torch.cuda.Stream()` S (non-blocking: nothing
orders it against the default stream) like this:

  1. inputs and param arrays lie on the device holding POISON -- NaN in float
     cells, 0x5A bytes in integer cells -- and so do the outputs;
  2. S: a delay (`torch.cuda._sleep`);
  3. S: copies of the real values into the inputs and params; event `filled`;
  4. the library call(s) under test, on S;
  5. the moment they return: `filled` has NOT fired -- the call was enqueued
     ahead of its inputs, or the run proves nothing (asserted, never skipped);
  6. S: copies of the outputs to side tensors, then poison over the inputs,
     the params and the outputs again;
  7. S.synchronize(); the side copies are what the caller compares.

A launch that is not ordered on S reads poison (it runs during the delay) or
leaves poison (S copies the outputs before it ran); work on another stream
that S does not wait for is copied out before it is done, or computes from
the poison of step 6.

The delay.  `torch.cuda._sleep` is calibrated once per session with events
(`cycles_per_ms`), the host time of every enqueue is taken with
time.perf_counter (`STATS`), and tests/test_async.py asserts at the end of its
run that DELAY_MS is at least ten times the slowest of them.  Measured on an
MI355X: 2.40e6 cycles per millisecond, 0.44 ms for the slowest enqueue (a
cold split pass with its side stream); see MEASURED below.  The assertion of
step 5 is what keeps the number honest."""
import time

import numpy as np

# Measured on an MI355X (tests/test_async.py, the whole module, 37 tests in
# 8 s, two runs): torch.cuda._sleep runs 2.40e6 and 2.38e6 cycles per
# millisecond; the slowest enqueue of the module (the split pass with its side
# stream, cold) took 0.44 and 0.43 ms of host time.  DELAY_MS is over 200
# times that, and at most 500.
MEASURED = {'cycles_per_ms': 2.40e6, 'slowest_enqueue_ms': 0.44}
DELAY_MS = 100.0

INT_POISON = 0x5A

# of this session: cycles of torch.cuda._sleep per millisecond; the slowest
# enqueue so far (milliseconds of host time) and which one it was
STATS = {'cycles_per_ms': None, 'enqueue_ms': 0.0, 'slowest': None}


def poison_like(arr):
  arr = np.asarray(arr)
  if arr.dtype.kind == 'f':
    return np.full(arr.shape, np.nan, arr.dtype)
  out = np.empty(arr.shape, arr.dtype)
  out.reshape(-1).view(np.uint8)[:] = INT_POISON
  return out


def cycles_per_ms():
  """Cycles of torch.cuda._sleep per millisecond of GPU time, measured once
  per session between two events."""
  import torch
  if STATS['cycles_per_ms'] is None:
    torch.cuda._sleep(1000000)         # the first launch loads the kernel
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    cycles = 10000000
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    STATS['cycles_per_ms'] = cycles / a.elapsed_time(b)
  return STATS['cycles_per_ms']


def _bytes(arr):
  import torch
  flat = np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()
  return torch.from_numpy(flat).cuda()


class LateFill:
  """One stream, its delay, its tensors.

  real      {name: array}: inputs and param arrays, in the order of the call
  out_like  {name: (shape, dtype)}: the outputs (of every call, where several
            calls run behind one delay: each has its own)
  late2     {name: (lo, hi)}: the first `lo` and the last `hi` rows (axis 0)
            of that input are filled on a SECOND stream behind a longer delay
            of its own, and `ghosts_ready` (a hipEvent_t) fires behind them
  delay     in units of DELAY_MS
  """

  def __init__(self, real, out_like, late2=None, stream=None, delay=1.0):
    import torch
    from soda_amd import runtime
    self.real = {n: np.ascontiguousarray(a) for n, a in real.items()}
    self.out_like = {n: (tuple(s), np.dtype(d)) for n, (s, d) in out_like.items()}
    self.late2 = dict(late2 or {})
    self.stream = stream if stream is not None else torch.cuda.Stream()
    self.delay = delay
    self._real = {n: _bytes(a) for n, a in self.real.items()}
    self._poison = {n: _bytes(poison_like(a)) for n, a in self.real.items()}
    self._ins = {n: t.clone() for n, t in self._poison.items()}
    self._out_poison = {n: _bytes(poison_like(np.empty(s, d)))
                        for n, (s, d) in self.out_like.items()}
    self._outs = {n: t.clone() for n, t in self._out_poison.items()}
    self._side = {n: torch.empty_like(t) for n, t in self._outs.items()}
    self.filled = torch.cuda.Event()
    self.second = torch.cuda.Stream() if self.late2 else None
    self._ready = runtime.Event() if self.late2 else None
    self.checked = False
    torch.cuda.synchronize()

  # -- what the call is handed ------------------------------------------------
  @property
  def ptr(self):
    return self.stream.cuda_stream

  def ins(self, names=None):
    return [self._ins[n].data_ptr() for n in (names or self.real)]

  def outs(self, names=None):
    return [self._outs[n].data_ptr() for n in (names or self.out_like)]

  @property
  def ghosts_ready(self):
    return self._ready.handle()

  def _row_bytes(self, name):
    a = self.real[name]
    return a.nbytes // a.shape[0]

  # -- steps 2 and 3 ------------------------------------------------------------
  def arm(self):
    import torch
    cycles = int(self.delay * DELAY_MS * cycles_per_ms())
    with torch.cuda.stream(self.stream):
      torch.cuda._sleep(cycles)
      for n, t in self._ins.items():
        lo, hi = self.late2.get(n, (0, 0))
        a, b = lo * self._row_bytes(n), t.numel() - hi * self._row_bytes(n)
        t[a:b].copy_(self._real[n][a:b])
      self.filled.record(self.stream)
    if self.late2:
      with torch.cuda.stream(self.second):
        torch.cuda._sleep(cycles + cycles // 2)
        for n, (lo, hi) in self.late2.items():
          t, a = self._ins[n], lo * self._row_bytes(n)
          b = t.numel() - hi * self._row_bytes(n)
          t[:a].copy_(self._real[n][:a])
          t[b:].copy_(self._real[n][b:])
      self._ready.record(self.second.cuda_stream)
    return self

  # -- step 5 -------------------------------------------------------------------
  def ahead(self):
    assert not self.filled.query(), \
        'the call returned after its inputs were filled: it was not enqueued ' \
        'ahead of them (it waited for the GPU, or the delay of %.0f ms is too ' \
        'short), so this run proves nothing' % (self.delay * DELAY_MS)
    self.checked = True

  # -- step 6 -------------------------------------------------------------------
  def collect(self, poison_outputs=True):
    import torch
    with torch.cuda.stream(self.stream):
      for n, t in self._outs.items():
        self._side[n].copy_(t)
      for n, t in self._ins.items():
        t.copy_(self._poison[n])
      if poison_outputs:
        for n, t in self._outs.items():
          t.copy_(self._out_poison[n])

  # -- step 7 -------------------------------------------------------------------
  def results(self):
    from soda_amd import runtime
    self.stream.synchronize()
    if self.second is not None:
      self.second.synchronize()
    # no error left behind by anything the library enqueued
    runtime.check(runtime.library().soda_hip_stream_synchronize(None),
                  'after a late-fill run')
    assert self.checked, 'step 5 was never asserted'
    return {n: self._side[n].cpu().numpy().view(d).reshape(s)
            for n, (s, d) in self.out_like.items()}


def timed(what, fn):
  """Runs fn(); its host time counts towards the slowest enqueue."""
  t0 = time.perf_counter()
  fn()
  ms = (time.perf_counter() - t0) * 1e3
  if ms > STATS['enqueue_ms']:
    STATS['enqueue_ms'], STATS['slowest'] = ms, what
  return ms


def late_fill(what, real, out_like, enqueue, late2=None, poison_outputs=True):
  """Steps 1 to 7 around `enqueue(run)` (run.ptr, run.ins(), run.outs(),
  run.ghosts_ready); returns {output name: array}."""
  run = LateFill(real, out_like, late2).arm()
  timed(what, lambda: enqueue(run))
  run.ahead()
  run.collect(poison_outputs)
  return run.results()
