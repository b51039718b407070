"""Residual of the last iteration with one rank per GPU (soda_amd/dist.py:
`run(..., residual=)`, `combine_residual`, `run_until`).

Ranks are threads that talk through tests/fabric.py, as in tests/test_dist.py;
every rank runs the real slab decomposition, exchange schedule and kernels.
The yardstick is the oracle on the whole grid (tests/test_residual.py
`_expected`), all four fields compared with `==`."""
import struct

import numpy as np
import pytest

import fabric
import values
from test_residual import _expected, _fields, _inputs, _opts, _stencil


class _Gathering:
  """A fabric endpoint with torch.distributed's all_gather on top of its
  point-to-point calls."""

  def __init__(self, endpoint):
    self._ep = endpoint

  def __getattr__(self, name):
    return getattr(self._ep, name)

  def all_gather(self, parts, mine, group=None):
    world, rank = self._ep.get_world_size(), self._ep.get_rank()
    ops = [self._ep.P2POp(self._ep.isend, mine, p)
           for p in range(world) if p != rank]
    ops += [self._ep.P2POp(self._ep.irecv, parts[p], p)
            for p in range(world) if p != rank]
    for req in self._ep.batch_isend_irecv(ops):
      req.wait()
    parts[rank].copy_(mine)


def _raw(changed, unordered, max_float, max_int):
  return struct.pack('<QQdQ', changed, unordered, max_float, max_int)


def test_fold_is_exact():
  from soda_amd import dist as sdist
  big = 2**64 - 1
  got = sdist.fold_residuals([_raw(3, 1, 0.5, 7), _raw(2**40, 0, float('inf'),
                                                      big),
                              _raw(0, 0, 0.0, 0)])
  assert _fields(got) == (2**40 + 3, 1, float('inf'), big)
  assert _fields(sdist.fold_residuals([_raw(0, 0, 0.0, 0)] * 3)) == \
      (0, 0, 0.0, 0)


@pytest.mark.parametrize('world', [1, 2, 3])
def test_combine_gathers_bytes_and_every_rank_agrees(world):
  """max_int above 2^63 (uint64 cells) survives: the bytes are gathered, never
  reduced as signed integers."""
  from soda_amd import dist as sdist
  shares = [_raw(10 * (r + 1), r, 0.25 * (r + 1), 2**63 + r)
            for r in range(world)]

  def rank_fn(rank, endpoint):
    return _fields(sdist.combine_residual(shares[rank], _Gathering(endpoint)))

  got = fabric.run_ranks(world, rank_fn)
  want = (sum(10 * (r + 1) for r in range(world)), sum(range(world)),
          0.25 * world, 2**63 + world - 1)
  assert got == [want] * world
  with pytest.raises(Exception, match='32 bytes'):
    sdist.combine_residual(b'\0' * 16, None)


def test_run_hands_the_residual_to_the_last_round_only():
  """dist.run with a recording engine: 13 iterations every 4 are rounds of 4,
  4, 4, 1; only the last is called with keep / residual / box_iterate, and
  box_iterate counts the iterations of earlier chained runs."""
  from soda_amd import dist as sdist
  stencil = _stencil('jacobi2d.soda', iterate=13)
  slab = sdist.Slab(stencil, (64, 60), 1, 0, 4)
  calls = []

  def step(dst, src, extent, iters, **kw):
    calls.append((iters, kw))

  sdist.run(slab, ['a'], ['b'], ['c'], step, 13, None, residual=4096,
            iterations_before=20)
  assert [c[0] for c in calls] == [4, 4, 4, 1]
  assert [c[1] for c in calls[:3]] == [{}] * 3
  assert calls[3][1] == dict(keep=slab.keep, residual=4096, box_iterate=33)
  del calls[:]
  sdist.run(slab, ['a'], ['b'], ['c'], step, 8, None)
  assert [c[1] for c in calls] == [{}] * 2


# ---------------------------------------------------------------------------
# GPU: thread ranks on one device
# ---------------------------------------------------------------------------

def _rank_engine(prog, slab, compute):
  def step(dst, cur, lext, iters, **kw):
    prog.run_device([t.data_ptr() for t in dst], [t.data_ptr() for t in cur],
                    lext, iterate=iters, stream=compute.cuda_stream,
                    origin=slab.origin, global_extent=slab.extent, **kw)
  return step


@pytest.mark.gpu
@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('border', ['ignore', 'preserve'])
def test_ranks_combine_to_the_oracles_figures(built, world, border):
  """jacobi2d 520 x 120, exchange every 4, overlapped: 12 iterations (a fused
  twin in the last round), then 13 more chained on the result (a last round of
  one iteration, the box of 25)."""
  import torch
  from soda_amd import dist as sdist, runtime
  extent, every = (520, 120), 4
  stencil = _stencil('jacobi2d.soda', iterate=13, border=border)
  ins = _inputs(stencil, extent)
  want12, _ = _expected(stencil, ins, extent, 12)
  want25, cur25 = _expected(stencil, ins, extent, 25)
  slabs = [sdist.Slab(stencil, extent, world, r, every) for r in range(world)]
  progs = [runtime.Program(stencil, _opts(fuse=(4,)), extent=s.local_extent,
                           calibrate=False) for s in slabs]

  def rank_fn(rank, endpoint):
    slab, prog, ep = slabs[rank], progs[rank], _Gathering(endpoint)
    compute = torch.cuda.Stream()
    with torch.cuda.stream(compute):
      hider = sdist.StreamOverlap(0)
      src = [torch.from_numpy(np.ascontiguousarray(
          ins[n][slab.begin:slab.end])).cuda() for n in stencil.input_names]
      work = [[torch.empty_like(t) for t in src] for _ in range(2)]
      struct32 = torch.full((4,), -1, dtype=torch.int64, device='cuda')
      step = _rank_engine(prog, slab, compute)

      def fetch():
        compute.synchronize()
        hider.comm.synchronize()
        return struct32.cpu()

      res = sdist.run(slab, src, work[0], work[1], step, 12, ep,
                      overlap=hider, residual=struct32.data_ptr())
      first = sdist.combine_residual(fetch(), ep)
      how = prog.last_residual()
      others = [x for x in [src] + work if x[0] is not res[0]]
      res = sdist.run(slab, res, others[0], others[1], step, 13, ep,
                      ghosts_fresh=False, overlap=hider,
                      residual=struct32.data_ptr(), iterations_before=12)
      second = sdist.combine_residual(fetch(), ep)
      own = res[0][slab.ghost_lo:slab.ghost_lo + slab.own_rows].cpu().numpy()
    return _fields(first), how, _fields(second), prog.last_residual(), own

  try:
    got = fabric.run_ranks(world, rank_fn)
  finally:
    for p in progs:
      p.close()
  assert [g[0] for g in got] == [want12] * world
  assert [g[1] for g in got] == [('twin', 4)] * world
  assert [g[2] for g in got] == [want25] * world
  assert [g[3] for g in got] == [('twin', 1)] * world
  whole = np.concatenate([g[4] for g in got], axis=0)
  lo, hi = stencil.valid_box(extent, 't0', 25)
  box = tuple(slice(l, max(l, h)) for l, h in zip(lo, hi))[::-1]
  assert values.same_bits(whole[box], cur25['t0'][box]).all()


@pytest.mark.gpu
def test_ranks_run_until(built):
  """The table of test_residual.py: jacobi2d `preserve`, shape (40, 64),
  default_rng(7), two ranks, a check every 16 iterations: a tolerance between
  the maxima of 16 and 32 iterations stops both ranks at 32."""
  import torch
  from soda_amd import dist as sdist, runtime
  extent, world = (64, 40), 2
  stencil = _stencil('jacobi2d.soda', iterate=16, border='preserve')
  ins = {'t1': np.random.default_rng(7).random((40, 64), dtype=np.float32)}
  want, cur = _expected(stencil, ins, extent, 32)
  assert want[0] == 2356 and abs(want[2] - 0.002126694) < 1e-8
  slabs = [sdist.Slab(stencil, extent, world, r, 4) for r in range(world)]
  progs = [runtime.Program(stencil, _opts(fuse=(4,)), extent=s.local_extent,
                           calibrate=False) for s in slabs]

  def rank_fn(rank, endpoint):
    slab, prog, ep = slabs[rank], progs[rank], _Gathering(endpoint)
    compute = torch.cuda.Stream()
    with torch.cuda.stream(compute):
      src = [torch.from_numpy(np.ascontiguousarray(
          ins['t1'][slab.begin:slab.end])).cuda()]
      work = [[torch.empty_like(t) for t in src] for _ in range(2)]
      struct32 = torch.zeros((4,), dtype=torch.int64, device='cuda')

      def fetch():
        compute.synchronize()
        return struct32.cpu()

      res, done, r = sdist.run_until(
          slab, src, work[0], work[1], _rank_engine(prog, slab, compute),
          struct32.data_ptr(), fetch, 0.003, 200, ep, check_every=16)
      compute.synchronize()
      own = res[0][slab.ghost_lo:slab.ghost_lo + slab.own_rows].cpu().numpy()
    return done, _fields(r), own

  try:
    got = fabric.run_ranks(world, rank_fn)
  finally:
    for p in progs:
      p.close()
  assert [g[0] for g in got] == [32, 32]
  assert [g[1] for g in got] == [want, want]
  assert values.same_bits(np.concatenate([g[2] for g in got], axis=0),
                          cur['t0']).all()
