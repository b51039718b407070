#!/usr/bin/env python3
"""Headline benchmark: jacobi2d fp32 on an 8192 x 8192 grid, iterate = 100.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--full]
                  [--dump-outputs DIR]

One "step" = one full pass of the hot path over one batch of synthetic input:
all 100 iterations of the program on the whole grid, inputs resident in HBM.
Metric: cells*iters/s (BASELINE.json).  N > 1: launched by torchrun, one rank
per GPU; the same 8192^2 grid is cut into slabs along the streamed dimension
(strong scaling) with halo exchange over RCCL (soda_amd/dist.py).

A plain run sets up, spins untimed until the clocks settle, restarts from the
seeded input, warms up (W steps, then a fixed number of settling steps), times
K chained steps and prints the JSON line; `--dump-outputs DIR` writes what the
last timed step computed -- the same bits on every run of the same arguments.
With `--full` the JSON line also carries
  roofline      HBM roofline of the dominant kernel: algorithmic bytes per
                launch / its average duration measured here with HIP events on
                the launch stream;
  cpu_baseline  the CPU oracle ("port" of the reference's loop nest, OpenMP on
                all host cores) timed on a bounded sample -- rank 0, N = 1 only;
  single_iter   the same workload with one iteration per launch (no temporal
                blocking), for the "LDS/register halo tile" config of BASELINE;
  rehearsed_scaling  (N = 1) what an N-GPU job would score if every rank ran
                its slab at the speed measured here for the middle rank's slab
                (compute only, no exchange);
  other_configs BASELINE's C3 / C4 / C5 on this GPU;
  parity        the result check of one more step against the CPU oracle.

N > 1 under torchrun: every step opens with a halo exchange; `--overlap auto`
(default) times a few steps with the exchange hidden under the compute
(soda_hip_run_device_slab) and a few without, all ranks agree on the faster
way (MAX over ranks), and the timed steps use it.  `--group`: ONE process
drives all N GPUs through soda_hip_group_* instead (peer copies, no RCCL);
`--group --virtual` puts the N slabs on one GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# --dump-outputs: cells per output array at most (4 Mi: 16 MiB as float32),
# and bytes of all outputs together at most
DUMP_CELLS = 1 << 22
DUMP_BYTES = 48 << 20
DUMP_SEED = 1234
# untimed chained steps after the restart from the seeded input, on top of
# --warmup, counted in iterations: the timed steps run on a field smoothed as
# far as in the sustained runs of earlier versions (500 steps of the headline)
SETTLE_ITERATIONS = 50000


def parse_args():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  # (a step is ~1.2 ms: a few hundred of them bring the GPU to the clocks it
  # sustains -- 20 steps right after idle read 5-6 % slower than 200)
  ap.add_argument('--steps', type=int, default=200)
  ap.add_argument('--warmup', type=int, default=50)
  ap.add_argument('--soda', default=os.path.join(
      ROOT, 'tests', 'golden', 'soda', 'jacobi2d.soda'))
  ap.add_argument('--extent', type=int, nargs='+', default=[8192, 8192])
  ap.add_argument('--iterate', type=int, default=100)
  ap.add_argument('--fuse', type=int, nargs='+', default=None,
                  help='iterations one launch may fuse (temporal blocking); '
                  'the library mixes the depths per extent so that they add '
                  'up to iterate at the least total time (100 = 4 x 13 + '
                  '4 x 12); default: soda_amd.codegen.hip.lower.DEFAULT_FUSE')
  ap.add_argument('--chunk-rows', type=int, default=None,
                  help='rows per wave; default: sized per kernel and GPU')
  ap.add_argument('--prefetch', type=int, default=None)
  ap.add_argument('--waves-x', type=int, default=1)
  ap.add_argument('--waves-y', type=int, default=1)
  ap.add_argument('--pipe', type=int, default=None,
                  help='wavefronts per block sharing the fused iterations')
  ap.add_argument('--strategy', default='auto')
  ap.add_argument('--exchange-every', type=int, default=0,
                  help='iterations between halo exchanges (N > 1); 0 = auto: '
                  'as many as keep the ghost rows below half a slab -- for '
                  'iterate=100 on 8192 rows that is all 100, i.e. the halo is '
                  'distributed once with the input, as the reference host '
                  'replicates it between tiles, and no exchange is needed')
  ap.add_argument('--scaling', choices=('strong', 'weak'), default='strong')
  ap.add_argument('--emulate-slab', type=int, default=0, metavar='N',
                  help='(rehearsal on one GPU) run the middle rank\'s slab of '
                  'an N-GPU run; only valid when no exchange is needed; the '
                  'JSON value is then what the N-GPU job would score if every '
                  'rank ran at this speed')
  ap.add_argument('--overlap', choices=('auto', 'on', 'off'), default='auto',
                  help='N > 1: hide the halo exchange under the compute')
  ap.add_argument('--group', action='store_true',
                  help='one process, N GPUs through soda_hip_group_* (peer '
                  'copies over xGMI) instead of one rank per GPU over RCCL')
  ap.add_argument('--virtual', action='store_true',
                  help='with --group: all N slabs on GPU 0')
  ap.add_argument('--no-rehearsal', action='store_true')
  ap.add_argument('--no-cpu-baseline', action='store_true')
  ap.add_argument('--no-parity', action='store_true',
                  help='skip the result check against the CPU oracle that '
                  'follows the timed region')
  ap.add_argument('--clock-warm-seconds', type=float, default=0.6,
                  help='upper bound of the untimed spin in front of the timed '
                  'region (10-step windows until three in a row are within 1 %% '
                  'of the fastest seen, at least 100 steps)')
  ap.add_argument('--no-single-iter', action='store_true')
  ap.add_argument('--no-other-configs', action='store_true',
                  help='skip BASELINE configs C3 / C4 / C5 (measured after '
                  'the timed region, ~2 s)')
  ap.add_argument('--cpu-seconds', type=float, default=12.0,
                  help='target CPU time of the cpu_baseline sample')
  ap.add_argument('--full', action='store_true',
                  help='besides the headline, measure and check everything '
                  'else: roofline of every scheduled kernel, result check '
                  'against the CPU oracle, single_iter, C3 / C4 / C5, '
                  'rehearsed scaling, CPU baseline (the --no-* options drop '
                  'single legs of it)')
  ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                  help='after the timed steps, write what the last of them '
                  'computed as DIR/<output>.npy (float32, or float64 for '
                  'other cell types): the valid box of each output array, or '
                  'where that exceeds %d cells a fixed seeded sample of it '
                  '(the same cells on every run of the same arguments)' %
                  DUMP_CELLS)
  args = ap.parse_args()
  if args.steps < 1:
    ap.error('--steps must be at least 1')
  return args


def time_events(fn, stream, repeats):
  """Average milliseconds of fn() over `repeats` calls, HIP events recorded on
  the stream the kernels are launched on."""
  from soda_amd import runtime
  start, stop = runtime.Event(), runtime.Event()
  start.record(stream)
  for _ in range(repeats):
    fn()
  stop.record(stream)
  return start.elapsed_ms(stop) / repeats


def dump_outputs(path, stencil, extent, iterate, arrays):
  """--dump-outputs: `arrays` = the program's output arrays over the whole
  grid (dim-0-fastest tensors), as a step of `iterate` iterations left them.
  Writes DIR/<output>.npy: the valid box of the output, or, where the box
  holds more than `most` cells, the cells at `most` positions drawn from it
  with a fixed seed (duplicates dropped, in memory order) -- a 1-D array
  then."""
  import numpy as np
  import torch
  os.makedirs(path, exist_ok=True)
  most = min(DUMP_CELLS, DUMP_BYTES // (8 * len(arrays)))
  for t, name, typ in zip(arrays, stencil.output_names, stencil.output_types):
    lo, hi = stencil.valid_box(extent, name, iterate)
    box = t[tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))]
    if box.numel() > most:
      rng = np.random.default_rng(DUMP_SEED)
      flat = np.unique(rng.integers(0, box.numel(), most))
      at = tuple(torch.from_numpy(np.ascontiguousarray(c)).to(t.device)
                 for c in np.unravel_index(flat, tuple(box.shape)))
      box = box[at]
    cells = box.contiguous().cpu().numpy().view(typ.np_name)
    out = cells.astype(np.float32 if cells.dtype == np.float32 else np.float64)
    np.save(os.path.join(path, '%s.npy' % name), out)


def cpu_baseline(stencil, extent, target_seconds):
  """The CPU oracle on a bounded sample of the same workload."""
  import numpy as np
  from oracle import c_oracle
  orc = c_oracle.COracle(stencil, openmp=True)
  cores = orc.max_threads
  rng = np.random.default_rng(0)
  a = {n: rng.random(tuple(extent[::-1]), dtype=np.float32)
       for n in stencil.input_names}
  cells = 1
  for e in extent:
    cells *= e
  orc.run(a, iterate=1)    # first touch: page faults, thread pool
  t0 = time.time()
  orc.run(a, iterate=4)
  t4 = time.time() - t0
  t0 = time.time()
  orc.run(a, iterate=20)
  probe = max(1e-4, (time.time() - t0 - t4) / 16)   # per iteration, net of setup
  iters = int(max(2, min(2000, target_seconds / max(probe, 1e-6))))
  t0 = time.time()
  orc.run(a, iterate=iters)
  dt = time.time() - t0
  # g++ -O2 single-thread AND OpenMP.  One thread takes ~0.2 s
  # per iteration of this grid: a few iterations, stated
  one = c_oracle.COracle(stencil, openmp=False)
  one.run(a, iterate=1)
  t0 = time.time()
  one.run(a, iterate=1)
  t1 = max(1e-4, time.time() - t0)
  iters1 = int(max(2, min(200, 0.25 * target_seconds / t1)))
  t0 = time.time()
  one.run(a, iterate=iters1)
  dt1 = time.time() - t0
  return {
      'value': cells * iters / dt, 'unit': 'cells*iters/s', 'cores': cores,
      'kind': 'port',
      'sample': '%s %s, iterate=%d (%.1f s), gcc -O2 -ffp-contract=off -fwrapv '
                '-fopenmp, %d threads' % (stencil.app_name,
                                          'x'.join(map(str, extent)), iters,
                                          dt, cores),
      'single_thread': {
          'value': cells * iters1 / dt1, 'unit': 'cells*iters/s', 'cores': 1,
          'kind': 'port',
          'sample': '%s %s, iterate=%d (%.1f s), gcc -O2 -ffp-contract=off -fwrapv, '
                    '1 thread' % (stencil.app_name, 'x'.join(map(str, extent)),
                                  iters1, dt1),
      },
  }


def rehearse(args, stencil, extent, fuses, options, stream, value_1gpu):
  """Compute-only scaling, measured in this process: for N = 2, 4, 8 the slab
  of the middle rank of an N-GPU run (its ghost rows included, cone-trimmed
  passes, the library's schedule for that extent), `iterate` iterations per
  step.  {N: what the job would score at that speed}; no exchange is timed --
  the gap to the driver's measured N-GPU value is communication + imbalance."""
  import torch
  from soda_amd import dist as sdist, runtime
  out = {'1': value_1gpu}
  cells = 1
  for e in extent:
    cells *= e
  for n in (2, 4, 8):
    try:
      dry = runtime.resolve_options(stencil, options(fuses), extent)
      fuse = 1
      if dry.fuse:
        fuse = max(dry.fuse)
      ex = sdist.planned_exchange_every(stencil, extent, n, args.iterate,
                                        options(fuses), multiple_of=fuse)
      slab = sdist.Slab(stencil, extent, n, n // 2, ex)
      lext = slab.local_extent
      with runtime.Program(stencil, options(fuses), extent=lext,
                           calibrate=True) as prog:
        shape = tuple(lext[::-1])
        a = [torch.rand(shape, device='cuda') for _ in stencil.input_names]
        b = [torch.empty_like(t) for t in a]

        def step():
          done, cur, nxt = 0, a, b
          while done < args.iterate:
            k = min(ex, args.iterate - done)
            prog.run_device([t.data_ptr() for t in nxt],
                            [t.data_ptr() for t in cur], lext, iterate=k,
                            stream=stream, origin=slab.origin,
                            global_extent=slab.extent, keep=slab.keep)
            cur, nxt = nxt, cur
            done += k

        step()
        torch.cuda.synchronize()
        ms = time_events(step, stream, 5)
      out[str(n)] = cells * args.iterate / (ms * 1e-3)
      out['slab_ms_%d' % n] = ms
    except Exception as e:        # a rehearsal must not take the bench down
      out[str(n)] = None
      out['error_%d' % n] = str(e)[:160]
  out['what'] = ('cells*iters/s of the whole job if every rank ran its slab '
                 'at the speed of the middle rank\'s slab measured on this '
                 'GPU; compute only')
  return out


def other_configs(stream):
  """BASELINE.json's other single-GPU configurations on this GPU, measured
  AFTER the timed region (the reference's host prints throughput
  for every run it makes, frt/host.py:324-335; until now only C2 was in the
  driver's line): C3 blur 16384^2 (fused two-stage, u16), C4 heat3d 512^3 x 50
  on one GPU, C5 jacobi2d 8192^2 x 1000 -- inputs resident, the whole run
  between HIP events on the launch stream, then the dominant pass alone for
  its roofline fraction.  Parity of these configs at full size is the GPU test
  suite's (tests/test_baseline_configs.py, test_hip_parity.py), not this
  leg's."""
  import torch
  from soda_amd import core, isa, runtime
  from soda_amd.codegen.hip import lower
  soda = os.path.join(ROOT, 'tests', 'golden', 'soda')
  tdt = {'float32': torch.float32, 'uint16': torch.int16,
         'int16': torch.int16}
  rows = []
  for label, name, extent, iterate, fuse, reps in (
      ('C3', 'blur.soda', (16384, 16384), 1, (), 10),
      ('C4', 'heat3d.soda', (512, 512, 512), 50, (2,), 3),
      ('C5', 'jacobi2d.soda', (8192, 8192), 1000, lower.DEFAULT_FUSE, 2)):
    row = {'config': label, 'workload': '%s %s iterate=%d' % (
        name[:-5], 'x'.join(map(str, extent)), iterate)}
    try:
      st = core.from_file(os.path.join(soda, name), iterate=iterate)
      shape = tuple(extent[::-1])
      ins = []
      for t in st.input_types:
        dt = tdt[t.np_name]
        ins.append(torch.rand(shape, device='cuda', dtype=dt)
                   if dt.is_floating_point else
                   torch.randint(0, 30000, shape, device='cuda', dtype=dt))
      outs = [torch.empty(shape, device='cuda', dtype=tdt[t.np_name])
              for t in st.output_types]
      table = st.symbol_table
      bpc = (sum(table[n].size_in_bytes for n in st.input_names) +
             sum(table[n].size_in_bytes for n in st.output_names))
      cells = 1
      for e in extent:
        cells *= e
      with runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=extent,
                           calibrate=True) as prog:

        def go(iters=iterate):
          prog.run_device([t.data_ptr() for t in outs],
                          [t.data_ptr() for t in ins], extent, iterate=iters,
                          stream=stream)

        go()
        torch.cuda.synchronize()
        ms = time_events(go, stream, reps)
        launches = prog.last_launches()[0]
        sched = prog.schedule(extent, iterate)
        us = prog.pass_times(extent)[0]
        depth = max(sched, key=lambda t: sched[t] * us.get(t, float(t)))
        n = min(8, max(1, iterate // depth))
        while n > 1 and prog.schedule(extent, depth * n) != {depth: n}:
          n -= 1
        kernel_ms = None
        if prog.schedule(extent, depth * n) == {depth: n}:
          go(depth * n)
          kernel_ms = time_events(lambda: go(depth * n), stream,
                                  max(1, 16 // n)) / n
        ps = [p for p in prog.module.sorted_passes() if p.fused_iters == depth]
        kname = prog.module.kernels[ps[0].kernels[0]].name
        row.update({
            'ms': ms, 'value': cells * iterate / (ms * 1e-3),
            'unit': 'cells*iters/s', 'launches': launches,
            'schedule': {str(t): c for t, c in sched.items()},
            'dtype': str(table[st.input_names[0]]),
            'kernel': kname, 'isa_key': isa.isa_key(prog.code, kname),
            'kernel_family': ps[0].kind, 'iterations_per_launch': depth,
            'kernel_ms': kernel_ms,
        })
        if kernel_ms:
          ach = cells * bpc / (kernel_ms * 1e-3) / 1e9
          row['roofline'] = {'bound': 'hbm', 'achieved': ach,
                             'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                             'frac': ach / HBM_PEAK_GBS,
                             'algorithmic_bytes_per_launch': cells * bpc}
          try:
            st_k = isa.module_static(prog.module, prog.code,
                                     prog.geometry(extent)[0],
                                     extent).get(kname)
          except Exception:     # noqa: BLE001
            st_k = None
          if st_k:
            row['roofline']['valu_frac'] = st_k['min_issue_ms'] / kernel_ms
            if row['roofline']['valu_frac'] > row['roofline']['frac']:
              row['roofline']['bound'] = 'valu'
      del ins, outs
    except Exception as e:        # a side measurement must not take the bench down
      row['error'] = '%s: %s' % (type(e).__name__, str(e)[:200])
    rows.append(row)
  return rows


def group_main(args):
  """`--group`: one process, one host thread, N GPUs (or N virtual slabs on
  GPU 0) through soda_hip_group_*: peer copies instead of RCCL."""
  import numpy as np
  import torch
  from soda_amd import core, runtime
  from soda_amd.codegen.hip import lower
  n = args.gpus
  have = torch.cuda.device_count()
  if not args.virtual and have < n:
    sys.stderr.write('bench.py: --group --gpus %d needs %d GPUs, %d visible '
                     '(--virtual runs the slabs on one)\n' % (n, n, have))
    sys.exit(2)
  stencil = core.from_file(args.soda, iterate=args.iterate)
  extent = list(args.extent)
  if args.scaling == 'weak' and n > 1:
    extent[-1] *= n
  fuses = sorted({f for f in args.fuse if f >= 1}, reverse=True)
  opts = lower.LowerOptions(strategy=args.strategy,
                            fuse=tuple(f for f in fuses if f > 1),
                            prefetch=args.prefetch, pipe=args.pipe)
  devices = [0] * n if args.virtual else list(range(n))
  rows = {}
  for way in ((True, False) if args.overlap == 'auto' and n > 1 else
              (args.overlap != 'off',)):
    with runtime.Group(stencil, extent, devices, opts,
                       exchange_every=args.exchange_every, overlap=way,
                       calibrate=True) as group:
      rng = np.random.default_rng(1234)
      group.load({name: rng.random(tuple(extent[::-1]), dtype=np.float32)
                  for name in stencil.input_names})
      for _ in range(max(1, args.warmup)):
        group.run()
      group.synchronize()
      enq = 0.0
      t0 = time.perf_counter()
      for _ in range(args.steps):
        group.run()
        enq += group.stats()['enqueue_ms']
      group.synchronize()
      dt = time.perf_counter() - t0
      st = group.stats()
      rows[way] = (dt, enq, st)
  way = min(rows, key=lambda w: rows[w][0])
  dt, enq, st = rows[way]
  cells = 1
  for e in extent:
    cells *= e
  table = stencil.symbol_table
  parity = None
  if args.full and not args.no_parity:
    # the same result check as the rank-per-GPU path: two chained steps from
    # the seeded input (the second opens with the exchange), gathered by the
    # library, against the CPU oracle (test infrastructure, the checker only)
    from oracle import c_oracle
    with runtime.Group(stencil, extent, devices, opts,
                       exchange_every=args.exchange_every, overlap=way,
                       calibrate=True) as group:
      rng = np.random.default_rng(1234)
      host_in = {name: rng.random(tuple(extent[::-1]), dtype=np.float32)
                 for name in stencil.input_names}
      group.load(host_in)
      group.run()
      group.run()
      got = group.store(2 * args.iterate)
    want = c_oracle.COracle(stencil, openmp=True).run(
        host_in, iterate=2 * args.iterate)
    checked = bad = 0
    for o in stencil.output_names:
      lo, hi = stencil.valid_box(extent, o, 2 * args.iterate)
      idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
      g = np.ascontiguousarray(got[o][idx]).view(np.uint32)
      w = np.ascontiguousarray(want[o][idx]).view(np.uint32)
      checked += int(g.size)
      bad += int((g != w).sum())
    parity = {'cells': checked, 'mismatches': bad,
              'against': 'oracle/c_oracle.py (OpenMP), %d iterations from the '
                         'seeded input, valid box, bit for bit' %
                         (2 * args.iterate)}
  print(json.dumps({
      'metric': 'stencil cells*iters/s, %s %s iterate=%d' %
                (stencil.app_name, 'x'.join(map(str, extent)), args.iterate),
      'value': cells * args.iterate * args.steps / dt,
      'unit': 'cells*iters/s', 'n_gpus': n, 'rccl_world': 0,
      'steps': args.steps, 'warmup': args.warmup,
      'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True,
      'scaling': args.scaling, 'vs_baseline': None, 'dtype': 'f32',
      'data': 'synthetic',
      'config': {
          'workload': '%s %s %s iterate=%d' % (
              stencil.app_name, str(table[stencil.input_names[0]]),
              'x'.join(map(str, extent)), args.iterate),
          'transport': 'one process, soda_hip_group_*: peer copies'
                       + (' between %d virtual slabs on GPU 0' % n
                          if args.virtual else ' over xGMI'),
          'overlap': bool(way),
          'ms_per_step_by_overlap': {str(w): rows[w][0] / args.steps * 1e3
                                     for w in rows},
          'exchange_every': st['exchange_every'],
          'exchanges_per_step': st['exchanges'],
          'launches_per_step': st['launches'],
          'split_passes_per_step': st['split_passes'],
          'copy_bytes_per_step': st['copy_bytes'],
          'host_enqueue_ms_per_step': enq / args.steps,
      },
      **({'parity': parity} if parity else {}),
  }))
  if parity and parity['mismatches']:
    sys.stderr.write('bench.py: the checked steps differ from the oracle in '
                     '%d cells\n' % parity['mismatches'])
    sys.exit(3)


class HostStagedP2P:
  """(REHEARSAL transports only.)  soda_amd.dist orders a halo exchange on a
  HIP stream, which is what RCCL's send / recv do.  gloo does not: handed a
  device tensor, its send / recv threads read and write the GPU's memory
  through the CPU's mapping of it whenever they get to it -- unordered against
  every stream, past the GPU's caches (round 4: the result check this file
  gained caught 2359 wrong cells in one of four two-rank rehearsals).  For any
  backend but nccl the point-to-point calls therefore go through host buffers:
  a send copies its rows out behind the current stream first, a receive lands
  in a host buffer and is copied in on the current stream by wait().  The
  collectives (all_reduce, broadcast, all_gather, barrier) are gloo's own,
  which do stage device tensors correctly."""
  isend, irecv = 'isend', 'irecv'

  class _Req:

    def __init__(self, work, tensor=None, host=None):
      self.work, self.tensor, self.host = work, tensor, host

    def wait(self):
      self.work.wait()
      if self.tensor is not None:
        self.tensor.copy_(self.host)       # on the caller's current stream

  def __init__(self, tdist):
    self._t = tdist

  def __getattr__(self, name):
    return getattr(self._t, name)

  @staticmethod
  def P2POp(op, tensor, peer, group=None):
    return (op, tensor, peer, group)

  def batch_isend_irecv(self, ops):
    import torch
    reqs = []
    for op, tensor, peer, group in ops:     # sends first: they never block
      if op == self.isend:
        host = tensor.cpu()                 # behind the current stream
        reqs.append(self._Req(self._t.isend(host, peer, group), host=host))
    for op, tensor, peer, group in ops:
      if op == self.irecv:
        host = torch.empty(tensor.shape, dtype=tensor.dtype, device='cpu')
        reqs.append(self._Req(self._t.irecv(host, peer, group), tensor, host))
    return reqs


def launch_ranks(args) -> int:
  """`bench.py --gpus N` started by hand (no WORLD_SIZE in the environment):
  this process becomes the launcher.  It touches no GPU (counting devices does
  not initialise one), starts N fresh rank processes through torchrun on the
  loopback address and returns their exit status; rank 0 writes the JSON line
  straight to the stdout the ranks inherit."""
  import socket
  import subprocess
  import torch
  have = torch.cuda.device_count()
  if have < args.gpus:
    sys.stderr.write('bench.py: --gpus %d needs %d GPUs on this node, %d '
                     'visible; nothing was launched\n' %
                     (args.gpus, args.gpus, have))
    return 2
  sock = socket.socket()
  sock.bind(('127.0.0.1', 0))
  port = sock.getsockname()[1]
  sock.close()
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
         '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
  env = dict(os.environ)
  env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC only (RCCL)
  return subprocess.run(cmd, env=env).returncode


def main():
  args = parse_args()
  if args.fuse is None:
    from soda_amd.codegen.hip import lower as _lower
    args.fuse = list(_lower.DEFAULT_FUSE)
  # the C-ABI library is a build artefact (git-ignored): make sure it exists;
  # a no-op when it is newer than its sources
  import __graft_entry__ as entry
  entry.build_library()
  if args.dump_outputs and (args.group or args.emulate_slab > 1):
    raise SystemExit('bench.py: --dump-outputs writes the whole grid of the '
                     'rank-per-GPU path; not with --group or --emulate-slab')
  if args.group:
    return group_main(args)
  if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
    sys.exit(launch_ranks(args))
  import torch
  from soda_amd import core, dist as sdist, runtime
  from soda_amd.codegen.hip import lower

  world = int(os.environ.get('WORLD_SIZE', '1'))
  rank = int(os.environ.get('RANK', '0'))
  emulate = args.emulate_slab if world == 1 else 0
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  if world != args.gpus:
    raise SystemExit('WORLD_SIZE=%d but --gpus %d' % (world, args.gpus))
  # Rehearsal on a box with ONE GPU (tests/test_dist.py): SODA_BENCH_ONE_GPU=1
  # maps every rank to device 0 and SODA_BENCH_BACKEND=gloo carries the halos
  # (RCCL refuses two ranks on one device); the code path is otherwise the
  # N-GPU one.  Never set by the driver.
  backend = os.environ.get('SODA_BENCH_BACKEND', 'nccl')
  if os.environ.get('SODA_BENCH_ONE_GPU'):
    local_rank = 0
  torch.cuda.set_device(local_rank)
  dev = torch.device('cuda', local_rank)
  tdist = None
  force_dist = bool(os.environ.get('SODA_BENCH_FORCE_DIST'))  # 1-rank rehearsal
  if world > 1 or force_dist:
    import torch.distributed as tdist
    if force_dist and 'RANK' not in os.environ:
      os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
      os.environ.setdefault('MASTER_PORT', '29531')
      tdist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
    elif backend != 'nccl':
      tdist.init_process_group(backend)
      tdist = HostStagedP2P(tdist)     # (a rehearsal: see the class)
    else:
      tdist.init_process_group('nccl', device_id=dev)
    rccl_world = tdist.get_world_size()
  else:
    rccl_world = 0      # one rank: no process group, RCCL not involved

  stencil = core.from_file(args.soda, iterate=args.iterate)
  extent = list(args.extent)
  if args.scaling == 'weak' and world > 1:
    extent[-1] *= world
  fuses = sorted({f for f in args.fuse if f >= 1}, reverse=True)

  def options(fuse_list):
    return lower.LowerOptions(strategy=args.strategy,
                              fuse=tuple(f for f in fuse_list if f > 1),
                              chunk_rows=args.chunk_rows,
                              prefetch=args.prefetch, waves_x=args.waves_x,
                              waves_y=args.waves_y, pipe=args.pipe)

  # the depth the lowering really fuses (3-D programs cap it, a program that
  # cannot iterate has none): a dry lowering tells, no GPU needed
  dry = runtime.resolve_options(stencil, options(fuses), extent)
  fuse = lower.lower(stencil, dry).sorted_passes()[0].fused_iters
  geo_world, geo_rank = (emulate, emulate // 2) if emulate > 1 else (world, rank)
  if geo_world == 1:
    ex = args.iterate
  elif args.exchange_every > 0:
    ex = args.exchange_every
    if fuse > 1:
      ex = max(fuse, ex // fuse * fuse)
  else:
    # the library's cost choice (pass times of the slab extent a candidate
    # implies against a transfer model; soda_hip_group_plan, no GPU needed),
    # the quarter-slab rule if it cannot be made.  Every rank must use the same
    # interval: rank 0's counts
    ex = sdist.planned_exchange_every(stencil, extent, geo_world, args.iterate,
                                      options(fuses), multiple_of=fuse,
                                      overlap=args.overlap != 'off')
    if tdist is not None and world > 1:
      t = torch.tensor([ex], dtype=torch.int64,
                       device=dev if backend == 'nccl' else 'cpu')
      tdist.broadcast(t, 0)
      ex = int(t.item())
  slab = sdist.Slab(stencil, extent, geo_world, geo_rank, ex)
  if emulate > 1:
    if sdist.rounds(args.iterate, ex) > 1:
      raise SystemExit('--emulate-slab needs an exchange-free schedule')
    slab.world = 1   # no peers: exchange() is a no-op
  local_extent = slab.local_extent

  # calibrate: the library times one launch of every pass on this rank's
  # extent and schedules the iterations by the clock (soda_hip_program_calibrate)
  prog = runtime.Program(stencil, options(fuses), device=local_rank,
                         extent=local_extent, calibrate=True)
  stream = torch.cuda.current_stream().cuda_stream

  # synthetic input: the same seeded global field on every rank, sliced
  shape = tuple(extent[::-1])
  np_dtypes = {'float32': torch.float32, 'float64': torch.float64,
               'uint16': torch.int16, 'int16': torch.int16,
               'int32': torch.int32}

  def seeded_fields():
    """The global input fields, one after the other (a generator: 256 MiB each
    at the headline size) -- the same on every rank and on every call."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    for name, t in zip(stencil.input_names, stencil.input_types):
      dt = np_dtypes[t.np_name]
      if dt.is_floating_point:
        yield torch.rand(shape, generator=gen, device=dev, dtype=dt)
      else:
        yield torch.randint(0, 30000, shape, generator=gen, device=dev,
                            dtype=dt)

  a_bufs, b_bufs, c_bufs = [], [], []
  for full in seeded_fields():
    a_bufs.append(full[slab.begin:slab.end].clone())
    del full
    b_bufs.append(torch.empty_like(a_bufs[-1]))
    if world > 1:
      c_bufs.append(torch.empty_like(a_bufs[-1]))
  torch.cuda.synchronize()

  hider = sdist.StreamOverlap(local_rank) if world > 1 else None

  def step_fn(dst, src, lext, iters, **kw):
    kw.setdefault('keep', slab.keep)
    if hider is not None and not kw.get('sendable'):
      # a run that records no `sendable` (a serial step, a timing loop): the
      # next overlapped exchange must wait for everything on the launch stream
      hider.invalidate()
    prog.run_device([t.data_ptr() for t in dst], [t.data_ptr() for t in src],
                    lext, iterate=iters, stream=stream, origin=slab.origin,
                    global_extent=slab.extent, **kw)

  mode = {'overlap': world > 1 and args.overlap != 'off'}

  # A sustained iterated run: the input of a step is the output of the step
  # before it.  On N > 1 GPUs the ghost rows of that input are stale, so every
  # step opens with a halo exchange (then one more per K iterations, if K <
  # iterate); the arrays rotate through the pool and the array that holds the
  # state is never written while it is read.
  pool = [a_bufs, b_bufs] + ([c_bufs] if c_bufs else [])
  chain = {'cur': a_bufs, 'first': True}

  def one_step():
    cur = chain['cur']
    others = [x for x in pool if x is not cur]
    res = sdist.run(slab, cur, others[0], others[-1], step_fn, args.iterate,
                    tdist, ghosts_fresh=chain['first'] or world == 1,
                    overlap=hider if mode['overlap'] else None)
    chain['first'] = False
    chain['cur'] = next(x for x in pool if x[0] is res[0])
    return res

  def barrier():
    if tdist is not None:
      tdist.barrier()

  # ---- the dominant kernel (this rank's slab) --------------------------------
  table = stencil.symbol_table
  bytes_cell = (sum(table[n].size_in_bytes for n in stencil.input_names) +
                sum(table[n].size_in_bytes for n in stencil.output_names))
  local_cells = 1
  for e in local_extent:
    local_cells *= e

  # The dominant kernel = the scheduled pass with the largest share of a
  # step's time (the schedule may mix depths: 100 = 4 x 13 + 4 x 12), timed
  # exactly as the step runs it: `per_call` launches in a row, state rotating
  # through the program's work arrays (a kernel that re-reads ONE input array
  # from the 256 MiB Infinity Cache times differently).  The run entry only
  # takes an iteration count, so the count is chosen such that the library's
  # schedule for it consists of that pass alone.
  interval = min(ex, args.iterate)
  sched = prog.schedule(local_extent, interval)
  cal_us = prog.pass_times(local_extent)[0]

  def pure_calls(depth):
    n = max(1, args.iterate // depth) if depth > 1 else 8
    while n > 1 and prog.schedule(local_extent, depth * n) != {depth: n}:
      n -= 1
    return n

  fuse_deepest = fuse
  fuse = max(sched, key=lambda t: sched[t] * cal_us.get(t, float(t)))
  passes = [p for p in prog.module.sorted_passes() if p.fused_iters == fuse]
  kname = prog.module.kernels[passes[0].kernels[0]].name if passes else '?'
  alg_bytes = float(local_cells) * bytes_cell

  roofline = None
  if args.full:
    # ---- roofline of the dominant kernel, HIP events (--full) ---------------
    # Measured BEFORE the timed region: it needs no result of it, and its ~60
    # launches bring the GPU to its sustained clocks, so a short --steps run is
    # not dominated by the first milliseconds after idle.
    per_call = pure_calls(fuse)
    if prog.schedule(local_extent, fuse * per_call) != {fuse: per_call}:
      raise SystemExit('cannot time pass T=%d alone' % fuse)

    def dominant():
      step_fn(b_bufs, a_bufs, local_extent, fuse * per_call)

    def time_pass(depth):
      n = pure_calls(depth)
      if prog.schedule(local_extent, depth * n) != {depth: n}:
        return None

      def go():
        step_fn(b_bufs, a_bufs, local_extent, depth * n)
      go()
      return time_events(go, stream, max(1, 24 // n)) / n

    dominant()
    torch.cuda.synchronize()
    calls = max(1, 48 // per_call)
    reps = calls * per_call
    kernel_ms = time_events(dominant, stream, calls) / per_call
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
    roofline = {
        'bound': 'hbm', 'achieved': achieved, 'peak': HBM_PEAK_GBS,
        'unit': 'GB/s', 'frac': achieved / HBM_PEAK_GBS, 'traffic': None,
        'kernel': kname, 'kernel_ms': kernel_ms,
        'algorithmic_bytes_per_launch': alg_bytes,
        'iterations_per_launch': fuse,
        'effective_GBs_at_8B_per_cell_iter': achieved * fuse,
        'timing': 'hipEvent pair around %d back-to-back launches on the '
                  'launch stream right after the timed steps, arrays rotating '
                  'as in a step' % reps,
    }
    # measured streaming roofline on THIS GPU: float4 copy, buffers rotating
    # as in an iterated run (the north star quotes its target against this)
    try:
      from soda_amd import streamcopy
      n = local_cells - local_cells % 4
      cp = streamcopy.StreamCopy(device=local_rank, unroll=1, nt_load=True)
      ring = [a_bufs[0], b_bufs[0], torch.empty_like(a_bufs[0])]
      state = {'i': 0}

      def copy_once():
        i = state['i']
        cp.run(ring[(i + 1) % 3].data_ptr(), ring[i % 3].data_ptr(), n, stream)
        state['i'] = i + 1

      copy_once()
      copy_ms = time_events(copy_once, stream, 30)
      copy_gbs = n * 8.0 / (copy_ms * 1e-3) / 1e9
      roofline['measured_copy_GBs'] = copy_gbs
      roofline['frac_of_measured_copy'] = achieved / copy_gbs
      cp.close()
      del ring
    except Exception as e:  # a measurement aid must not take the bench down
      roofline['measured_copy_GBs'] = None
      roofline['measured_copy_error'] = str(e)[:200]
    # PMC traffic is collected in separate rocprofv3 passes (tools/
    # profile_round.sh) and kept in profiles/traffic.json under the key of the
    # KERNEL it was measured on -- a hash of that kernel's machine code and
    # descriptor (soda_amd/isa.py; until round 4 the key covered the whole
    # module source, so an edit to a helper orphaned every number).  A number
    # taken on other code under the same name is dropped, not reported.
    from soda_amd import isa
    kernel_key = runtime.source_key(prog.module.source)
    roofline['kernel_key'] = kernel_key
    roofline['isa_key'] = isa.isa_key(prog.code, kname)
    roofline['compiler'] = runtime.compiler_version()
    # vector-ALU wave-instructions per launch counted from the code object
    # (straight-line prologue + loop body x trips, over the launch geometry):
    # the second roof of a temporally blocked stencil, present with or without
    # a PMC pass
    static = {}
    try:
      static = isa.module_static(prog.module, prog.code,
                                 prog.geometry(local_extent)[0], local_extent)
    except Exception as e:   # a measurement aid must not take the bench down
      roofline['static_error'] = '%s: %s' % (type(e).__name__, str(e)[:160])

    def valu_roof(name, ms, pmc_insts=None):
      st = static.get(name)
      if not st:
        return None
      out = {
          'wave_instructions_per_launch': st['valu_per_launch'],
          'min_issue_ms': st['min_issue_ms'],
          'frac_of_valu_issue_peak': st['min_issue_ms'] / ms if ms else None,
          'per_row_step': {k: st['%s_per_row_step' % k]
                           for k in ('valu', 'dpp', 'lds_crossbar',
                                     'vmem_load', 'vmem_store', 'waitcnt')},
          'source': 'static: llvm-objdump of the code object, loop body x '
                    'trips over the launch geometry (soda_amd/isa.py); peak = '
                    '1024 SIMDs x 2.4 GHz / 2 cycles per wave64 instruction',
      }
      if pmc_insts:
        out['measured_wave_instructions_per_launch'] = pmc_insts
        out['static_over_measured'] = st['valu_per_launch'] / pmc_insts
      return out

    def pmc_of(name, key):
      """The counter entry of profiles/traffic.json for `name`, if it was
      taken on this very machine code (else None and why)."""
      entry = traffic_table.get(name)
      if not entry:
        return None, None
      if entry.get('isa_key'):
        if entry['isa_key'] == key:
          return entry, None
        return None, ('profiles/traffic.json holds %s for machine code %s; '
                      'this run built %s' % (name, entry['isa_key'], key))
      if entry.get('kernel_key') == kernel_key:     # (files of rounds 1-4)
        return entry, None
      return None, ('profiles/traffic.json holds %s for module key %s; this '
                    'run built %s' % (name, entry.get('kernel_key'),
                                      kernel_key))

    traffic_file = os.path.join(ROOT, 'profiles', 'traffic.json')
    traffic_table = {}
    if os.path.exists(traffic_file):
      try:
        with open(traffic_file) as f:
          traffic_table = json.load(f)
      except (OSError, ValueError):
        traffic_table = {}
    pmc, why = pmc_of(kname, roofline['isa_key'])
    if why:
      roofline['traffic_dropped'] = why
    if pmc and pmc.get('hbm_bytes_per_launch'):
      roofline['traffic'] = pmc['hbm_bytes_per_launch']
      roofline['traffic_source'] = pmc.get('source')
    v = valu_roof(kname, kernel_ms,
                  (pmc or {}).get('valu_wave_instructions_per_launch'))
    if v:
      roofline['valu'] = v

  launches_per_step = 0
  overlap_trial = None
  if world > 1 and args.overlap == 'auto':
    # both ways, a few steps each; every rank must take the same decision
    trial = {}
    failed = None

    def guarded(n_steps):
      """n_steps steps; never raises: every rank reaches the collective that
      follows whatever happened here (a rank that left the sequence would
      leave the others in a barrier nobody completes)."""
      try:
        # (test hook: every rank fails its overlapped steps before touching a
        # peer -- what a refused argument or a missing symbol looks like)
        if mode['overlap'] and os.environ.get('SODA_BENCH_INJECT_OVERLAP_FAILURE'):
          raise RuntimeError('injected failure of the overlapped step')
        for _ in range(n_steps):
          one_step()
        torch.cuda.synchronize()
        return None
      except Exception as e:          # noqa: BLE001
        return '%s: %s' % (type(e).__name__, str(e)[:200])

    # (What this cannot cure: ONE rank failing in the middle of an exchange --
    # its peers then wait for a message inside one_step() and never reach the
    # reduction; RCCL's watchdog ends such a job.  Failures every rank sees at
    # the same point -- the realistic kind for a code path that has never run
    # on real links -- fall back to the serial exchange cleanly.)
    def any_rank(err):
      t = torch.tensor([1.0 if err else 0.0], device=dev, dtype=torch.float64)
      tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
      return float(t.item()) > 0

    for way in (True, False, True, False):
      if way and failed:              # (set from a reduced flag: same everywhere)
        continue
      mode['overlap'] = way
      err = guarded(1)
      bad = any_rank(err)             # doubles as the barrier in front of the clock
      dt = 0.0
      if not bad:
        t0 = time.perf_counter()
        err = guarded(3)
        dt = time.perf_counter() - t0
      t = torch.tensor([dt, 1.0 if err else 0.0], device=dev,
                       dtype=torch.float64)
      tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
      bad = bad or float(t[1].item()) > 0
      if bad:
        if not way:                   # the serial way is the fallback: give up
          raise SystemExit('bench.py: the serial exchange failed: %s' %
                           (err or 'on another rank'))
        failed = err or 'another rank failed'
        trial[True] = float('inf')
        # all ranks restart from the same point of the rotation
        chain['cur'] = a_bufs
        hider.invalidate()
        continue
      trial[way] = min(trial.get(way, 1e9), float(t[0].item()) / 3 * 1e3)
    mode['overlap'] = trial[True] <= trial[False]
    overlap_trial = {'overlapped_ms_per_step': trial[True]
                     if trial[True] != float('inf') else None,
                     'serial_ms_per_step': trial[False],
                     **({'overlapped_failed': failed} if failed else {})}
  # Bring the GPU to the clocks it sustains, OUTSIDE the timed region: a step
  # is ~1.2 ms, and 20 steps right after idle read 5-7 % slower than 200
  # (round 3: driver 5.55e12 with --steps 20 --warmup 5, own 200-step runs
  # 5.9e12).  Windows of 10 steps until the clocks have stopped rising: three
  # windows in a row within 1 % of the fastest seen, not before 100 steps (two
  # agreeing windows -- round 4's rule -- were met 30-40 steps in, with the
  # fused kernel still 5 % off its sustained time: profiles/r05_bench_driver_
  # like.json 1.177 ms against 1.129), at most --clock-warm-seconds; every rank
  # takes the decision from MAX-reduced numbers, so all run the same number of
  # steps (steps exchange halos).
  clock_warm_steps, best_window, stable = 0, None, 0
  warm_begin = time.perf_counter()
  while args.clock_warm_seconds > 0:
    t0 = time.perf_counter()
    for _ in range(10):
      one_step()
    torch.cuda.synchronize()
    now = time.perf_counter()
    pair = [now - t0, now - warm_begin]
    if tdist is not None:
      t = torch.tensor(pair, device=dev, dtype=torch.float64)
      tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
      pair = [float(v) for v in t.tolist()]
    clock_warm_steps += 10
    if best_window is None or pair[0] < 0.99 * best_window:
      best_window, stable = pair[0], 0          # still getting faster
    elif pair[0] <= 1.01 * best_window:
      best_window = min(best_window, pair[0])
      stable += 1
    else:
      stable = 0                                # a slow window: look again
    if (stable >= 3 and clock_warm_steps >= 100) or \
        pair[1] >= args.clock_warm_seconds:
      break

  def restart():
    """Every array of the rotation back to the seeded input (each rank's
    slab of it): a step writes only the valid box of its output, and the next
    step reads the rest of that array too."""
    for i, full in enumerate(seeded_fields()):
      a_bufs[i].copy_(full[slab.begin:slab.end])
      del full
    for bufs in pool[1:]:
      for t, a in zip(bufs, a_bufs):
        t.copy_(a)
    chain['cur'], chain['first'] = a_bufs, True
    if hider is not None:
      hider.invalidate()

  # Then back to the seeded input, and the warm-up steps from there: how many
  # steps the spin above ran depends on the clocks, and what the last timed
  # step computes (the arrays --dump-outputs writes) must depend on the
  # arguments alone.  The speed of a step depends on the field it runs on:
  # timed steps 1 / 6 / 51 steps after the restart ran 3 / 1.5 / 0.9 % slower
  # than after the few hundred steps that used to precede them, hence the
  # settling steps.  The one step after them, untimed, counts the launches of
  # a step and makes the first timed step open with a halo exchange, as every
  # later one does.
  restart()
  settle_steps = -(-SETTLE_ITERATIONS // max(1, args.iterate))
  for _ in range(args.warmup + settle_steps):
    one_step()
  _orig_step = step_fn

  def counting_step(dst, src, lext, iters, **kw):
    nonlocal launches_per_step
    _orig_step(dst, src, lext, iters, **kw)
    launches_per_step += prog.last_launches()[0]

  step_fn_real, step_fn = step_fn, counting_step
  one_step()
  step_fn = step_fn_real
  barrier()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    last = one_step()
  torch.cuda.synchronize()
  barrier()
  torch.cuda.synchronize()
  elapsed = time.perf_counter() - t0
  if tdist is not None:
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    tdist.all_reduce(t, op=tdist.ReduceOp.MAX)
    elapsed = float(t.item())
  transport = ('RCCL send/recv' if backend == 'nccl' else backend +
               ' (REHEARSAL on one GPU, not a measurement)')

  def whole_grid(res):
    """The output arrays of a step as the caller of the whole grid receives
    them: every rank's own rows, gathered on rank 0 (a collective: every rank
    calls it)."""
    own = [r[slab.ghost_lo:slab.ghost_lo + slab.own_rows] for r in res]
    if world > 1:
      most = -(-extent[-1] // world)
      gathered = []
      for t in own:
        pad = torch.zeros((most,) + tuple(t.shape[1:]), dtype=t.dtype,
                          device=dev if backend == 'nccl' else 'cpu')
        pad[:t.shape[0]].copy_(t)
        parts = [torch.empty_like(pad) for _ in range(world)]
        tdist.all_gather(parts, pad)
        rows_of = [extent[-1] // world + (1 if r < extent[-1] % world else 0)
                   for r in range(world)]
        gathered.append(torch.cat([p[:n] for p, n in zip(parts, rows_of)]))
      own = gathered
    return own

  if args.dump_outputs:
    # (before anything else runs on the arrays of the rotation)
    grid = whole_grid(last)
    if rank == 0:
      dump_outputs(args.dump_outputs, stencil, extent, args.iterate, grid)
    del grid

  if args.full:
    # the dominant kernel again, now at the clocks the timed steps ran at (the
    # pre-measurement above starts ~1 ms after idle and reads up to 20 % slow
    # on the VALU-bound fused kernel); this is the number the roofline reports
    kernel_ms_cold = kernel_ms
    kernel_ms = time_events(dominant, stream, calls) / per_call
    torch.cuda.synchronize()
    achieved = alg_bytes / (kernel_ms * 1e-3) / 1e9
    roofline.update({
        'achieved': achieved, 'frac': achieved / HBM_PEAK_GBS,
        'kernel_ms': kernel_ms,
        'kernel_ms_before_timed_region': kernel_ms_cold,
        'effective_GBs_at_8B_per_cell_iter': achieved * fuse,
    })
    if roofline.get('measured_copy_GBs'):
      roofline['frac_of_measured_copy'] = (achieved /
                                           roofline['measured_copy_GBs'])
    # every pass of the step's schedule, timed the same way (the dominant one
    # is the object above)
    scheduled = []
    for depth, count in sorted(sched.items(), reverse=True):
      ms = kernel_ms if depth == fuse else time_pass(depth)
      ps = [p for p in prog.module.sorted_passes() if p.fused_iters == depth]
      name = prog.module.kernels[ps[0].kernels[0]].name if ps else '?'
      key = isa.isa_key(prog.code, name)
      pmc_k, _ = pmc_of(name, key)
      vk = valu_roof(name, ms, (pmc_k or {}).get(
          'valu_wave_instructions_per_launch'))
      scheduled.append({
          'kernel': name, 'isa_key': key,
          'traffic': (pmc_k or {}).get('hbm_bytes_per_launch'),
          'iterations_per_launch': depth,
          'launches_per_exchange_interval': count,
          'kernel_ms': ms,
          'frac': (alg_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                   if ms else None),
          **({'valu_frac': vk['frac_of_valu_issue_peak'],
              'valu_wave_instructions_per_launch':
                  vk['wave_instructions_per_launch']} if vk else {}),
      })
    torch.cuda.synchronize()
    roofline['scheduled_kernels'] = scheduled
    if 'valu' in roofline:
      roofline['valu']['frac_of_valu_issue_peak'] = (
          roofline['valu']['min_issue_ms'] / kernel_ms)
      # which roof the launch is nearer to.  `achieved` / `peak` / `frac`
      # stay the HBM figures of the contract (algorithmic bytes / duration); a
      # fused kernel that sits nearer its VALU-issue roof says so here
      if roofline['valu']['frac_of_valu_issue_peak'] > roofline['frac']:
        roofline['bound'] = 'valu'
        roofline['bound_frac'] = roofline['valu']['frac_of_valu_issue_peak']
        roofline['bound_note'] = (
            'VALU issue: %.3g wave-instructions per launch need %.1f us at '
            'peak issue; `frac` is the HBM fraction of the same launch' %
            (roofline['valu']['wave_instructions_per_launch'],
             roofline['valu']['min_issue_ms'] * 1e3))

  cells = 1
  for e in extent:
    cells *= e
  value = cells * args.iterate * args.steps / elapsed

  result = {
      'metric': 'stencil cells*iters/s, %s %s iterate=%d' %
                (stencil.app_name, 'x'.join(map(str, extent)), args.iterate),
      'value': value, 'unit': 'cells*iters/s', 'n_gpus': world,
      'rccl_world': rccl_world,
      **({'emulated_n_gpus': emulate} if emulate > 1 else {}),
      'steps': args.steps, 'warmup': args.warmup,
      'clock_warm_steps': clock_warm_steps, 'settle_steps': settle_steps,
      'ms_per_step': elapsed / args.steps * 1e3, 'higher_is_better': True,
      'scaling': args.scaling, 'vs_baseline': None, 'dtype': 'f32',
      'data': 'synthetic',
      'config': {
          'workload': '%s %s %s iterate=%d' %
                      (stencil.app_name,
                       str(table[stencil.input_names[0]]),
                       'x'.join(map(str, extent)), args.iterate),
          'kernel_family': passes[0].kind if passes else '?',
          'fused_iterations_per_launch': fuse,
          'decomposition': ('slabs along dim %d, %d ghost rows per side, '
                            '%d halo exchange(s) per step' %
                            (stencil.dim - 1, slab.ghost_hi or slab.ghost_lo,
                             sdist.rounds(args.iterate, ex)))
                           if world > 1 else 'none',
          # steps are chained (each starts from the previous step's output),
          # so on N > 1 GPUs every step opens with a halo exchange
          'exchanges_per_step': sdist.rounds(args.iterate, ex)
                                if world > 1 else 0,
          'overlap': bool(mode['overlap']),
          **({'overlap_trial': overlap_trial} if overlap_trial else {}),
          'transport': transport + ' (torch.distributed, one rank per GPU)'
                       if world > 1 else 'none',
          'ghost_rows_per_side': (slab.ghost_hi or slab.ghost_lo)
                                 if geo_world > 1 else 0,
          'ghost_row_fraction': (slab.rows - slab.own_rows) / float(slab.rows),
          'launches_per_step': launches_per_step,
          'passes': [p.fused_iters for p in prog.module.sorted_passes()],
          'schedule_per_exchange_interval': {
              str(t): c for t, c in prog.schedule(
                  local_extent, min(ex, args.iterate)).items()},
          'pass_us_measured': {str(t): round(v, 1) for t, v in
                               prog.pass_times(local_extent)[0].items()},
      },
      **({'roofline': roofline} if roofline else {}),
  }

  # ---- result check (outside the timed region; --full) -----------------------
  # The reference's generated host checks every run it times, in the same
  # process (frt/host.py:545-553 run, :625-657 compare).  Here: ONE more step
  # -- the same programs, schedule, exchange mode and code path as the timed
  # ones -- from the seeded input, the ranks' own rows gathered on rank 0 and
  # compared with the CPU oracle (test infrastructure, used as the checker
  # only) on the valid box, bit for bit.
  if args.full and not args.no_parity and emulate <= 1:
    host_in = {}
    for i, (name, full) in enumerate(zip(stencil.input_names,
                                         seeded_fields())):
      a_bufs[i].copy_(full[slab.begin:slab.end])
      if rank == 0:
        host_in[name] = full.cpu().numpy().view(
            stencil.input_types[i].np_name)
      del full
    chain['cur'], chain['first'] = a_bufs, True
    if hider is not None:
      hider.invalidate()
    # N > 1: TWO chained steps -- the first starts on fresh ghosts (with one
    # interval per step it exchanges nothing), the second opens with the halo
    # exchange the timed steps open with
    checked_steps = 2 if world > 1 else 1
    for _ in range(checked_steps):
      res = one_step()
    torch.cuda.synchronize()
    own = whole_grid(res)
    if rank == 0:
      import numpy as np
      from oracle import c_oracle
      t0 = time.time()
      want = c_oracle.COracle(stencil, openmp=True).run(
          host_in, iterate=checked_steps * args.iterate)
      cells_checked = bad = 0
      for t, o in zip(own, stencil.output_names):
        got = t.cpu().numpy().view(want[o].dtype)
        lo, hi = stencil.valid_box(extent, o, checked_steps * args.iterate)
        idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
        g, w = got[idx], want[o][idx]
        if g.dtype.kind == 'f':
          bits = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
          g = np.ascontiguousarray(g).view(bits)
          w = np.ascontiguousarray(w).view(bits)
        cells_checked += int(g.size)
        bad += int((g != w).sum())
      result['parity'] = {
          'cells': cells_checked, 'mismatches': bad,
          'against': 'oracle/c_oracle.py (OpenMP), %d iterations from the '
                     'seeded input, valid box, bit for bit; %.1f s' %
                     (checked_steps * args.iterate, time.time() - t0),
          'what_ran': '%d more chained step(s) after the timed region: same '
                      'program, schedule and exchange mode' % checked_steps,
      }
      del want, host_in

  if args.full and world == 1 and rank == 0:
    if not args.no_single_iter and fuse > 1:
      prog1 = runtime.Program(stencil, options([1]), device=local_rank,
                              extent=local_extent)

      def single():
        prog1.run_device([t.data_ptr() for t in b_bufs],
                         [t.data_ptr() for t in a_bufs], local_extent,
                         iterate=args.iterate, stream=stream)

      single()
      torch.cuda.synchronize()
      ms = time_events(single, stream, 3)
      k1 = alg_bytes / (ms / args.iterate * 1e-3) / 1e9
      result['single_iter'] = {
          'value': cells * args.iterate / (ms * 1e-3),
          'unit': 'cells*iters/s', 'ms_per_step': ms,
          'kernel': prog1.module.kernels[0].name,
          'kernel_key': runtime.source_key(prog1.module.source),
          'isa_key': isa.isa_key(prog1.code, prog1.module.kernels[0].name),
          'roofline': {'bound': 'hbm', 'achieved': k1, 'peak': HBM_PEAK_GBS,
                       'unit': 'GB/s', 'frac': k1 / HBM_PEAK_GBS,
                       'frac_of_measured_copy':
                           k1 / roofline['measured_copy_GBs']
                           if roofline.get('measured_copy_GBs') else None},
      }
      prog1.close()
    if not args.no_other_configs and emulate <= 1:
      result['other_configs'] = other_configs(stream)
    if not args.no_rehearsal and emulate <= 1:
      result['rehearsed_scaling'] = rehearse(args, stencil, extent, fuses,
                                             options, stream, value)
    if not args.no_cpu_baseline:
      result['cpu_baseline'] = cpu_baseline(stencil, extent, args.cpu_seconds)

  if rank == 0:
    print(json.dumps(result))
  if tdist is not None:
    tdist.destroy_process_group()
  if rank == 0 and result.get('parity', {}).get('mismatches'):
    sys.stderr.write('bench.py: the checked step differs from the oracle in '
                     '%d cells\n' % result['parity']['mismatches'])
    sys.exit(3)


if __name__ == '__main__':
  main()
