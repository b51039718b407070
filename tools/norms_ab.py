#!/usr/bin/env python3
"""Sustained A/B of the exact norms (soda_hip_run_device_norms)
against the residual taken by the generic path, in ONE process, the arms
alternating in sub-blocks (as tools/ab.py and tools/residual_ab.py: clock
drift then shows instead of deciding):

  arm a  soda_hip_run_device_residual with SODA_HIP_RESIDUAL_GENERIC=1 -- the
         yardstick: iterate - 1 iterations scheduled, the one-iteration pass,
         then `<app>_residual`;
  arm b  soda_hip_run_device_norms: the same passes, then soda_norms_zero and
         the norms kernel;
  arm k  the norms kernels alone (zero + accumulate) on the arrays arm b left:
         the deltas of a real last iteration;
  arm s  the norms kernels alone on arrays of the same extent whose deltas
         alternate between 2^100 and 2^-100: no two neighbours of a lane share
         a window, every cell takes the slow path through LDS.

  here (hiprtc, no GPU):  python tools/norms_ab.py --compile-only
  on the box:             python tools/norms_ab.py --out profiles/norms_ab.json

One JSON object: per case and arm the microseconds per run of every
sub-block, their median, minimum and maximum, b - a, and the registers of the
norms kernels."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, extent, fuse, runs per sub-block)
CASES = [
    ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 2),
    ('heat3d.soda', 48, (512, 512, 512), (2,), 2),
]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3,
                  help='sub-blocks per arm per round')
  ap.add_argument('--only', type=int, nargs='*', help='indices into CASES')
  ap.add_argument('--out', help='also write the JSON object to this file')
  ap.add_argument('--compile-only', action='store_true')
  args = ap.parse_args()
  from soda_amd import core, runtime
  from soda_amd.codegen.hip import lower
  out = {'tool': 'tools/norms_ab.py', 'unit': 'us per run (all iterations; '
         'arms k and s: the norms kernels alone)',
         'rounds': args.rounds, 'blocks': args.blocks, 'cases': []}
  if not args.compile_only:
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream().cuda_stream
    out['gpu'] = torch.cuda.get_device_name(0)
  for at, (name, iterate, extent, fuse, runs) in enumerate(CASES):
    if args.only and at not in args.only:
      continue
    st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                        iterate=iterate)
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'fuse': list(fuse), 'runs_per_block': runs, 'arms': {}}
    out['cases'].append(rec)
    _, res = runtime.norms_resources('float', st.dim)
    rec['registers'] = {k: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch',
                                              'code')}
                        for k, v in sorted(res.items())}
    if args.compile_only:
      opts = runtime.resolve_options(
          st, lower.LowerOptions(fuse=fuse, residual=True), extent)
      mod = lower.lower(st, opts)
      runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      continue
    shape = tuple(extent[::-1])
    a_in = torch.rand(shape, device=dev, dtype=torch.float32)
    a_out = torch.empty_like(a_in)
    struct = torch.zeros(4, device=dev, dtype=torch.int64)
    acc = torch.zeros(105, device=dev, dtype=torch.int64)
    prog = runtime.Program(st, lower.LowerOptions(fuse=fuse, residual=True),
                           extent=extent)
    nm = prog.norms()
    o, i = [a_out.data_ptr()], [a_in.data_ptr()]
    # arm s: |cur - prev| alternates between 2^100 and 2^-100 along a row
    s_cur = torch.empty(shape, device=dev, dtype=torch.float32)
    s_cur.view(-1)[0::2] = 2.0 ** 100
    s_cur.view(-1)[1::2] = 2.0 ** -100
    s_prev = torch.zeros_like(s_cur)
    lo, hi = prog.residual_box(extent, iterate)[0]

    def run_a():
      os.environ['SODA_HIP_RESIDUAL_GENERIC'] = '1'
      prog.run_device(o, i, extent, iterate, stream=stream,
                      residual=struct.data_ptr())
      os.environ.pop('SODA_HIP_RESIDUAL_GENERIC', None)

    def run_b():
      prog.run_device(o, i, extent, iterate, stream=stream,
                      norms=acc.data_ptr())

    def run_k():
      nm.zero(acc.data_ptr(), stream=stream)
      nm.accumulate(a_out.data_ptr(), a_in.data_ptr(), extent, lo, hi,
                    acc.data_ptr(), stream=stream)

    def run_s():
      nm.zero(acc.data_ptr(), stream=stream)
      nm.accumulate(s_cur.data_ptr(), s_prev.data_ptr(), extent, lo, hi,
                    acc.data_ptr(), stream=stream)

    arms = (('a', run_a), ('b', run_b), ('k', run_k), ('s', run_s))
    for arm, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {'us_per_run_by_block': []}
      if arm in 'ab':
        rec['arms'][arm]['launches'] = prog.last_launches()[0]
        rec['arms'][arm]['residual'] = list(prog.last_residual())
      if arm != 'a':
        got = nm.fetch(acc.data_ptr(), stream=stream)
        rec['arms'][arm]['struct'] = {
            'count': int(got.count), 'unordered': int(got.unordered),
            'infinite': int(got.infinite),
            'l1': runtime.norms_value(got, 'l1'),
            'l2_squared': runtime.norms_value(got, 'l2')}
    for _ in range(args.rounds):
      rows = {arm: [] for arm, _ in arms}
      for _ in range(args.blocks):
        for arm, run in arms:
          a, b = runtime.Event(), runtime.Event()
          a.record(stream)
          for _ in range(runs):
            run()
          b.record(stream)
          torch.cuda.synchronize()
          rows[arm].append(round(a.elapsed_ms(b) * 1000 / runs, 1))
      for arm, row in rows.items():
        rec['arms'][arm]['us_per_run_by_block'].append(row)
    for arm in rec['arms'].values():
      flat = [x for row in arm['us_per_run_by_block'] for x in row]
      arm['median_us'] = round(statistics.median(flat), 1)
      arm['min_us'], arm['max_us'] = min(flat), max(flat)
    med = {k: v['median_us'] for k, v in rec['arms'].items()}
    rec['b_minus_a_us'] = round(med['b'] - med['a'], 1)
    rec['a_spread_us'] = round(rec['arms']['a']['max_us'] -
                               rec['arms']['a']['min_us'], 1)
    cells = 1
    for l, h in zip(lo, hi):
      cells *= h - l
    rec['cells_counted'] = cells
    rec['k_bytes_per_ns'] = round(2 * 4 * cells / (med['k'] * 1e3), 1)
    prog.close()
    del a_in, a_out, s_cur, s_prev
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
