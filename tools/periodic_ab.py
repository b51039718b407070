#!/usr/bin/env python3
"""Sustained A/B of a run on a torus (soda_hip_periodic_*)
against the same program on the open box of the PADDED extent, in ONE process,
the arms alternating in sub-blocks (as tools/ab.py and tools/norms_ab.py:
clock drift then shows instead of deciding):

  arm a  soda_hip_run_device on the padded extent, same `iterate` and `fuse`
         -- the yardstick: the kernels arm b launches, without the refills;
  arm b  soda_hip_periodic_run_padded: chunks of k iterations, a fill behind
         each;
  arm c  soda_hip_periodic_run_device: pad, the loop of arm b, crop;
  arm k  the fill kernel alone on one padded array.

  here (hiprtc, no GPU):  python tools/periodic_ab.py --compile-only
  on the box:             python tools/periodic_ab.py --out profiles/periodic_ab.json

One JSON object: per case and arm the microseconds per run of every
sub-block, their median, minimum and maximum, b - a against a's own spread,
c - b, and the registers of the wrap kernel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, torus, fuse, runs per sub-block)
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
  out = {'tool': 'tools/periodic_ab.py',
         'unit': 'us per run (all iterations; arm k: one fill)',
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
    # the padded extent the program is built for: the frame of the deepest
    # fusion depth, the row rounded to the vector width
    k = max(fuse)
    lo, hi = runtime.periodic_ghosts(st, k)
    vec = lower.default_vec(st)
    padded = [l + n + h for l, n, h in zip(lo, extent, hi)]
    padded[0] = -(-padded[0] // vec) * vec
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'padded': padded, 'fuse': list(fuse), 'refill_every': k,
           'runs_per_block': runs, 'arms': {}}
    out['cases'].append(rec)
    _, res = runtime.wrap_resources(4, st.dim)
    rec['registers'] = {q: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch',
                                              'code')}
                        for q, v in sorted(res.items())}
    cells, torus = 1, 1
    for p, n in zip(padded, extent):
      cells, torus = cells * p, torus * n
    rec['ghost_fraction'] = round(1 - torus / cells, 5)
    if args.compile_only:
      opts = runtime.resolve_options(st, lower.LowerOptions(fuse=fuse), padded)
      mod = lower.lower(st, opts)
      runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      continue
    p_in = torch.rand(tuple(padded[::-1]), device=dev, dtype=torch.float32)
    p_out = torch.empty_like(p_in)
    d_in = torch.rand(tuple(extent[::-1]), device=dev, dtype=torch.float32)
    d_out = torch.empty_like(d_in)
    prog = runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=padded)
    per = prog.periodic(extent, k)
    info = per.info()
    assert list(info['padded']) == padded, (info, padded)
    rec['scratch_bytes'] = info['scratch_bytes']
    per.fill([p_in.data_ptr()], stream=stream)       # arm b's inputs: wrapped
    po, pi = [p_out.data_ptr()], [p_in.data_ptr()]
    do, di = [d_out.data_ptr()], [d_in.data_ptr()]

    def run_a():
      prog.run_device(po, pi, padded, iterate, stream=stream)

    def run_b():
      per.run_padded(po, pi, iterate, stream=stream)

    def run_c():
      per.run_device(do, di, iterate, stream=stream)

    def run_k():
      per.fill(po, stream=stream)

    arms = (('a', run_a), ('b', run_b), ('c', run_c), ('k', run_k))
    for arm, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {'us_per_run_by_block': []}
    rec['schedule'] = {str(q): v for q, v in
                       prog.schedule(padded, iterate).items()}
    rec['chunk_schedule'] = {str(q): v for q, v in
                             prog.schedule(padded, k).items()}
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
    med = {q: v['median_us'] for q, v in rec['arms'].items()}
    rec['refills'] = -(-iterate // k)
    rec['b_minus_a_us'] = round(med['b'] - med['a'], 1)
    rec['a_spread_us'] = round(rec['arms']['a']['max_us'] -
                               rec['arms']['a']['min_us'], 1)
    rec['c_minus_b_us'] = round(med['c'] - med['b'], 1)
    rec['refills_times_k_us'] = round(rec['refills'] * med['k'], 1)
    per.close()
    prog.close()
    del p_in, p_out, d_in, d_out
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
