#!/usr/bin/env python3
"""Sustained A/B of a bordered run (soda_hip_border_*), every
dimension `clamp`, against the same launches without fills and against the
torus, in ONE process, the arms alternating in sub-blocks (as tools/ab.py and
tools/periodic_ab.py: clock drift then shows instead of deciding):

  arm a  soda_hip_run_device on the padded extent, fuse=(1,), same `iterate`
         -- the yardstick: the launches arm b makes, without the fills;
  arm b  soda_hip_border_run_padded: one iteration, one fill, `iterate` times;
  arm c  soda_hip_border_run_device: pad, the loop of arm b, crop;
  arm k  the fill kernel alone on one padded array;
  arm p  soda_hip_periodic_run_padded of the program at its usual fusion depth
         on the same grid -- what giving up fusion costs.

  here (hiprtc, no GPU):  python tools/border_ab.py --compile-only
  on the box:             python tools/border_ab.py --out profiles/border_ab.json

One JSON object: per case and arm the microseconds per run of every sub-block,
their median, minimum and maximum, b - a against iterate x k and against a's
own spread, c - b, b / p, and the registers of the extend kernel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, domain, the torus's fuse, runs per sub-block)
CASES = [
    ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 2),
    ('heat3d.soda', 48, (512, 512, 512), (2,), 2),
]
MODE = 'clamp'


def _padded(st, lo, hi, extent, vec):
  padded = [l + n + h for l, n, h in zip(lo, extent, hi)]
  padded[0] = -(-padded[0] // vec) * vec
  return padded


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
  out = {'tool': 'tools/border_ab.py', 'mode': MODE,
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
    vec = lower.default_vec(st)
    # the bordered domain: the frame of one iteration; the torus: of max(fuse)
    padded = _padded(st, *runtime.border_ghosts(st, MODE), extent, vec)
    torus = _padded(st, *runtime.periodic_ghosts(st, max(fuse)), extent, vec)
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'padded': padded, 'torus_padded': torus, 'torus_fuse': list(fuse),
           'runs_per_block': runs, 'arms': {}}
    out['cases'].append(rec)
    _, res = runtime.extend_resources(4, st.dim)
    rec['registers'] = {q: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch',
                                              'code')}
                        for q, v in sorted(res.items())}
    if args.compile_only:
      for f, ext in (((1,), padded), (fuse, torus)):
        opts = runtime.resolve_options(st, lower.LowerOptions(fuse=f), ext)
        mod = lower.lower(st, opts)
        runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      runtime.wrap_resources(4, st.dim)
      continue
    p_in = torch.rand(tuple(padded[::-1]), device=dev, dtype=torch.float32)
    p_out = torch.empty_like(p_in)
    t_in = torch.rand(tuple(torus[::-1]), device=dev, dtype=torch.float32)
    t_out = torch.empty_like(t_in)
    d_in = torch.rand(tuple(extent[::-1]), device=dev, dtype=torch.float32)
    d_out = torch.empty_like(d_in)
    prog = runtime.Program(st, lower.LowerOptions(fuse=(1,)), extent=padded)
    deep = runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=torus)
    bor = prog.bordered(extent, MODE)
    per = deep.periodic(extent, max(fuse))
    info = bor.info()
    assert list(info['padded']) == padded and info['refill_every'] == 1, info
    assert list(per.info()['padded']) == torus, per.info()
    rec['scratch_bytes'] = info['scratch_bytes']
    bor.fill([p_in.data_ptr()], stream=stream)     # arm b's inputs: extended
    per.fill([t_in.data_ptr()], stream=stream)     # arm p's: wrapped
    po, pi = [p_out.data_ptr()], [p_in.data_ptr()]
    to, ti = [t_out.data_ptr()], [t_in.data_ptr()]
    do, di = [d_out.data_ptr()], [d_in.data_ptr()]

    def run_a():
      prog.run_device(po, pi, padded, iterate, stream=stream)

    def run_b():
      bor.run_padded(po, pi, iterate, stream=stream)

    def run_c():
      bor.run_device(do, di, iterate, stream=stream)

    def run_k():
      bor.fill(po, stream=stream)

    def run_p():
      per.run_padded(to, ti, iterate, stream=stream)

    arms = (('a', run_a), ('b', run_b), ('c', run_c), ('k', run_k),
            ('p', run_p))
    for arm, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {'us_per_run_by_block': []}
    rec['schedule'] = {str(q): v for q, v in
                       prog.schedule(padded, iterate).items()}
    rec['chunk_schedule'] = {str(q): v for q, v in
                             prog.schedule(padded, 1).items()}
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
    rec['fills'] = iterate
    rec['b_minus_a_us'] = round(med['b'] - med['a'], 1)
    rec['a_spread_us'] = round(rec['arms']['a']['max_us'] -
                               rec['arms']['a']['min_us'], 1)
    rec['fills_times_k_us'] = round(iterate * med['k'], 1)
    rec['c_minus_b_us'] = round(med['c'] - med['b'], 1)
    rec['b_over_p'] = round(med['b'] / med['p'], 3)
    bor.close()
    per.close()
    prog.close()
    deep.close()
    del p_in, p_out, t_in, t_out, d_in, d_out
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
