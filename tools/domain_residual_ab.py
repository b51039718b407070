#!/usr/bin/env python3
"""Sustained A/B of the residual and the norms on periodic and bordered domains
(soda_hip_*_run_padded_residual / _norms) against the plain
padded run, ONE program at its usual fusion depth, in ONE process, the arms
alternating in sub-blocks (as tools/ab.py and tools/border_fused_ab.py: clock
drift then shows instead of deciding).  Per case three domains -- the torus,
`clamp` walls at depth 1, `clamp` walls at depth 0 (the deepest pass) -- and
per domain three arms:

  arm a    <handle>_run_padded;
  arm r    <handle>_run_padded_residual;
  arm n    <handle>_run_padded_norms.

  here (hiprtc, no GPU):  python tools/domain_residual_ab.py --compile-only
  on the box:             python tools/domain_residual_ab.py \\
                              --out profiles/domain_residual_ab.json

One JSON object: per case, domain and arm the microseconds per run of every
sub-block, their median, minimum and maximum; r - a and n - a by the medians,
and how the residual was taken (twin or generic, depth of the last pass)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, domain, fuse, runs per sub-block)
CASES = [
    ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 2),
    ('heat3d.soda', 48, (512, 512, 512), (2,), 2),
]
MODE = 'clamp'
DOMAINS = ('torus', 'walls_depth1', 'walls_fused')


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
  out = {'tool': 'tools/domain_residual_ab.py', 'mode': MODE,
         'unit': 'us per run of all iterations',
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
    depth = max(fuse)
    lo, hi = runtime.periodic_ghosts(st, depth)
    torus = [l + n + h for l, n, h in zip(lo, extent, hi)]
    torus[0] = -(-torus[0] // vec) * vec
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'fuse': list(fuse), 'runs_per_block': runs, 'domains': {}}
    out['cases'].append(rec)
    opts = runtime.resolve_options(
        st, lower.LowerOptions(fuse=fuse, residual=True), torus)
    if args.compile_only:
      mod = lower.lower(st, opts)
      runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      runtime.wrap_resources(4, st.dim)
      runtime.extend_resources(4, st.dim)
      runtime.box_resources(4, st.dim)
      runtime.norms_resources('float', st.dim)
      continue
    prog = runtime.Program(st, opts, extent=torus)
    res = torch.zeros(4, device=dev, dtype=torch.int64)
    acc = torch.zeros(ctypes.sizeof(runtime.NormsStruct) // 8, device=dev,
                      dtype=torch.int64)
    handles = {'torus': prog.periodic(extent, depth),
               'walls_depth1': prog.bordered(extent, MODE),
               'walls_fused': prog.bordered(extent, MODE, depth=0)}
    for dom in DOMAINS:
      h = handles[dom]
      info = h.info()
      p_in = torch.rand(tuple(info['padded'][::-1]), device=dev,
                        dtype=torch.float32)
      p_out = torch.empty_like(p_in)
      if dom == 'walls_fused':           # (no fill entry: depth 1's frame)
        assert info['padded'] == handles['walls_depth1'].info()['padded']
        handles['walls_depth1'].fill([p_in.data_ptr()], stream=stream)
      else:
        h.fill([p_in.data_ptr()], stream=stream)
      po, pi = [p_out.data_ptr()], [p_in.data_ptr()]
      drec = {'padded': list(info['padded']),
              'depth': info.get('depth', info['refill_every']), 'arms': {}}
      rec['domains'][dom] = drec
      arms = [('a', lambda: h.run_padded(po, pi, iterate, stream=stream)),
              ('r', lambda: h.run_padded(po, pi, iterate, stream=stream,
                                         residual=res.data_ptr())),
              ('n', lambda: h.run_padded(po, pi, iterate, stream=stream,
                                         norms=acc.data_ptr()))]
      for arm, run in arms:
        run()                             # calibrates, allocates the scratch
        torch.cuda.synchronize()
        drec['arms'][arm] = {'us_per_run_by_block': []}
        if arm == 'r':
          drec['residual_taken'] = list(prog.last_residual())
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
          drec['arms'][arm]['us_per_run_by_block'].append(row)
      for arm in drec['arms'].values():
        flat = [x for row in arm['us_per_run_by_block'] for x in row]
        arm['median_us'] = round(statistics.median(flat), 1)
        arm['min_us'], arm['max_us'] = min(flat), max(flat)
      med = {q: v['median_us'] for q, v in drec['arms'].items()}
      drec['r_minus_a_us'] = round(med['r'] - med['a'], 1)
      drec['n_minus_a_us'] = round(med['n'] - med['a'], 1)
      del p_in, p_out
    for h in handles.values():
      h.close()
    prog.close()
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
