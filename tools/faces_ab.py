#!/usr/bin/env python3
"""Sustained A/B of the faces fill (soda_rt_faces.h) against
the extend fill it restates, on ONE symmetric request -- every dimension
`clamp` --, in ONE process, the arms alternating in sub-blocks (as tools/ab.py
and tools/border_fused_ab.py: clock drift then shows instead of deciding):

  arm a   the handle of soda_hip_border_create / _fused_create: the extend
          kernels fill the frame -- what a symmetric request always takes;
  arm b   the same request through the `_faces` twin with
          SODA_HIP_FACES_FORCE=1 set while the handle is made: the faces
          kernels fill the frame, with the selects an asymmetric request pays.

  here (hiprtc, no GPU):  python tools/faces_ab.py --compile-only
  on the box:             python tools/faces_ab.py --out profiles/faces_ab.json

One JSON object: per case and arm the microseconds per run of every sub-block,
their median, minimum and maximum; b / a, and whether b's median lies inside
a's own min-max spread."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, domain, fuse, depth of the handle, runs per sub-block)
CASES = [
    ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 1, 2),
    ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 13, 2),
    ('heat3d.soda', 48, (512, 512, 512), (2,), 1, 2),
]
MODE = 'clamp'
SWITCH = 'SODA_HIP_FACES_FORCE'


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
  os.environ.pop(SWITCH, None)
  out = {'tool': 'tools/faces_ab.py', 'mode': MODE,
         'unit': 'us per run of all iterations',
         'rounds': args.rounds, 'blocks': args.blocks, 'cases': []}
  if not args.compile_only:
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream().cuda_stream
    out['gpu'] = torch.cuda.get_device_name(0)
  for at, (name, iterate, extent, fuse, depth, runs) in enumerate(CASES):
    if args.only and at not in args.only:
      continue
    st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                        iterate=iterate)
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'fuse': list(fuse), 'depth': depth, 'runs_per_block': runs,
           'arms': {}}
    out['cases'].append(rec)
    rec['registers'] = {}
    for resources in (runtime.extend_resources, runtime.faces_resources):
      _, res = resources(4, st.dim)
      rec['registers'].update({
          q: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch', 'code')}
          for q, v in sorted(res.items())})
    _, _, lo, hi = runtime.border_fused_ghosts(st, MODE, depth)
    vec = lower.default_vec(st)
    padded = [l + n + h for l, n, h in zip(lo, extent, hi)]
    padded[0] = -(-padded[0] // vec) * vec
    opts = runtime.resolve_options(st, lower.LowerOptions(fuse=fuse), padded)
    if args.compile_only:
      mod = lower.lower(st, opts)
      runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      runtime.box_resources(4, st.dim)
      continue
    prog = runtime.Program(st, opts, extent=padded)
    arm_a = prog.bordered(extent, MODE, depth=depth)
    os.environ[SWITCH] = '1'
    try:
      arm_b = prog.bordered(extent, MODE, depth=depth)
    finally:
      os.environ.pop(SWITCH, None)
    info = arm_a.info()
    assert arm_b.info() == info and list(info['padded']) == padded, info
    p_in = torch.rand(tuple(padded[::-1]), device=dev, dtype=torch.float32)
    outs = {q: torch.empty_like(p_in) for q in 'ab'}
    if depth == 1:
      arm_a.fill([p_in.data_ptr()], stream=stream)     # the inputs: extended
    else:
      with prog.bordered(extent, MODE) as plain:
        plain.fill([p_in.data_ptr()], stream=stream)
    arms = [(q, (lambda h, o: lambda: h.run_padded(
        [o.data_ptr()], [p_in.data_ptr()], iterate, stream=stream))(
            h, outs[q])) for q, h in (('a', arm_a), ('b', arm_b))]
    for arm, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {'us_per_run_by_block': []}
    rec['same_bits'] = bool(torch.equal(outs['a'].view(torch.int32),
                                        outs['b'].view(torch.int32)))
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
    a, b = rec['arms']['a'], rec['arms']['b']
    rec['b_over_a'] = round(b['median_us'] / a['median_us'], 4)
    rec['b_median_inside_a_range'] = \
        a['min_us'] <= b['median_us'] <= a['max_us']
    for handle in (arm_a, arm_b):
      handle.close()
    prog.close()
    del p_in, outs
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
