#!/usr/bin/env python3
"""Sustained A/B of batched runs (LowerOptions.batch,
soda_hip_run_device_batch) against what a caller did before them, in ONE
process, the two arms alternating in sub-blocks (as tools/ab.py: clock drift
then shows instead of deciding):

  arm A  an unbatched Program and a loop of N run_device calls, one per item,
         on one stream;
  arm B  a batched Program and one run_device(batch=N) call.

Both programs are built for the extent and calibrate by themselves on their
first run, as a caller's would.  The last case is the guard: one 8192^2 grid,
batched program against unbatched -- the same work in the same launches, so the
two arms should not differ by more than their own spread.

  here (hiprtc, no GPU):  python tools/batch_ab.py --compile-only
  on the box:             python tools/batch_ab.py --out profiles/batch_ab.json

One JSON object: per case and arm the microseconds per JOB (all N items, all
iterations) of every sub-block, their median, minimum and maximum, the
schedule and the chunk lengths the library chose."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, items, extent, jobs per sub-block)
CASES = [
    ('jacobi2d.soda', 100, 64, (512, 512), 4),
    ('jacobi2d.soda', 100, 16, (1024, 1024), 4),
    ('jacobi2d.soda', 100, 8, (1920, 1080), 4),
    ('blur.soda', None, 32, (1920, 1080), 20),
    ('heat3d.soda', 50, 8, (128, 128, 128), 4),
    ('jacobi2d.soda', 100, 1, (8192, 8192), 4),      # guard
]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=4,
                  help='sub-blocks per arm per round')
  ap.add_argument('--only', type=int, nargs='*', help='indices into CASES')
  ap.add_argument('--out', help='also write the JSON object to this file')
  ap.add_argument('--compile-only', action='store_true')
  args = ap.parse_args()
  from soda_amd import core, runtime
  from soda_amd.codegen.hip import lower
  out = {'tool': 'tools/batch_ab.py', 'unit': 'us per job (all items, all '
         'iterations)', 'rounds': args.rounds, 'blocks': args.blocks,
         'cases': []}
  if not args.compile_only:
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream().cuda_stream
    out['gpu'] = torch.cuda.get_device_name(0)
    tdt = {'float32': torch.float32, 'float64': torch.float64,
           'uint16': torch.int16, 'int16': torch.int16, 'int32': torch.int32,
           'uint8': torch.uint8, 'int8': torch.int8}
  for at, (name, iterate, items, extent, jobs) in enumerate(CASES):
    if args.only and at not in args.only:
      continue
    st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                        **({'iterate': iterate} if iterate else {}))
    fuse = lower.DEFAULT_FUSE if st.iterate > 1 else ()
    rec = {'program': st.app_name, 'iterate': st.iterate, 'items': items,
           'extent': list(extent), 'jobs_per_block': jobs,
           'launches_per_job': {}, 'arms': {}}
    out['cases'].append(rec)
    if args.compile_only:
      for arm, batch in (('A', False), ('B', True)):
        opts = runtime.resolve_options(
            st, lower.LowerOptions(fuse=fuse, batch=batch), extent)
        mod = lower.lower(st, opts)
        res = runtime.kernel_resources(
            runtime.compile_source(mod.source, '%s.hip' % st.app_name))
        plan = runtime.make_plan(mod, res)
        n = items if batch else 1
        tiles, ns = runtime.plan_geometry_batch(plan, extent, n)
        depths = [p.fused_iters for p in mod.sorted_passes()]
        rec['arms'][arm] = {
            'kernels': {k.name: res.get(k.name) for k in mod.kernels},
            'tiles': {k.name: list(t[:st.dim])
                      for k, t in zip(mod.kernels, tiles)},
            'model_us_per_pass': {str(t): round(v / 1e3, 1)
                                  for t, v in zip(depths, ns)},
            'schedule': {str(t): c for t, c in zip(
                depths, runtime.plan_schedule_batch(plan, extent, n,
                                                    st.iterate)) if c}}
      continue
    shape = (items,) + tuple(extent[::-1])

    def field(t, rand):
      dt = tdt[t.np_name]
      if not rand:
        return torch.empty(shape, device=dev, dtype=dt)
      if dt.is_floating_point:
        return torch.rand(shape, device=dev, dtype=dt)
      return torch.randint(0, 100, shape, device=dev, dtype=dt)

    ins = [field(t, True) for t in st.input_types]
    outs = [field(t, False) for t in st.output_types]
    step_in = [t[0].numel() * t.element_size() for t in ins]
    step_out = [t[0].numel() * t.element_size() for t in outs]
    prog_a = runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=extent)
    prog_b = runtime.Program(st, lower.LowerOptions(fuse=fuse, batch=True),
                             extent=extent)
    each = [([t.data_ptr() + i * s for t, s in zip(outs, step_out)],
             [t.data_ptr() + i * s for t, s in zip(ins, step_in)])
            for i in range(items)]
    whole = ([t.data_ptr() for t in outs], [t.data_ptr() for t in ins])

    def job_a():
      for o, i in each:
        prog_a.run_device(o, i, extent, stream=stream)

    def job_b():
      prog_b.run_device(whole[0], whole[1], extent, stream=stream, batch=items)

    arms = (('A', prog_a, job_a, 1), ('B', prog_b, job_b, items))
    for arm, prog, job, n in arms:
      job()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['launches_per_job'][arm] = prog.last_launches()[0] * (
          items if arm == 'A' else 1)
      rec['arms'][arm] = {
          'kernels': [k.name for k in prog.module.kernels],
          'schedule': {str(t): c for t, c in
                       prog.schedule(extent, st.iterate, n).items()},
          'tiles': {k: list(v) for k, v in prog.geometry(extent, n)[0].items()},
          'us_per_job_by_block': []}
    for _ in range(args.rounds):
      rows = {arm: [] for arm, _, _, _ in arms}
      for _ in range(args.blocks):
        for arm, _, job, _ in arms:
          a, b = runtime.Event(), runtime.Event()
          a.record(stream)
          for _ in range(jobs):
            job()
          b.record(stream)
          torch.cuda.synchronize()
          rows[arm].append(round(a.elapsed_ms(b) * 1000 / jobs, 1))
      for arm, row in rows.items():
        rec['arms'][arm]['us_per_job_by_block'].append(row)
    for arm in rec['arms'].values():
      flat = [x for r in arm['us_per_job_by_block'] for x in r]
      arm['median_us'] = round(statistics.median(flat), 1)
      arm['min_us'], arm['max_us'] = min(flat), max(flat)
    a, b = rec['arms']['A'], rec['arms']['B']
    rec['b_over_a'] = round(b['median_us'] / a['median_us'], 3)
    rec['a_spread_us'] = round(a['max_us'] - a['min_us'], 1)
    rec['a_minus_b_us'] = round(a['median_us'] - b['median_us'], 1)
    prog_a.close()
    prog_b.close()
    del ins, outs
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
