#!/usr/bin/env python3
"""Sustained A/B of the residual entry (LowerOptions.residual,
soda_hip_run_device_residual) against a plain run, in ONE process, the arms
alternating in sub-blocks (as tools/ab.py and tools/batch_ab.py: clock drift
then shows instead of deciding):

  arm a  soda_hip_run_device on a program built WITHOUT the option -- the
         default kernels, what the others are measured against;
  arm b  the residual entry on a program built with it: the same passes, the
         deepest one last, launched as its twin;
  arm c  the residual entry forced onto the generic path
         (SODA_HIP_RESIDUAL_GENERIC=1): a one-iteration last pass plus
         `<app>_residual`.

All programs are built for the extent and calibrate by themselves on their
first run, as a caller's would.  Per kernel and twin: VGPRs, waves per SIMD,
and one launch timed alone (a run of exactly its depth).

  here (hiprtc, no GPU):  python tools/residual_ab.py --compile-only
                          python tools/residual_ab.py --regs profiles/residual_regs.json
  on the box:             python tools/residual_ab.py --out profiles/residual_ab.json

One JSON object: per case and arm the microseconds per run of every
sub-block, their median, minimum and maximum (the sub-block spread), the
schedule, and how the residual was taken."""
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
# the modules whose register counts profiles/residual_regs.json records
REGS = [
    ('jacobi2d.soda', 104, None, (13, 12, 8, 4), None),
    ('jacobi2d.soda', 104, None, (8, 4), 'preserve'),
    ('heat3d.soda', 48, None, (2,), None),
    ('heat3d.soda', 48, (512, 512, 512), (2,), None),
]


def resources(st, fuse, extent, residual):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(
      st, lower.LowerOptions(fuse=fuse, residual=residual), extent)
  mod = lower.lower(st, opts)
  res = runtime.kernel_resources(
      runtime.compile_source(mod.source, '%s.hip' % st.app_name))
  return mod, res, runtime.make_plan(mod, res)


def register_table(mod, res, plan):
  from soda_amd import runtime
  rows = []
  for i, k in enumerate(mod.kernels):
    if k.twin < 0:
      continue
    t = mod.kernels[k.twin]
    rows.append({
        'kernel': k.name, 'fused': k.tune.get('fused'),
        'vgpr': res[k.name]['vgpr'], 'twin_vgpr': res[t.name]['vgpr'],
        'waves_per_simd': runtime.waves_per_simd(res[k.name]['vgpr']),
        'twin_waves_per_simd': runtime.waves_per_simd(res[t.name]['vgpr']),
        'scratch': res[k.name]['scratch'], 'twin_scratch': res[t.name]['scratch'],
        'twin_kept': plan.kernels[i].twin >= 0})
  return rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3,
                  help='sub-blocks per arm per round')
  ap.add_argument('--only', type=int, nargs='*', help='indices into CASES')
  ap.add_argument('--out', help='also write the JSON object to this file')
  ap.add_argument('--compile-only', action='store_true')
  ap.add_argument('--regs', help='write the register table of REGS here '
                  '(no GPU) and stop')
  args = ap.parse_args()
  from soda_amd import core, runtime
  from soda_amd.codegen.hip import lower
  if args.regs:
    table = {'tool': 'tools/residual_ab.py --regs',
             'compiler': runtime.compiler_version(), 'modules': []}
    for name, iterate, extent, fuse, border in REGS:
      st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                          iterate=iterate, **({'border': border} if border
                                              else {}))
      mod, res, plan = resources(st, fuse, extent, True)
      table['modules'].append({
          'program': st.app_name, 'border': border or 'ignore',
          'extent': list(extent) if extent else None, 'fuse': list(fuse),
          'kernels': register_table(mod, res, plan),
          'generic': res['%s_residual' % st.app_name]})
    text = json.dumps(table, indent=1)
    print(text)
    with open(args.regs, 'w') as f:
      f.write(text + '\n')
    return
  out = {'tool': 'tools/residual_ab.py', 'unit': 'us per run (all iterations)',
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
    mod, res, plan = resources(st, fuse, extent, True)
    rec['registers'] = register_table(mod, res, plan)
    if args.compile_only:
      resources(st, fuse, extent, False)
      depths = [p.fused_iters for p in mod.sorted_passes()]
      rec['schedule'] = {str(t): c for t, c in zip(
          depths, runtime.plan_schedule(plan, extent, iterate)) if c}
      continue
    shape = tuple(extent[::-1])
    a_in = torch.rand(shape, device=dev, dtype=torch.float32)
    a_out = torch.empty_like(a_in)
    struct = torch.zeros(4, device=dev, dtype=torch.int64)
    plain = runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=extent)
    twin = runtime.Program(st, lower.LowerOptions(fuse=fuse, residual=True),
                           extent=extent)
    o, i, r = [a_out.data_ptr()], [a_in.data_ptr()], struct.data_ptr()

    def run_a(n=iterate):
      plain.run_device(o, i, extent, n, stream=stream)

    def run_b(n=iterate):
      os.environ.pop('SODA_HIP_RESIDUAL_GENERIC', None)
      twin.run_device(o, i, extent, n, stream=stream, residual=r)

    def run_c(n=iterate):
      os.environ['SODA_HIP_RESIDUAL_GENERIC'] = '1'
      twin.run_device(o, i, extent, n, stream=stream, residual=r)
      os.environ.pop('SODA_HIP_RESIDUAL_GENERIC', None)

    arms = (('a', plain, run_a), ('b', twin, run_b), ('c', twin, run_c))
    for arm, prog, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {
          'launches': prog.last_launches()[0],
          'schedule': {str(t): c for t, c in
                       prog.schedule(extent, iterate).items()},
          'residual': list(prog.last_residual()) if arm != 'a' else None,
          'us_per_run_by_block': []}
    rec['struct'] = twin.residual(r).__dict__
    for _ in range(args.rounds):
      rows = {arm: [] for arm, _, _ in arms}
      for _ in range(args.blocks):
        for arm, _, run in arms:
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
    rec['c_minus_a_us'] = round(med['c'] - med['a'], 1)
    rec['a_spread_us'] = round(rec['arms']['a']['max_us'] -
                               rec['arms']['a']['min_us'], 1)
    # one launch of every depth alone: the plain kernel against its twin
    rec['launch_us'] = {}
    for t in sorted({p.fused_iters for p in twin.module.sorted_passes()}):
      row = {}
      for arm, run in (('plain', run_a), ('twin', run_b)):
        run(t)
        torch.cuda.synchronize()
        took = []
        for _ in range(5):
          a, b = runtime.Event(), runtime.Event()
          a.record(stream)
          for _ in range(10):
            run(t)
          b.record(stream)
          torch.cuda.synchronize()
          took.append(a.elapsed_ms(b) * 100)
        row[arm] = round(min(took), 1)
        row[arm + '_how'] = (list(twin.last_residual()) if arm == 'twin'
                             else plain.schedule(extent, t))
      rec['launch_us'][str(t)] = row
    plain.close()
    twin.close()
    del a_in, a_out
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
