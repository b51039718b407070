#!/usr/bin/env python3
"""Sustained A/B of a fused bordered run (soda_hip_border_fused_*, DESIGN.md
4.13), every dimension `clamp`, against the depth-1 loop and against the torus,
ONE program at its usual fusion depth, in ONE process, the arms alternating in
sub-blocks (as tools/ab.py and tools/border_ab.py: clock drift then shows
instead of deciding):

  arm b    soda_hip_border_run_padded at depth 1: one iteration, one fill,
           `iterate` times;
  arm f    soda_hip_border_fused_run_padded at depth 0 (the deepest pass);
  arm p    soda_hip_periodic_run_padded on the same grid: the torus;
  arm s<d> the iterations of ONE chunk of the strip of dimension d alone: a
           depth-1 bordered run of `depth` iterations on the strip's extent;
  arm g    one gather plus one scatter of every strip alone
           (soda_hip_border_fused_move).

  here (hiprtc, no GPU):  python tools/border_fused_ab.py --compile-only
  on the box:             python tools/border_fused_ab.py \\
                              --out profiles/border_fused_ab.json

One JSON object: per case and arm the microseconds per run of every sub-block,
their median, minimum and maximum; b / f, f / p, whether f's whole range lies
below b's, and what the strips and the moves of all chunks add up to."""
import argparse
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


def _padded(lo, hi, extent, vec):
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
  out = {'tool': 'tools/border_fused_ab.py', 'mode': MODE,
         'unit': 'us per run (arms b, f, p: all iterations; s<d>: the strip '
                 'iterations of one chunk; g: one gather and one scatter per '
                 'strip)',
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
    rlo, rhi, lo, hi = runtime.border_fused_ghosts(st, MODE, depth)
    padded = _padded(lo, hi, extent, vec)
    torus = _padded(*runtime.periodic_ghosts(st, depth), extent, vec)
    rec = {'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
           'padded': padded, 'torus_padded': torus, 'fuse': list(fuse),
           'runs_per_block': runs, 'arms': {}}
    out['cases'].append(rec)
    _, res = runtime.box_resources(4, st.dim)
    rec['registers'] = {q: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch',
                                              'code')}
                        for q, v in sorted(res.items())}
    opts = runtime.resolve_options(st, lower.LowerOptions(fuse=fuse), torus)
    if args.compile_only:
      mod = lower.lower(st, opts)
      runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      runtime.wrap_resources(4, st.dim)
      runtime.extend_resources(4, st.dim)
      continue
    p_in = torch.rand(tuple(padded[::-1]), device=dev, dtype=torch.float32)
    p_out = torch.empty_like(p_in)
    t_in = torch.rand(tuple(torus[::-1]), device=dev, dtype=torch.float32)
    t_out = torch.empty_like(t_in)
    prog = runtime.Program(st, opts, extent=torus)
    bor = prog.bordered(extent, MODE)
    fus = prog.bordered(extent, MODE, depth=0)
    per = prog.periodic(extent, depth)
    info = fus.info()
    assert list(info['padded']) == padded and info['depth'] == depth, info
    assert bor.info()['padded'] == info['padded'], bor.info()
    assert list(per.info()['padded']) == torus, per.info()
    rec['depth'] = info['depth']
    rec['chunks'] = -(-iterate // depth)
    rec['strips'] = [{k: s[k] for k in ('dim', 'lo', 'hi', 'take_lo',
                                        'take_hi', 'extent', 'padded')}
                     for s in info['strips']]
    rec['scratch_bytes'] = {'b': bor.info()['scratch_bytes'],
                            'f': info['scratch_bytes']}
    bor.fill([p_in.data_ptr()], stream=stream)     # arms b, f: extended
    per.fill([t_in.data_ptr()], stream=stream)     # arm p: wrapped
    po, pi = [p_out.data_ptr()], [p_in.data_ptr()]
    to, ti = [t_out.data_ptr()], [t_in.data_ptr()]
    strips = []
    for s in info['strips']:
      handle = prog.bordered(s['extent'], MODE)
      assert handle.info()['padded'] == s['padded'], (handle.info(), s)
      a = torch.rand(tuple(s['padded'][::-1]), device=dev,
                     dtype=torch.float32)
      handle.fill([a.data_ptr()], stream=stream)
      strips.append((handle, a, torch.empty_like(a)))

    def run_b():
      bor.run_padded(po, pi, iterate, stream=stream)

    def run_f():
      fus.run_padded(po, pi, iterate, stream=stream)

    def run_p():
      per.run_padded(to, ti, iterate, stream=stream)

    def run_s(k):
      handle, a, b = strips[k]
      return lambda: handle.run_padded([b.data_ptr()], [a.data_ptr()], depth,
                                       stream=stream)

    def run_g():
      for k, (_, a, b) in enumerate(strips):
        fus.gather(k, [a.data_ptr()], pi, stream=stream)
        fus.scatter(k, po, [b.data_ptr()], stream=stream)

    arms = [('b', run_b), ('f', run_f), ('p', run_p)] + [
        ('s%d' % s['dim'], run_s(k)) for k, s in enumerate(info['strips'])] + [
            ('g', run_g)]
    for arm, run in arms:
      run()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      rec['arms'][arm] = {'us_per_run_by_block': []}
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
    rec['b_over_f'] = round(med['b'] / med['f'], 3)
    rec['f_over_p'] = round(med['f'] / med['p'], 3)
    rec['f_range_below_b_range'] = \
        rec['arms']['f']['max_us'] < rec['arms']['b']['min_us']
    rec['strips_of_all_chunks_us'] = {
        q: round(rec['chunks'] * v, 1) for q, v in med.items() if q[0] == 's'}
    rec['moves_of_all_chunks_us'] = round(rec['chunks'] * med['g'], 1)
    rec['f_minus_p_us'] = round(med['f'] - med['p'], 1)
    for handle, _, _ in strips:
      handle.close()
    for handle in (bor, fus, per):
      handle.close()
    prog.close()
    del p_in, p_out, t_in, t_out, strips
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
