#!/usr/bin/env python3
"""Sustained A/B of the residual on a slab group (soda_hip_group_run_residual)
against plain group runs, in ONE process, the arms alternating in sub-blocks
(as tools/residual_ab.py: clock drift then shows instead of deciding):

  arm a  Group.run on a group built WITHOUT LowerOptions.residual;
  arm b  Group.run on a group built with it: the same launches -- asserted:
         every kernel the plain group launches has the same machine code in
         both builds (isa.isa_key without the code's position in its object);
  arm c  Group.run(residual=True) + Group.residual(): the last interval of
         every slab ends in its twin, then N structs are fetched and folded.

jacobi2d 8192^2 x 104 at fuse=(13, 12) on 4 VIRTUAL slabs of one GPU: the whole
schedule with its streams, events and copies, but the slabs share the GPU --
these are NOT scaling numbers.  What to read: (c) - (a) against the one-GPU
table's (b) - (a) (profiles/residual_ab.json: one twin launch's contention on
one struct; here four structs, a quarter of the waves each), and (b) - (a)
against (a)'s own spread.

  here (hiprtc, no GPU):  python tools/group_residual_ab.py --compile-only
  on the box:             python tools/group_residual_ab.py \\
                              --out profiles/group_residual_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASE = ('jacobi2d.soda', 104, (8192, 8192), (13, 12), 4)


def same_machine_code(plain, twin):
  """{kernel: key} of every kernel the plain build has; asserts the build with
  the option holds the same machine code for each."""
  from soda_amd import isa
  names = [k.name for k in plain.module.kernels]
  a, b = (isa.isa_keys(plain.code, names, placed=False),
          isa.isa_keys(twin.code, names, placed=False))
  for n in names:
    assert a[n] is not None and a[n] == b[n], \
        'kernel %s differs between the builds' % n
  return a


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=3)
  ap.add_argument('--blocks', type=int, default=3,
                  help='sub-blocks per arm per round')
  ap.add_argument('--runs', type=int, default=2, help='runs per sub-block')
  ap.add_argument('--out', help='also write the JSON object to this file')
  ap.add_argument('--compile-only', action='store_true')
  args = ap.parse_args()
  import numpy as np
  from soda_amd import core, isa, runtime
  from soda_amd.codegen.hip import lower
  name, iterate, extent, fuse, slabs = CASE
  st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                      iterate=iterate)
  out = {'tool': 'tools/group_residual_ab.py',
         'unit': 'us per run (all iterations, enqueue to synchronised)',
         'note': 'virtual slabs share one GPU: not scaling numbers',
         'program': st.app_name, 'iterate': iterate, 'extent': list(extent),
         'fuse': list(fuse), 'slabs': slabs, 'rounds': args.rounds,
         'blocks': args.blocks, 'runs_per_block': args.runs, 'arms': {}}
  if args.compile_only:
    own = extent[:-1] + (extent[-1] // slabs,)
    keys = []
    for residual in (False, True):
      opts = runtime.resolve_options(
          st, lower.LowerOptions(fuse=fuse, residual=residual), own)
      mod = lower.lower(st, opts)
      code = runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      keys.append((mod, code))
    names = [k.name for k in keys[0][0].kernels]
    a = isa.isa_keys(keys[0][1], names, placed=False)
    b = isa.isa_keys(keys[1][1], names, placed=False)
    assert all(a[n] is not None and a[n] == b[n] for n in names), (a, b)
    out['isa_keys'] = a
    print(json.dumps(out, indent=1))
    return
  import torch
  out['gpu'] = torch.cuda.get_device_name(0)
  rng = np.random.default_rng(0)
  ins = {'t1': rng.random(extent[::-1], dtype=np.float32)}
  plain = runtime.Group(st, extent, [0] * slabs, lower.LowerOptions(fuse=fuse))
  twin = runtime.Group(st, extent, [0] * slabs,
                       lower.LowerOptions(fuse=fuse, residual=True),
                       exchange_every=plain.exchange_every)
  out['isa_keys'] = same_machine_code(plain, twin)
  out['exchange_every'] = plain.exchange_every
  assert twin.exchange_every == plain.exchange_every
  plain.load(ins)
  twin.load(ins)

  def run_a():
    plain.run()
    plain.synchronize()

  def run_b():
    twin.run()
    twin.synchronize()

  def run_c():
    twin.run(residual=True)
    return twin.residual()

  arms = (('a', plain, run_a), ('b', twin, run_b), ('c', twin, run_c))
  for arm, group, run in arms:
    group.loaded()                        # (as every timed sub-block starts)
    run()                                 # sizes the scratch
    st_ = group.stats()
    out['arms'][arm] = {'launches': st_['launches'],
                        'split_passes': st_['split_passes'],
                        'intervals': st_['intervals'],
                        'us_per_run_by_block': []}
  assert out['arms']['a']['launches'] == out['arms']['b']['launches']
  out['arms']['c']['residual'] = [list(twin.last_residual(s))
                                  for s in range(slabs)]
  out['struct'] = run_c().__dict__
  for _ in range(args.rounds):
    rows = {arm: [] for arm, _, _ in arms}
    for _ in range(args.blocks):
      for arm, group, run in arms:
        # every sub-block starts from "just loaded": the count of iterations
        # the residual's box follows starts again (after ~4000 iterations the
        # valid box of this grid is empty and arm c would count nothing), and
        # all arms open their first interval alike, without an exchange
        group.loaded()
        t0 = time.perf_counter()
        for _ in range(args.runs):
          run()
        rows[arm].append(round((time.perf_counter() - t0) * 1e6 / args.runs, 1))
    for arm, row in rows.items():
      out['arms'][arm]['us_per_run_by_block'].append(row)
  for arm in out['arms'].values():
    flat = [x for row in arm['us_per_run_by_block'] for x in row]
    arm['median_us'] = round(statistics.median(flat), 1)
    arm['min_us'], arm['max_us'] = min(flat), max(flat)
  med = {k: v['median_us'] for k, v in out['arms'].items()}
  out['b_minus_a_us'] = round(med['b'] - med['a'], 1)
  out['c_minus_a_us'] = round(med['c'] - med['a'], 1)
  out['a_spread_us'] = round(out['arms']['a']['max_us'] -
                             out['arms']['a']['min_us'], 1)
  plain.close()
  twin.close()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
