#!/usr/bin/env python3
"""A/B of the banked form of a wire stream's dense program (StreamProgram(...,
banked=True)) on device-resident banks.  Three arms per case, alternated in one
process, every window a few hundred calls between two device events:

  copy     banked=False: unwire_ kernels, the dense program, wire_ kernels
  banked   banked=True:  the marching kernel addresses the banks itself
  floor    the same program with every tensor on ONE bank (read / written in
           place by the dense program): what no banked form can beat

Writes one JSON document (--out, default profiles/wire_banked_ab.json) with the
per-window times, their mean / min / max / standard deviation, the path every
arm took, the launches of every program it ran in its last call (the copy and
floor arms schedule an iterated program by the clock, the banked arm by the
model: `launched` says what each really ran) and the VGPRs of those
kernels."""
import argparse
import ctypes
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [
    # (label, file, tile, extent, iterate, banks per tensor)
    ('blur 16384^2, four banks', 'blur.soda', (16384,), (16384, 16384), 1, 4),
    ('blur 16384^2, two banks', 'blur.soda', (16384,), (16384, 16384), 1, 2),
    ('jacobi2d 8192^2 x 1, two banks', 'jacobi2d.soda', (8192,), (8192, 8192),
     1, 2),
    ('heat3d 512^3 x 2, 512 x 512 tiles, two banks', 'heat3d.soda', (512, 512),
     (512, 512, 512), 2, 2),
]


def program(name, tile, iterate, banks):
  from soda_amd import core
  text = open(os.path.join(ROOT, 'tests', 'golden', 'soda', name)).read()
  dram = '.'.join(map(str, range(banks)))
  text = re.sub(r'(input|output) dram [\d.]+', r'\1 dram ' + dram, text)
  return core.from_text(text, iterate=iterate, tile_size=list(tile))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--steps', type=int, default=200, help='calls per window')
  ap.add_argument('--rounds', type=int, default=7, help='windows per arm')
  ap.add_argument('--only', type=int, nargs='*', default=None,
                  help='indices into the case list')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                                'wire_banked_ab.json'))
  args = ap.parse_args()
  from soda_amd import runtime, stream
  lib = runtime.library()
  if runtime.device_count() < 1:
    raise SystemExit('no GPU: nothing to measure')
  try:
    import torch
    device = torch.cuda.get_device_name(0)
  except Exception:
    device = 'unknown'
  results = []

  def launched(prog):
    """{spec tag: {launches, fused launches, kernels with VGPRs}} of the
    marching programs `prog` ran in its last call."""
    out = {}
    for tag in ('dense', 'dense_banked', 'dense_banked_first',
                'dense_banked_last'):
      if tag not in prog.specs:
        continue
      la, fu = ctypes.c_int32(), ctypes.c_int32()
      lib.soda_hip_last_launches(prog._programs[tag], ctypes.byref(la),
                                 ctypes.byref(fu))
      if not la.value:
        continue
      spec = prog.specs[tag]
      res = runtime.kernel_resources(runtime.compile_source(
          spec.source, '%s.hip' % tag))
      out[tag] = {'launches': la.value, 'fused_launches': fu.value,
                  'kernels_of_the_program': {
                      k: res.get(k, {}).get('vgpr') for k in spec.kernel_names}}
    return out

  for index, (label, name, tile, extent, iterate, nb) in enumerate(CASES):
    if args.only is not None and index not in args.only:
      continue
    arms = {}
    allocated = []

    def dev_banks(st, lay, names):
      out = {}
      for n in names:
        count = lay.bank_count[n]
        out[n] = []
        for _ in range(count):
          p = ctypes.c_void_p()
          nbytes = lay.buf_elems[n] // count * st.symbol_table[n].size_in_bytes
          runtime.check(lib.soda_hip_malloc(0, nbytes, ctypes.byref(p)),
                        'malloc')
          runtime.check(lib.soda_hip_memset(p, 1, nbytes, None), 'memset')
          out[n].append(p.value)
          allocated.append(p)
      return out

    for arm, banks, banked in (('copy', nb, False), ('banked', nb, True),
                               ('floor', 1, False)):
      st = program(name, tile, iterate, banks)
      lay = stream.WireLayout(st, extent)
      prog = stream.StreamProgram(st, banked=banked)
      arms[arm] = dict(prog=prog, lay=lay,
                       ins=dev_banks(st, lay, st.input_names),
                       outs=dev_banks(st, lay, st.output_names), ms=[])
    for a in arms.values():                       # warm every arm's kernels
      for _ in range(5):
        a['prog'].run_banked_device(a['outs'], a['ins'], a['lay'].cycle_count)
    runtime.synchronize()
    for _ in range(args.rounds):
      for a in arms.values():
        e0, e1 = runtime.Event(), runtime.Event()
        e0.record()
        for _ in range(args.steps):
          a['prog'].run_banked_device(a['outs'], a['ins'], a['lay'].cycle_count)
        e1.record()
        runtime.synchronize()
        a['ms'].append(e0.elapsed_ms(e1) / args.steps)
    row = {'case': label, 'extent': list(extent), 'tile': list(tile),
           'iterate': iterate, 'banks': nb, 'steps_per_window': args.steps,
           'arms': {}}
    for arm, a in arms.items():
      row['arms'][arm] = {
          'path': a['prog'].last_mode,
          'launched': launched(a['prog']),
          'ms_per_call': [round(v, 5) for v in a['ms']],
          'mean_ms': round(statistics.mean(a['ms']), 5),
          'min_ms': round(min(a['ms']), 5), 'max_ms': round(max(a['ms']), 5),
          'stdev_ms': round(statistics.pstdev(a['ms']), 5)}
    specs = arms['banked']['prog'].specs
    if 'dense_banked' in specs:
      row['in_kernel'] = specs['dense_banked'].in_kernel
    print(json.dumps(row), flush=True)
    results.append(row)
    for a in arms.values():
      a['prog'].close()
    for p in allocated:
      lib.soda_hip_free(0, p)
  with open(args.out, 'w') as f:
    json.dump({'tool': 'tools/wire_banked_ab.py', 'device': device,
               'compiler': runtime.compiler_version(), 'cases': results}, f,
              indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
