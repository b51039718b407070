#!/usr/bin/env python3
"""Sustained A/B of batched domains (soda_hip_border_create_batch,
soda_hip_periodic_create_batch) against what a caller did
before them, in ONE process, the two arms alternating in sub-blocks (as
tools/ab.py and tools/batch_ab.py: clock drift then shows instead of
deciding):

  arm A  an unbatched Program, ONE handle on the domain and a loop of N
         run_device calls on it, one per item, on one stream;
  arm B  a batched Program, one batched handle, ONE run_device call.

Both programs are built for the padded extent and calibrate by themselves on
their first run, as a caller's would.  The two arms write arrays of their own;
after the first job of each the outputs are compared bit for bit.

  here (hiprtc, no GPU):  python tools/domain_batch_ab.py --compile-only
  on the box:             python tools/domain_batch_ab.py \\
                              --out profiles/domain_batch_ab.json

One JSON object: per case and arm the microseconds per JOB (all N items, all
iterations) of every sub-block, their median, minimum and maximum, the kernel
launches of a job -- pads, the program's, fills, crops -- and whether the two
arms' outputs are bit-identical."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (program, iterate, items, extent, modes -- None: a torus --, jobs per
# sub-block)
CASES = [
    ('blur.soda', None, 64, (1920, 1080), 'clamp', 4),
    ('jacobi2d.soda', 104, 16, (1024, 1024), None, 4),
]


def _handle(prog, extent, modes, batch):
  if modes is None:
    return prog.periodic(extent, batch=batch)
  return prog.bordered(extent, modes, batch=batch)


def _launches(prog, info, iterate, items):
  """{pad, program, fill, crop} launches of ONE run_device call of a handle
  with `info` (one cell size: one helper launch per job)."""
  k = info['refill_every']
  chunks = [k] * (iterate // k) + ([iterate % k] if iterate % k else [])
  return {'pad': 1, 'crop': 1, 'fill': len(chunks), 'chunks': len(chunks),
          'program': sum(sum(prog.schedule(info['padded'], n, items).values())
                         for n in chunks)}


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
  out = {'tool': 'tools/domain_batch_ab.py', 'unit': 'us per job (all items, '
         'all iterations)', 'rounds': args.rounds, 'blocks': args.blocks,
         'cases': []}
  if not args.compile_only:
    import torch
    dev = torch.device('cuda', 0)
    stream = torch.cuda.current_stream().cuda_stream
    out['gpu'] = torch.cuda.get_device_name(0)
    tdt = {'float32': torch.float32, 'uint16': torch.int16}
  for at, (name, iterate, items, extent, modes, jobs) in enumerate(CASES):
    if args.only and at not in args.only:
      continue
    st = core.from_file(os.path.join(ROOT, 'tests/golden/soda', name),
                        **({'iterate': iterate} if iterate else {}))
    fuse = lower.DEFAULT_FUSE if st.iterate > 1 else ()
    k = max(fuse) if fuse and modes is None else 1
    lo, hi = runtime.periodic_ghosts(st, k)
    vec = lower.default_vec(st)
    padded = [l + n + h for l, n, h in zip(lo, extent, hi)]
    padded[0] = -(-padded[0] // vec) * vec
    rec = {'program': st.app_name, 'iterate': st.iterate, 'items': items,
           'extent': list(extent), 'domain': modes or 'torus',
           'padded': padded, 'jobs_per_block': jobs, 'launches_per_job': {},
           'arms': {}}
    out['cases'].append(rec)
    elem = st.input_types[0].size_in_bytes
    resources = runtime.wrap_resources if modes is None else \
        runtime.extend_resources
    rec['registers'] = {
        q: {f: v[f] for f in ('vgpr', 'sgpr', 'lds', 'scratch', 'code')}
        for batch in (False, True)
        for q, v in sorted(resources(elem, st.dim, batch=batch)[1].items())}
    if args.compile_only:
      for batch in (False, True):
        opts = runtime.resolve_options(
            st, lower.LowerOptions(fuse=fuse, batch=batch), padded)
        mod = lower.lower(st, opts)
        runtime.compile_source(mod.source, '%s.hip' % st.app_name)
      continue
    shape = (items,) + tuple(extent[::-1])

    def field(t, rand):
      dt = tdt[t.np_name]
      if not rand:
        return torch.zeros(shape, device=dev, dtype=dt)
      if dt.is_floating_point:
        return torch.rand(shape, device=dev, dtype=dt)
      return torch.randint(0, 100, shape, device=dev, dtype=dt)

    ins = [field(t, True) for t in st.input_types]
    outs_a = [field(t, False) for t in st.output_types]
    outs_b = [field(t, False) for t in st.output_types]
    step_in = [t[0].numel() * t.element_size() for t in ins]
    step_out = [t[0].numel() * t.element_size() for t in outs_a]
    prog_a = runtime.Program(st, lower.LowerOptions(fuse=fuse), extent=padded)
    prog_b = runtime.Program(st, lower.LowerOptions(fuse=fuse, batch=True),
                             extent=padded)
    dom_a = _handle(prog_a, extent, modes, None)
    dom_b = _handle(prog_b, extent, modes, items)
    rec['padded'] = list(dom_a.info()['padded'])
    assert dom_b.info() == dict(
        dom_a.info(), scratch_bytes=dom_a.info()['scratch_bytes'] * items)
    rec['refill_every'] = dom_a.info()['refill_every']
    rec['scratch_bytes'] = {'A': dom_a.info()['scratch_bytes'],
                            'B': dom_b.info()['scratch_bytes']}
    each = [([t.data_ptr() + i * s for t, s in zip(outs_a, step_out)],
             [t.data_ptr() + i * s for t, s in zip(ins, step_in)])
            for i in range(items)]
    whole = ([t.data_ptr() for t in outs_b], [t.data_ptr() for t in ins])

    def job_a():
      for o, i in each:
        dom_a.run_device(o, i, stream=stream)

    def job_b():
      dom_b.run_device(whole[0], whole[1], stream=stream)

    arms = (('A', prog_a, dom_a, job_a, 1), ('B', prog_b, dom_b, job_b, items))
    for arm, prog, dom, job, n in arms:
      job()                               # calibrates, allocates the scratch
      torch.cuda.synchronize()
      per_call = _launches(prog, dom.info(), st.iterate, n)
      calls = items if arm == 'A' else 1
      rec['launches_per_job'][arm] = dict(
          {q: v * calls for q, v in per_call.items() if q != 'chunks'},
          calls=calls, chunks_per_call=per_call['chunks'],
          total=calls * sum(v for q, v in per_call.items() if q != 'chunks'))
      rec['arms'][arm] = {
          'kernels': [q.name for q in prog.module.kernels],
          'us_per_job_by_block': []}
    rec['bit_identical'] = all(torch.equal(a, b)
                               for a, b in zip(outs_a, outs_b))
    for _ in range(args.rounds):
      rows = {arm[0]: [] for arm in arms}
      for _ in range(args.blocks):
        for arm, _, _, job, _ in arms:
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
    dom_a.close()
    dom_b.close()
    prog_a.close()
    prog_b.close()
    del ins, outs_a, outs_b
    torch.cuda.empty_cache()
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')


if __name__ == '__main__':
  main()
