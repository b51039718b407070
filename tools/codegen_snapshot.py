#!/usr/bin/env python3
"""What the HIP backend generates, as a file two trees can be compared by.

  tools/codegen_snapshot.py snapshot OUT.json
  tools/codegen_snapshot.py diff A.json B.json

`snapshot` lowers a fixed list of rows -- the rows the tests already use
(tests/knobs.py, tests/celltypes.py, tests/fuzz.py, the golden programs) and a
handful of hand-built MarchConfigs -- and records for each the sha256 of the
module source, the kernel names in order, every kernel's tile, block, LDS
bytes, twin and `tune`, every pass's fused_iters, kind, kernel list and
`traffic_model`, the sha256 of every chunk; or, where lowering refuses, the
exception's class and text.  It also prints how many rows produced a marching
kernel of each form (FORMS): a form without a row is a gap in the list.

`diff` prints every row that differs and exits non-zero if there is one or if
the row sets differ.  A change that claims to leave the generated code alone
takes a snapshot of its parent commit (this file copied into a checkout of
it) and one of its own tree, and shows an empty diff.

CPU only: no GPU, no library, no compiler."""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

FUZZ_SEEDS = range(0, 250)
WINDOW_SEEDS = range(0, 250)
GOLDEN_FUSE = ((4,), (13, 12, 8, 4))
GOLDEN_EXTENT = {1: (None, (600,)), 2: (None, (300, 90)),
                 3: (None, (130, 18, 28)), 4: (None, (40, 12, 10, 9))}

FORMS = (
    '2-D', '3-D', 'T=1', 'fused', 'dpp', 'mixh', 'edge loads taken',
    'edge loads declined', 'pipe 2', 'pipe 4', 'waves_x > 1', 'waves_y > 1',
    'xshare', 'xshare_block', 'banked', 'banked with lead', '_rs twin',
    'border: preserve', 'one-byte cells', 'sliding sum',
    'x-window + (V <= taps)', 'x-window + (V > taps)',
    'x-window min (V <= taps)', 'x-window min (V > taps)',
    'x-window max (V <= taps)', 'x-window max (V > taps)',
    'let', 'param', 'stamps', 'occupancy', 'min_waves', 'align_lanes > 1',
    'peel -1', 'peel 0', 'peel k', 'nt_store on', 'nt_load off',
    'xcd_swizzle off')


# ---------------------------------------------------------------------------
# rows: (id, a function that answers with the module or raises)
# ---------------------------------------------------------------------------

def _lower(stencil, kw, extent=None):
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, lower.LowerOptions(**kw), extent,
                                 probe=False)
  return lower.lower(stencil, opts)


def _text(v):
  return str(v).replace(' ', '')


def _knobs_rows():
  import knobs
  for prog in sorted(knobs.PROGRAMS):
    st = knobs.stencil_of(prog)
    rows = knobs.single_rows(prog) + knobs.pair_rows(prog)
    for twin in (False, True):
      for row in rows:
        kw = knobs.keywords(prog, row)
        if twin:
          kw['residual'] = True
        yield ('knobs%s/%s/%s' % ('_rs' if twin else '', prog,
                                  knobs.row_id(row)),
               lambda st=st, kw=kw: _lower(st, kw))
  # what the table says cannot be: the refusals and fall-backs themselves
  seen = set()
  for progs, o1, v1, o2, v2, _ in knobs.INADMISSIBLE:
    for prog in progs or sorted(knobs.PROGRAMS):
      if o1 not in knobs.options_of(prog):
        continue
      for a in v1:
        if o2 in (knobs.ANY, knobs.ALONE):
          rows = [{o1: a}]
        elif o2 in knobs.options_of(prog):
          rows = [knobs.context(o1, a, o2, b) for b in v2]
        else:
          rows = []
        for row in rows:
          rid = 'inadmissible/%s/%s' % (prog, knobs.row_id(row))
          if rid in seen:
            continue
          seen.add(rid)
          yield (rid, lambda prog=prog, row=row: _lower(
              knobs.stencil_of(prog), knobs.keywords(prog, row)))


def _celltype_rows():
  import celltypes as ct
  for t, dim, kind in ct.programs():
    for row in ct.ROWS:
      if row.dim == dim:
        yield ('celltypes/' + ct.row_id(t, row, kind),
               lambda t=t, row=row, kind=kind: _lower(
                   ct.stencil_of(t, row.dim, kind), ct.keywords(t, row, kind)))
  for t in ct.TYPES:
    for nb in ct.BANKS:
      for lead in (0, 4 * nb):
        kw = dict(fuse=(2,), peel=0, banks={'a': nb, 'b': nb})
        if lead:
          kw['bank_lead'] = {'a': lead}
        yield ('celltypes/%s-wire-%dbanks-lead%d' % (t, nb, lead),
               lambda t=t, kw=kw: _lower(ct.stencil_of(t, 2, 'main', 2), kw))


FUZZ_OPTIONS = (
    ('default', {}, {}),
    ('fuse2', dict(fuse=(2,), peel=0), {}),
    ('fuse32', dict(fuse=(3, 2), chunk_rows=9, waves_y=2), {}),
    ('preserve', dict(fuse=(2,)), dict(border='preserve')),
    ('xshare', dict(fuse=(2,), xshare=True, row_cells=300), {}),
)


def _fuzz_rows():
  import fuzz
  from soda_amd import core
  for rich in (False, True):
    for seed in FUZZ_SEEDS:
      text = fuzz.program(seed, rich)[0]
      for tag, kw, skw in FUZZ_OPTIONS:
        yield ('fuzz%s/%d/%s' % ('_rich' if rich else '', seed, tag),
               lambda text=text, kw=kw, skw=skw: _lower(
                   core.from_text(text, **skw), kw))
  for seed in WINDOW_SEEDS:
    text = fuzz.window_program(seed)[0]
    for tag, kw in (('default', {}), ('fuse2', dict(fuse=(2,), peel=0)),
                    ('nowindows', dict(fuse=(2,), windows=False)),
                    ('vec2', dict(fuse=(2,), vec=2)),
                    ('vec16', dict(vec=16))):
      yield ('wfuzz/%d/%s' % (seed, tag),
             lambda text=text, kw=kw: _lower(core.from_text(text), kw))


def _golden_rows():
  import knobs
  from soda_amd import core
  names = sorted(n for d in knobs.SODA_DIRS for n in os.listdir(d)
                 if n.endswith('.soda'))
  for name in names:
    for iterate in (None, 13):
      skw = {} if iterate is None else dict(iterate=iterate)
      for fuse in GOLDEN_FUSE:
        for which in (0, 1):
          def run(name=name, skw=skw, fuse=fuse, which=which):
            st = core.from_file(knobs.soda_path(name), **skw)
            return _lower(st, dict(fuse=fuse),
                          GOLDEN_EXTENT[st.dim][which])
          yield ('golden/%s/it%s/fuse%s/extent%d' %
                 (name, iterate, _text(fuse), which), run)


# MarchConfigs no LowerOptions reaches, through add_march_pass: (id, program,
# stencil keywords, MarchConfig keywords, bank slots of the module)
HAND_BUILT = [
    # three row steps per barrier (tests/test_lower_steps.py)
    ('pipe_rows3', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, vec=4, prefetch=4, pipe=2, pipe_rows=3, tile_rows=4),
     None),
    ('pipe_depth', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=3, pipe=2), None),
    ('pipe_waves', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, pipe=2, waves_x=2), None),
    ('pipe_banks', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, pipe=2, banks={'t1': 2}), {'t1': 2}),
    ('banks_differ', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, banks={'t1': 2}), {'t1': 4}),
    ('banks_vec', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, vec=2, banks={'t1': 4}), {'t1': 4}),
    ('bank_lead_odd', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, banks={'t1': 2}, bank_lead={'t1': 3}), {'t1': 2}),
    ('bank_lead_output', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, banks={'t1': 2}, bank_lead={'t0': 2}), {'t1': 2}),
    ('bank_lead', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=2, banks={'t1': 2}, bank_lead={'t1': 8}), {'t1': 2}),
    ('xshare_block1', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare_block=1), None),
    ('xshare_block17', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare_block=17), None),
    ('xshare_mixh', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=2, lane_shift='mixh'), None),
    ('xshare_pipe', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=2, pipe=2), None),
    ('xshare17', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=17), None),
    ('xshare_block_wins', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=3, xshare_block=2), None),
    ('xshare_rows25', 'heat3d.soda', dict(iterate=3),
     dict(fused_iters=2, prefetch=1, xshare=2, tile_rows=25), None),
    ('xshare_rows24', 'heat3d.soda', dict(iterate=3),
     dict(fused_iters=2, vec=1, prefetch=1, xshare=2, tile_rows=24), None),
    ('residual_pipe', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, pipe=2, residual=True), None),
    ('residual_seg', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare_block=2, residual=True), None),
    ('residual_waves', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, waves_y=2, residual=True), None),
    ('residual_xshare', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, xshare=2, residual=True), None),
    ('residual_preserve', 'jacobi2d.soda', dict(iterate=8, border='preserve'),
     dict(fused_iters=4, residual=True), None),
    ('unequal_fused', 'denoise2d.soda', {}, dict(fused_iters=2), None),
    ('four_dimensions', 'heat4d.soda', {}, dict(fused_iters=1), None),
    ('halo_too_wide', 'jacobi2d.soda', dict(iterate=13),
     dict(fused_iters=12, vec=1, prefetch=4, lane_shift='mixh'), None),
    ('window_too_tall', 'xcorr.soda', {},
     dict(fused_iters=1, prefetch=8, xwindow=False, slide=False), None),
    ('registers', 'denoise3d.soda', {},
     dict(fused_iters=1, vec=4, prefetch=1, tile_rows=24), None),
    ('shift_temps', 'contrast.soda', {}, dict(fused_iters=1, vec=1), None),
    ('stamps', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=4, stamps=True), None),
    ('stamps3d', 'heat3d.soda', dict(iterate=3),
     dict(fused_iters=2, prefetch=1, stamps=True, nt_load=False), None),
    ('occupancy_pipe', 'jacobi2d.soda', dict(iterate=13),
     dict(fused_iters=12, pipe=4, pipe_rows=4, occupancy=2), None),
    ('min_waves_nts', 'blur.soda', {},
     dict(fused_iters=1, min_waves=2, nt_store=True, nt_load=False,
          xcd_swizzle=False, align_lanes=4), None),
    ('align_half_strip', 'jacobi2d.soda', dict(iterate=13),
     dict(fused_iters=8, lane_shift='mixh', prefetch=4, align_lanes=4), None),
    ('no_edge', 'jacobi2d.soda', dict(iterate=8),
     dict(fused_iters=1, edge_loads=False), None),
    ('peel2', 'jacobi2d.soda', dict(iterate=13),
     dict(fused_iters=12, lane_shift='mixh', prefetch=4, peel=2), None),
    ('peel0', 'jacobi2d.soda', dict(iterate=13),
     dict(fused_iters=12, lane_shift='mixh', prefetch=4, peel=0), None),
    ('preserve', 'jacobi2d.soda', dict(iterate=8, border='preserve'),
     dict(fused_iters=4), None),
    ('preserve3d', 'heat3d.soda', dict(iterate=3, border='preserve'),
     dict(fused_iters=2, prefetch=1, nt_load=False), None),
    ('preserve_seg', 'jacobi2d.soda', dict(iterate=8, border='preserve'),
     dict(fused_iters=4, xshare_block=3), None),
    ('params', 'conv2d.soda', {}, dict(fused_iters=1, waves_x=2, waves_y=2),
     None),
    ('lets', 'lets2d.soda', {}, dict(fused_iters=1, vec=2), None),
    ('erosion_no_xwindow', 'erosion.soda', {},
     dict(fused_iters=1, vec=1, prefetch=1, xwindow=False), None),
    ('xcorr_no_slide', 'xcorr.soda', {},
     dict(fused_iters=1, vec=1, prefetch=1, slide=False), None),
    ('winsum_vec16', 'winsum2d.soda', {}, dict(fused_iters=1, vec=16), None),
    ('winsum_vec2_seg', 'winsum2d.soda', {},
     dict(fused_iters=1, vec=2, xshare_block=2), None),
]


def _hand_rows():
  import knobs
  from soda_amd import core
  from soda_amd.codegen.hip import lower
  for rid, soda, skw, ckw, slots in HAND_BUILT:
    def run(soda=soda, skw=skw, ckw=ckw, slots=slots):
      st = core.from_file(knobs.soda_path(soda), **skw)
      mod = lower.Module(st, slots)
      cfg = lower.MarchConfig(**ckw)
      lower.add_march_pass(mod, cfg)
      if not cfg.residual:
        lower.add_march_twin(mod, cfg)
      return mod
    yield 'hand/' + rid, run


def rows():
  for gen in (_knobs_rows, _celltype_rows, _fuzz_rows, _golden_rows,
              _hand_rows):
    for row in gen():
      yield row


# ---------------------------------------------------------------------------
# one row's record
# ---------------------------------------------------------------------------

def _sha(text):
  return hashlib.sha256(text.encode()).hexdigest()


def _canon(value):
  return json.dumps(value, sort_keys=True, default=repr)


_MARCH = re.compile(r'_march([23])d_(T\d+_V\d+_P\d+_W(\d+)x(\d+)_R\d+\S*)$')
_HEAD = re.compile(r'^// march[23]d: T=\d+ fused iteration\(s\), (\d+) cells/lane')


def _xwindow_forms(source):
  """The x-window forms of a module's text: (op, V above the taps?)."""
  out = set()
  vec = block = None
  for line in source.split('\n'):
    m = _HEAD.match(line)
    if m:
      vec = int(m.group(1))
    elif line.startswith('        int xw_') and ' = ' in line:
      taps = line.count('(int)')
      out.add(('+', vec > taps))
    elif line.startswith('        const ') and ' xm_' in line:
      first = '_b0 = ' in line
      if first:
        if block:
          out.add(tuple(block))
        block = ['?', False]
      elif block:
        block[1] = True
    if block and line.startswith('        ') and block[0] == '?':
      if 'SODA_MIN(' in line:
        block[0] = 'min'
      elif 'SODA_MAX(' in line:
        block[0] = 'max'
  if block:
    out.add(tuple(block))
  return out


def forms_of(mod):
  """The forms (FORMS) some marching kernel of `mod` has."""
  out = set()
  st = mod.stencil
  edges = {}
  for p in mod.passes:
    if p.kind.startswith('march'):
      edges[mod.kernels[p.kernels[0]].name] = tuple(p.traffic_model['edge'])
  marching = False
  for k in mod.kernels:
    m = _MARCH.search(k.name[:-3] if k.name.endswith('_bt') else k.name)
    if not m:
      continue
    marching = True
    key, tune = m.group(2), k.tune
    out.add('%s-D' % m.group(1))
    out.add('T=1' if tune['fused'] == 1 else 'fused')
    out.add(tune['lane_shift'])
    if tune['pipe'] in (2, 4):
      out.add('pipe %d' % tune['pipe'])
    if int(m.group(3)) > 1 and m.group(1) == '2':
      out.add('waves_x > 1')
    if int(m.group(4)) > 1 and m.group(1) == '2':
      out.add('waves_y > 1')
    if re.search(r'_xs\d', key):
      out.add('xshare')
    if '_xb' in key:
      out.add('xshare_block')
    if '_bk_' in key:
      out.add('banked with lead' if re.search(r'x\d+l\d+', key) else 'banked')
    if key.endswith('_rs'):
      out.add('_rs twin')
    edge = edges.get(k.name)
    if edge is not None and edge != (0, 0):
      out.add('edge loads taken')
    elif edge is not None and '_edge' in key and tune['pipe'] == 1 and \
        tune['lane_shift'] == 'dpp' and '_xs' not in key and '_xb' not in key:
      out.add('edge loads declined')
    for tag, form in (('_st', 'stamps'), ('_occ', 'occupancy'),
                      ('_mw', 'min_waves'), ('_al', 'align_lanes > 1'),
                      ('_nts', 'nt_store on')):
      if re.search(tag + r'(\d|_|$)', key):
        out.add(form)
    if '_ntl' not in key:
      out.add('nt_load off')
    if '_xcd' not in key:
      out.add('xcd_swizzle off')
    peel = re.search(r'_k(\d+)', key)
    out.add('peel -1' if not peel else
            'peel 0' if peel.group(1) == '0' else 'peel k')
  if not marching:
    return []
  source = '\n'.join(mod.chunks)
  if '  const bool keepx_' in source:
    out.add('border: preserve')
  if 'soda_own_register<' in source:
    out.add('one-byte cells')
  if '  int xa_' in source:
    out.add('sliding sum')
  for op, above in _xwindow_forms(source):
    out.add('x-window %s (V %s taps)' % (op, '>' if above else '<='))
  if any(s.stmt.let for s in st.ordered_stages):
    out.add('let')
  if st.param_names:
    out.add('param')
  return sorted(out)


def record(run):
  try:
    mod = run()
  except Exception as e:      # a refusal: SemanticError, InternalError, ...
    return {'refused': [type(e).__name__, str(e)]}
  return {
      'source': _sha(mod.source),
      'kernels': [k.name for k in mod.kernels],
      'descs': [_canon([k.block, k.tile, k.lds_bytes, k.note, k.twin])
                for k in mod.kernels],
      'tune': [_canon(k.tune) for k in mod.kernels],
      'passes': [_canon([p.fused_iters, p.kind, p.kernels, p.traffic_model])
                 for p in mod.passes],
      'chunks': [_sha(c) for c in mod.chunks],
      'forms': forms_of(mod),
  }


def snapshot(path):
  out = {}
  for rid, run in rows():
    if rid in out:
      raise SystemExit('row %s listed twice' % rid)
    out[rid] = record(run)
  with open(path, 'w') as f:
    json.dump(out, f, sort_keys=True, indent=0)
  report(out)
  return 0


def report(snap):
  refused = sum(1 for r in snap.values() if 'refused' in r)
  print('%d rows, %d refused' % (len(snap), refused))
  gaps = []
  for form in FORMS:
    n = sum(1 for r in snap.values() if form in r.get('forms', ()))
    print('  %-28s %5d' % (form, n))
    if not n:
      gaps.append(form)
  if gaps:
    print('NO ROW for: ' + ', '.join(gaps))


def diff(a_path, b_path):
  with open(a_path) as f:
    a = json.load(f)
  with open(b_path) as f:
    b = json.load(f)
  bad = 0
  for rid in sorted(set(a) | set(b)):
    if rid not in a or rid not in b:
      print('%s: only in %s' % (rid, a_path if rid in a else b_path))
      bad += 1
    elif a[rid] != b[rid]:
      fields = sorted(f for f in set(a[rid]) | set(b[rid])
                      if a[rid].get(f) != b[rid].get(f))
      print('%s: differs in %s' % (rid, ', '.join(fields)))
      for f in fields:
        print('    %s: %s\n    %s  %s' % (f, _canon(a[rid].get(f))[:300],
                                          ' ' * len(f),
                                          _canon(b[rid].get(f))[:300]))
      bad += 1
  report(b)
  print('%d differences' % bad)
  return 1 if bad else 0


def main(argv):
  if len(argv) == 3 and argv[1] == 'snapshot':
    return snapshot(argv[2])
  if len(argv) == 4 and argv[1] == 'diff':
    return diff(argv[2], argv[3])
  sys.stderr.write(__doc__)
  return 2


if __name__ == '__main__':
  sys.exit(main(sys.argv))
