"""The banked form of a wire stream's dense program (stream_specs(...,
banked=True), StreamProgram(..., banked=True)): the marching kernel addresses
the 2 or 4 device-resident banks of a tensor itself, through a buffer resource
per bank, and (de)interleaves in registers -- no unwire_ / wire_ kernel, no
staging array for such a tensor.

CPU: the default path is untouched, when the form is offered, the fragment <->
bank map against numpy's strided views, the kernels compile for gfx950.
GPU: every case against the reference's kernel contract (oracle/frt_layout.py)
AND against the banks the copy path leaves, with the stream's tail and guard
elements around every bank watched.  Extents are the smallest at which each
seam exists (strips, chunks, tiles, ragged ends)."""
import ctypes
import re

import numpy as np
import pytest

from conftest import soda_path


def _program(name, banks_in=1, banks_out=1, tile=None, iterate=None):
  """`name` with every input on `banks_in` banks, every output on `banks_out`,
  tile sizes replaced by `tile` (dimensions 0..dim-2)."""
  from soda_amd import core
  text = name if '\n' in name else open(soda_path(name)).read()

  def deal(m):
    nb = banks_in if m.group(1) == 'input' else banks_out
    first = int(m.group(2) or 0)
    return '%s dram %s ' % (m.group(1), '.'.join(
        str(first + b) for b in range(nb)))

  text = re.sub(r'^(input|output)(?: dram (\d+))? (?=\w+\s*:)', deal, text,
                flags=re.M)
  if tile:
    text = re.sub(r'\((\d+, )+\*\)',
                  '(%s, *)' % ', '.join(str(t) for t in tile), text, count=1)
  return core.from_text(text, **({'iterate': iterate} if iterate else {}))


APART = ('kernel: k\nburst width: 64\nunroll factor: 2\niterate: 2\n'
         'input dram 0.1 float: a(32, *)\ninput dram 2.3 float: b(32, *)\n'
         'output dram 0.1 float: a2(0, 0) = a(0, 1) + b(0, 0)\n'
         'output dram 2.3 float: b2(0, 0) = b(1, 0) + a(0, 0)\n')


# One side banked, the other on one bank: the stream format wants every tensor
# to move the same number of elements per cycle (burst width / cell width x
# banks), so the side on one bank has cells half as wide.
MIXED_IN = ('kernel: mixed_in\nburst width: 64\nunroll factor: 2\niterate: 1\n'
            'input dram 0 float: a(32, *)\n'
            'output dram 2 int16: b(0, 0) = a(0, 1) * 100.0f + a(1, 0) * 10.0f '
            '+ a(-1, -1)\n')
MIXED_OUT = ('kernel: mixed_out\nburst width: 64\nunroll factor: 2\niterate: 1\n'
             'input dram 0 int16: a(32, *)\n'
             'output dram 1 float: b(0, 0) = a(0, 1) * 0.5f + a(1, 0) + '
             'a(-1, -1)\n')


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('vec', [4, 8, 16])
@pytest.mark.parametrize('nb', [2, 4])
def test_fragment_map_is_numpys_strided_view(vec, nb):
  """Cell j of a fragment that starts on a bank-group boundary is element
  j / NB of the lane's piece of bank j % NB; the halo cells beside a strip
  lie in the banks the generator works out from their position alone.
  (`edge_cell_banks` drives the generated edge loads; `bank_fragment_map`
  restates the C++ helpers, which the GPU cases guard.)"""
  from soda_amd.codegen.hip import march
  stream = np.arange(1000, 1000 + 40 * vec)
  banks = [stream[b::nb] for b in range(nb)]
  fmap = march.bank_fragment_map(vec, nb)
  assert len(fmap) == vec
  for first in range(0, len(stream) - vec + 1, vec):    # every lane's fragment
    for j, (bank, idx) in enumerate(fmap):
      assert banks[bank][first // nb + idx] == stream[first + j]
    # every bank gives vec / nb CONSECUTIVE elements from first / nb on
    for b in range(nb):
      assert sorted(i for bank, i in fmap if bank == b) == list(range(vec // nb))
  for i in range(2):
    left, right = march.edge_cell_banks(i, vec, nb)
    for first in range(vec, len(stream) - 2 * vec, vec):
      cell = first - 1 - i                    # left of a strip that starts here
      assert banks[left][cell // nb] == stream[cell]
      cell = first + vec + i                  # right of a strip whose last lane
      assert banks[right][cell // nb] == stream[cell]   # starts here


def test_fragments_that_split_a_bank_group_are_refused():
  from soda_amd import util
  from soda_amd.codegen.hip import march
  with pytest.raises(util.SemanticError):
    march.bank_fragment_map(2, 4)
  with pytest.raises(util.SemanticError):
    march.edge_cell_banks(0, 1, 2)


CPU_PROGRAMS = [
    ('jacobi2d.soda', 2, 2, None, None),
    ('jacobi2d.soda', 4, 4, None, None),
    ('jacobi2d.soda', 2, 2, (520,), None),
    ('blur.soda', 2, 2, (2048,), None),
    ('blur.soda', 4, 4, (2048,), None),
    ('blur.soda', 3, 3, (1008,), None),
    ('sobel2d.soda', 2, 2, None, None),
    ('heat3d.soda', 2, 2, None, None),
    ('heat3d.soda', 2, 2, (34, 32), None),
    ('denoise2d.soda', 2, 2, None, None),
    ('coupled2d.soda', 2, 2, None, None),
    (MIXED_IN, 2, 1, None, None),
    (MIXED_OUT, 1, 2, None, None),
]


@pytest.fixture(scope='module')
def specs(built):
  """stream_specs of every program of this file, built once."""
  from soda_amd import stream
  memo = {}

  def get(case, **kw):
    key = (case, tuple(sorted(kw.items())))
    if key not in memo:
      memo[key] = (_program(*case),) + stream.stream_specs(_program(*case), **kw)
    return memo[key]
  return get


@pytest.mark.parametrize('case', CPU_PROGRAMS)
def test_defaults_are_bit_identical(specs, case):
  """Opt-in: without banked=True every source and plan is what it was, and
  with it every OTHER tag's too."""
  _, d0, s0 = specs(case)
  _, d1, s1 = specs(case, banked=False)
  _, d2, s2 = specs(case, banked=True)
  assert 'dense_banked' not in s0 and 'dense_banked' not in s1
  assert bytes(d0) == bytes(d1) == bytes(d2)
  assert list(s0) == list(s1) == [t for t in s2
                                  if not t.startswith('dense_banked')]
  for tag in s0:
    for other in (s1, s2):
      assert s0[tag].source == other[tag].source, tag
      assert bytes(s0[tag].plan) == bytes(other[tag].plan), tag
      assert s0[tag].kernel_names == other[tag].kernel_names, tag
    assert 'banked' not in s0[tag].source and '_bk' not in s0[tag].source


def test_offer_rules(specs):
  from soda_amd import core, stream
  # two banks each side: both tensors in the kernel, neither copy kernel used
  st, _, sp = specs(('jacobi2d.soda', 2, 2, None, None), banked=True)
  b = sp['dense_banked']
  assert b.in_kernel == {'t1': 2, 't0': 2}
  assert b.plan.num_inputs == 2 and b.plan.num_outputs == 2
  assert b.plan.num_passes == 1 and b.plan.passes[0].fused_iters == 1
  assert b.plan.passes[0].num_kernels == 1 and len(b.kernel_names) == 1
  assert '_T2_' in b.kernel_names[0] and '_bk' in b.kernel_names[0]
  assert b.kernel_names[0] not in sp['dense'].kernel_names
  assert 'soda_unwire' not in b.source and 'soda_wire' not in b.source
  # two iterations: also as two launches of the one-iteration kernel, the
  # first reads the banks, the last writes them
  first, last = sp['dense_banked_first'], sp['dense_banked_last']
  assert first.in_kernel == {'t1': 2} and last.in_kernel == {'t0': 2}
  assert (first.plan.num_inputs, first.plan.num_outputs) == (2, 1)
  assert (last.plan.num_inputs, last.plan.num_outputs) == (1, 2)
  for one in (first, last):
    assert '_T1_' in one.kernel_names[0] and '_bk_' in one.kernel_names[0]
    assert one.plan.num_passes == 1 and one.plan.passes[0].fused_iters == 1
  # ... of two-iteration programs only
  for case in (('blur.soda', 2, 2, (2048,), None),
               ('coupled2d.soda', 2, 2, None, None)):
    assert 'dense_banked' in specs(case, banked=True)[2]
    assert 'dense_banked_first' not in specs(case, banked=True)[2]
  # three banks: no fragment is whole bank groups
  _, _, sp = specs(('blur.soda', 3, 3, (1008,), None), banked=True)
  assert 'dense_banked' not in sp and 'wire_blur_y' in sp
  # a bank count that does not divide the tile row
  st = _program('jacobi2d.soda', 4, 4, (34,))
  assert 'dense_banked' not in stream.stream_specs(st, banked=True)[1]
  # more launches than one: dense temporaries in between
  st = _program('jacobi2d.soda', 2, 2, None, 100)
  assert 'dense_banked' not in stream.stream_specs(st, banked=True)[1]
  # outputs that are not born at their wire positions keep wire_<out>
  st = core.from_text(APART)
  assert stream.emit_late(st) is None
  sp = stream.stream_specs(st, banked=True)[1]
  assert 'wire_a2' in sp and 'wire_b2' in sp
  if 'dense_banked' in sp:
    assert not set(sp['dense_banked'].in_kernel) & {'a2', 'b2'}
  st = _program('jacobi2d.soda', 2, 2)
  sp = stream.stream_specs(st, banked=True, direct=False)[1]
  assert 'wire_t0' in sp and sp['dense_banked'].in_kernel == {'t1': 2}
  # mixed: only the banked side
  _, _, sp = specs((MIXED_IN, 2, 1, None, None), banked=True)
  assert sp['dense_banked'].in_kernel == {'a': 2}
  assert sp['dense_banked'].plan.num_inputs == 2
  assert sp['dense_banked'].plan.num_outputs == 1
  assert 'unwire_a' in sp and 'wire_b' not in sp
  _, _, sp = specs((MIXED_OUT, 1, 2, None, None), banked=True)
  assert sp['dense_banked'].in_kernel == {'b': 2}
  assert 'unwire_a' not in sp and 'wire_b' in sp
  # a delayed input: the delay is a multiple of the bank count
  st, _, sp = specs(('denoise2d.soda', 2, 2, None, None), banked=True)
  assert stream.input_shifts(st) == {'f': 64, 'u': 0}
  assert sp['dense_banked'].in_kernel == {'f': 2, 'u': 2, 'output': 2}
  assert 'a.reserved[0] - 64' in sp['dense_banked'].source
  # ... and of the cells per lane: the start into the banks and the end of
  # the clipped window then fall on fragment boundaries
  for shift, vec, want in ((64, 2, True), (6, 2, True), (6, 4, False),
                           (3, 2, False)):
    got = stream.banked_tensors(st, vec, True, {'f': shift, 'u': 0})
    assert ('f' in got) == want and 'u' in got, (shift, vec)
  # the linear form, a 1-D program: nothing to offer
  st = _program('jacobi2d.soda', 2, 2)
  assert 'dense_banked' not in stream.stream_specs(st, dense=False,
                                                   banked=True)[1]


def test_families_without_the_form_refuse_it(built):
  from soda_amd import util
  from soda_amd.codegen.hip import lower
  st = _program('heat3d.soda', 2, 2)
  for opts in (dict(strategy='direct'), dict(strategy='tile3d', fuse=(2,)),
               dict(strategy='ldswin')):
    with pytest.raises(util.SemanticError):
      lower.lower(st, lower.LowerOptions(banks={'in': 2}, **opts))
  j = _program('jacobi2d.soda', 2, 2, None, 4)
  # stage-pipelined blocks: the depth is dropped, no fused pass is left
  mod = lower.lower(j, lower.LowerOptions(fuse=(4,), pipe=2, vec=4,
                                          banks={'t1': 2, 't0': 2}))
  assert [p.fused_iters for p in mod.passes] == [1]
  with pytest.raises(util.SemanticError):       # NB does not divide V
    lower.lower(j, lower.LowerOptions(strategy='march', fuse=(), vec=2,
                                      banks={'t1': 4}))
  with pytest.raises(util.SemanticError):       # two or four banks
    lower.lower(j, lower.LowerOptions(banks={'t1': 3}))


@pytest.mark.parametrize('case', [c for c in CPU_PROGRAMS if c[1] != 3])
def test_banked_kernels_compile_for_gfx950(specs, case):
  """... with NB buffer resources per tensor the kernel addresses itself and
  one per tensor it does not."""
  from soda_amd import runtime
  st, _, sp = specs(case, banked=True)
  assert 'dense_banked' in sp
  for tag in [t for t in sp if t.startswith('dense_banked')]:
    _banked_kernel_text(st, sp[tag])


def _banked_kernel_text(st, b):
  from soda_amd import runtime
  code = runtime.compile_source(b.source, '%s_banked.hip' % st.app_name)
  res = runtime.kernel_resources(code)
  assert res[b.kernel_names[0]]['scratch'] == 0
  body = b.source[b.source.index('extern "C" __global__'):]
  for n in list(st.input_names) + list(st.output_names):
    which = 'r' if n in st.input_names else 'w'
    nb = b.in_kernel.get(n)
    if nb:
      made = re.findall(r'const soda_rsrc_t %s_%s_b(\d) = soda_make_rsrc_bank<%d>'
                        % (which, n, nb), body)
      assert made == [str(i) for i in range(nb)], n
      assert not re.search(r'soda_rsrc_t %s_%s =' % (which, n), body)
    else:
      assert len(re.findall(r'soda_rsrc_t %s_%s = soda_make_rsrc\('
                            % (which, n), body)) == 1, n
  # the slots: inputs bank by bank, then outputs
  slots = sum(b.in_kernel.get(n, 1) for n in st.input_names)
  assert b.plan.num_inputs == slots
  assert b.plan.num_outputs == sum(b.in_kernel.get(n, 1)
                                   for n in st.output_names)
  assert b.plan.num_inputs + b.plan.num_outputs <= 15


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def model_schedules(monkeypatch):
  """Every program of these tests schedules its passes by the model, never by
  timing them (read when a program is loaded): which launches the copy arm of
  a GPU case runs is then the same in every run, and from the same source as
  the banked arm's."""
  monkeypatch.setenv('SODA_HIP_NO_CALIBRATE', '1')


GUARD = 64           # bytes around every device bank
FILL = 0xA5          # what output banks and guards hold before a run


def _inputs(stencil, extent, seed):
  rng = np.random.default_rng(seed)
  ins = {}
  for n, t in zip(stencil.input_names, stencil.input_types):
    shape = tuple(extent[::-1])
    ins[n] = (rng.random(shape).astype(t.np_name) if t.is_float else
              rng.integers(-100, 100, shape).astype(t.np_name))
  return ins


def _device_run(prog, layout, in_banks, lead=0):
  """Runs `prog` on device copies of `in_banks`; every bank sits `GUARD + lead`
  bytes into an allocation filled with FILL.  Returns ({output: [bank bytes,
  guards included]}, last_mode)."""
  import torch
  st = prog.stencil
  dev_in, dev_out = {}, {}
  for n in st.input_names:
    dev_in[n] = []
    for bank in in_banks[n]:
      t = torch.full((2 * GUARD + bank.nbytes,), FILL, dtype=torch.uint8,
                     device='cuda')
      t[GUARD + lead:GUARD + lead + bank.nbytes] = torch.from_numpy(
          bank.view(np.uint8).copy()).cuda()
      dev_in[n].append(t)
  from oracle import frt_layout
  shapes = frt_layout.alloc(layout, st.output_names)
  for n in st.output_names:
    dev_out[n] = [torch.full((2 * GUARD + bank.nbytes,), FILL,
                             dtype=torch.uint8, device='cuda')
                  for bank in shapes[n]]
  assert all(t.data_ptr() % 16 == 0 for ts in list(dev_in.values()) +
             list(dev_out.values()) for t in ts)
  prog.run_banked_device(
      {n: [t.data_ptr() + GUARD + lead for t in ts] for n, ts in dev_out.items()},
      {n: [t.data_ptr() + GUARD + lead for t in ts] for n, ts in dev_in.items()},
      layout.cycle_count, stream=torch.cuda.current_stream().cuda_stream)
  torch.cuda.synchronize()
  return ({n: [t.cpu().numpy() for t in ts] for n, ts in dev_out.items()},
          prog.last_mode)


def _check_case(stencil, extent, expect='banked', lead=0, seed=7,
                in_kernel=None):
  from oracle import frt_layout
  from soda_amd import stream
  layout = stream.WireLayout(stencil, extent)
  ins = _inputs(stencil, extent, seed)
  in_banks = frt_layout.scatter(layout, ins)
  shapes = frt_layout.alloc(layout, stencil.output_names)
  n = layout.cycle_count * layout.epc[stencil.input_names[0]]
  block = int(np.prod(stencil.tile_size[:-1]))
  view = (n // block) * block                  # elements of the dense view
  assert 0 < view <= n
  prog = stream.StreamProgram(stencil, dense=True, banked=True)
  try:
    if in_kernel is not None:
      assert prog.specs['dense_banked'].in_kernel == in_kernel
    raw, mode = _device_run(prog, layout, in_banks, lead)
    picked = dict(prog.specs['dense_banked'].in_kernel) \
        if 'dense_banked' in prog.specs else {}
  finally:
    prog.close()
  copy = stream.StreamProgram(stencil, dense=True, banked=False)
  try:
    raw_copy, mode_copy = _device_run(copy, layout, in_banks, lead)
    copy_launches = ctypes.c_int32()
    copy._lib.soda_hip_last_launches(copy._programs['dense'],
                                     ctypes.byref(copy_launches), None)
  finally:
    copy.close()
  # (d) the path taken
  assert mode == expect and mode_copy == 'dense'

  def banks_of(raw_banks):
    return {o: [r[GUARD + lead:GUARD + lead + shapes[o][b].nbytes].view(
        shapes[o][b].dtype) for b, r in enumerate(rs)]
            for o, rs in raw_banks.items()}
  got_banks, copy_banks = banks_of(raw), banks_of(raw_copy)
  # (a) what the host gathers is what the kernel contract leaves
  got = {o: np.zeros(tuple(extent[::-1]), np.dtype(t.np_name))
         for o, t in zip(stencil.output_names, stencil.output_types)}
  ref = {o: np.zeros_like(got[o]) for o in got}
  frt_layout.gather(layout, got_banks, got)
  frt_layout.gather(layout, frt_layout.kernel_on_streams(layout, in_banks), ref)
  boxes = [stencil.valid_box(extent, o) for o in stencil.output_names]
  lo = [max(b[0][d] for b in boxes) for d in range(stencil.dim)]
  hi = [min(b[1][d] for b in boxes) for d in range(stencil.dim)]
  idx = tuple(slice(l, h) for l, h in zip(lo[::-1], hi[::-1]))
  for o in stencil.output_names:
    assert ref[o][idx].any()
    if len(stencil.output_names) == 1:
      assert np.array_equal(got[o], ref[o]), o
    else:
      assert np.array_equal(got[o][idx], ref[o][idx]), o
  for o in stencil.output_names:
    nb = layout.bank_count[o]
    for b in range(nb):
      inside = len(range(b, view, nb))         # elements of the dense view
      print('%s bank %d: %d of %d elements of the dense view differ from the '
            'copy path (its dense program: %d launch(es))' %
            (o, b, int((got_banks[o][b][:inside] !=
                        copy_banks[o][b][:inside]).sum()), inside,
             copy_launches.value))
      # (b) the same banks as the copy path, over the dense view
      assert np.array_equal(got_banks[o][b][:inside],
                            copy_banks[o][b][:inside]), (o, b)
      # (c) guards, and -- where the program itself writes the bank -- the tail
      r = raw[o][b]
      assert (r[:GUARD + lead] == FILL).all(), (o, b)
      assert (r[GUARD + lead + shapes[o][b].nbytes:] == FILL).all(), (o, b)
      if mode == 'banked' and (o in picked or nb == 1):
        tail = r[GUARD + lead + inside * shapes[o][b].itemsize:]
        assert (tail == FILL).all(), (o, b)
  return picked


def _rows_spanning_chunks(stencil, rows):
  """A row count (last dimension of the dense view) on which the banked kernel
  runs at least two chunks, from the kernel's own launch geometry."""
  from soda_amd import runtime, stream
  plan = stream.stream_specs(stencil, dense=True, banked=True)[1][
      'dense_banked'].plan
  for _ in range(4):
    tiles, _ = runtime.plan_geometry(plan,
                                     tuple(stencil.tile_size[:-1]) + (rows,))
    chunk = tiles[0][stencil.dim - 1]
    if rows > chunk + 2:
      return rows, chunk
    rows = 2 * chunk + 3
  raise AssertionError('no extent of two chunks found')


GPU_CASES = [
    # jacobi2d fp32, iterate 2 in one fused kernel, two banks each side
    ('jacobi2d.soda', 2, 2, None, (32, 45)),
    ('jacobi2d.soda', 2, 2, None, (100, 9)),         # four overlapping tiles
    ('jacobi2d.soda', 2, 2, (520,), (520, 70)),      # 3 strips, ragged last
    ('jacobi2d.soda', 4, 4, None, (32, 45)),         # four banks: 4-byte pieces
    # blur uint16: 8 cells per lane, packed de-interleave, two stages
    ('blur.soda', 2, 2, (2048,), (2048, 20)),
    ('blur.soda', 4, 4, (2048,), (2048, 20)),
    ('blur.soda', 2, 2, (2048,), (5000, 37)),        # three tiles, ragged last
    ('blur.soda', 4, 4, (2048,), (5000, 37)),
    ('sobel2d.soda', 2, 2, None, (32, 8)),           # int16, three stages
    # heat3d fp32, iterate 2, rows shared through LDS
    ('heat3d.soda', 2, 2, None, (32, 32, 9)),
    ('heat3d.soda', 2, 2, None, (70, 40, 7)),        # 3 x 2 tiles
    ('heat3d.soda', 2, 2, (34, 32), (34, 32, 9)),    # even, no multiple of 4
    ('denoise2d.soda', 2, 2, None, (32, 14)),        # f delayed by 64 = 32 x NB
    ('coupled2d.soda', 2, 2, None, (32, 14)),        # two outputs circulate
    ('coupled2d.soda', 2, 2, None, (32, 11)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('name,nb_in,nb_out,tile,extent', GPU_CASES)
def test_banked_form_on_device_banks(built, name, nb_in, nb_out, tile, extent):
  """(a) reference agreement, (b) the copy path's banks over the dense view,
  (c) tail and guards untouched, (d) `last_mode == 'banked'`.

  (b) covers the array's border cells, which no host gathers and on which a
  fused kernel and the same iterations as separate launches do not agree (a
  fused kernel computes intermediate rows outside the array from the rows
  inside, separate launches read them as zero).  The banked path takes the
  launches the dense program's MODEL schedule names -- heat3d's two iterations
  on 32 x 32 tiles: two one-iteration launches, the first reads the banks, the
  last writes them -- so the copy arm is scheduled by the model here as well
  (`model_schedules`); scheduled by the clock it may split otherwise."""
  st = _program(name, nb_in, nb_out, tile)
  picked = _check_case(st, extent)
  assert set(picked) == set(st.input_names) | set(st.output_names)


@pytest.mark.gpu
def test_banked_form_across_chunks(built):
  """Tile 520: three strips per row, and a row count the kernel's own geometry
  cuts into at least two chunks."""
  st = _program('jacobi2d.soda', 2, 2, (520,))
  rows, chunk = _rows_spanning_chunks(st, 70)
  # (the dense view holds a few rows more than the array: the void tail)
  assert rows > chunk
  _check_case(st, (520, rows), in_kernel={'t1': 2, 't0': 2})


@pytest.mark.gpu
@pytest.mark.parametrize('text,nb_in,nb_out,want', [
    (MIXED_IN, 2, 1, {'a': 2}), (MIXED_OUT, 1, 2, {'b': 2})])
def test_banked_form_of_one_side_only(built, text, nb_in, nb_out, want):
  """Tensors are decided one by one: the side on one bank is read / written
  in place as before."""
  st = _program(text, nb_in, nb_out)
  _check_case(st, (32, 21), in_kernel=want)


@pytest.mark.gpu
def test_misaligned_banks_take_the_copy_path(built):
  """Banks that start 4 bytes into their allocations: the call succeeds on
  the copy path and leaves the same streams."""
  st = _program('jacobi2d.soda', 2, 2)
  _check_case(st, (32, 45), expect='dense', lead=4)


@pytest.mark.gpu
def test_three_banks_run_the_copy_path(built):
  st = _program('blur.soda', 3, 3, (1008,))
  picked = _check_case(st, (1008, 9), expect='dense')
  assert picked == {}
