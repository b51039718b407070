"""Batched domains: many tori or bordered grids of one extent in one launch per
kernel (soda_hip_periodic_create_batch, soda_hip_border_create_batch and their
plan entries).

Every comparison is on bit patterns.  The expected value of item i is that of
tests/periodic.py resp. tests/borders.py -- np.pad and the existing oracle --
on item i's slice alone; the items come from different seeds, so that a wrong
item stride cannot pass.

CPU: the plan entries against the unbatched ones, their refusals, the batched
wrap and extend modules compiled for gfx950 without scratch, what the feature
leaves untouched, the ABI.
GPU: the dense entry for batches of 1, 2 and 5, against an unbatched handle
item by item, at several refill intervals, the padded entry across calls,
fills, guard bands, a captured graph, refusals."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, soda_path
import asyncrun
import borders
import guarded
import periodic

SIZES = (1, 2, 4, 8)
MAX_BATCH = 65535
NEW = ['soda_hip_periodic_plan_batch', 'soda_hip_periodic_create_batch',
       'soda_hip_border_plan_batch', 'soda_hip_border_create_batch']


def _stencil(name, **kw):
  from soda_amd import core
  kw = {k: v for k, v in kw.items() if v is not None}
  return core.from_file(soda_path(name), **kw)


def _opts(**kw):
  from soda_amd.codegen.hip import lower
  kw.setdefault('peel', 0)
  return lower.LowerOptions(**kw)


def _plan(stencil, extent=None, **kw):
  """The launch plan of a program, lowered without trial compilations."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import lower
  opts = runtime.resolve_options(stencil, _opts(**kw), extent, probe=False)
  return runtime.make_plan(lower.lower(stencil, opts))


# ---------------------------------------------------------------------------
# CPU: the plan entries
# ---------------------------------------------------------------------------

PLANS = [
    ('jacobi2d.soda', dict(fuse=(4,)), (40, 7), 9),
    ('heat3d.soda', dict(fuse=(2,)), (32, 6, 5), 5),
]


@pytest.mark.parametrize('name,okw,extent,iterate', PLANS,
                         ids=[p[0].split('.')[0] for p in PLANS])
def test_plan_is_the_unbatched_plan_but_for_the_scratch(built, name, okw,
                                                        extent, iterate):
  """P, ghosts, k and chunks are what the unbatched entries give for the same
  program built without `batch`; scratch_bytes is that figure times the
  batch."""
  from soda_amd import runtime
  st = _stencil(name, iterate=iterate)
  one, many = _plan(st, **okw), _plan(st, batch=True, **okw)
  assert not one.batched and many.batched
  dim = st.dim
  for k in (0, 1, 2):
    lo, hi = runtime.periodic_ghosts(st, k or max(okw['fuse']))
    want, chunks = runtime.periodic_plan(one, extent, k, lo, hi, iterate)
    for batch in (1, 2, 5, MAX_BATCH):
      got, got_chunks = runtime.periodic_plan(many, extent, k, lo, hi, iterate,
                                              batch=batch)
      assert got_chunks == chunks
      assert got == dict(want, scratch_bytes=want['scratch_bytes'] * batch)
  if name == 'jacobi2d.soda':
    assert chunks == [2, 2, 2, 2, 1]
    lo, hi = runtime.periodic_ghosts(st, 4)
    assert runtime.periodic_plan(many, extent, 0, lo, hi, iterate,
                                 batch=3)[1] == [4, 4, 1]
  for modes in ('clamp', ('wrap', 'constant', 'mirror')[:dim], 'wrap'):
    lo, hi = runtime.periodic_ghosts(
        st, max(okw['fuse']) if modes == 'wrap' else 1)
    want, chunks = runtime.border_plan(one, extent, modes, lo, hi, iterate)
    for batch in (1, 3):
      got, got_chunks = runtime.border_plan(many, extent, modes, lo, hi,
                                            iterate, batch=batch)
      assert got_chunks == chunks
      assert got == dict(want, scratch_bytes=want['scratch_bytes'] * batch)
    if modes != 'wrap':
      assert chunks == [1] * iterate and want['refill_every'] == 1
  # the scratch: one padded array per input, two per output, per item
  cells = int(np.prod(want['padded']))
  assert want['scratch_bytes'] == 3 * 4 * cells


def test_plan_refusals_without_a_gpu(built):
  from soda_amd import runtime, util
  st = _stencil('jacobi2d.soda', iterate=9)
  one, many = _plan(st, fuse=(4,)), _plan(st, fuse=(4,), batch=True)
  per = lambda plan=many, batch=2, lo=(4, 4), hi=(4, 4), **kw: \
      runtime.periodic_plan(plan, (40, 7), 0, lo, hi, 9, batch=batch, **kw)
  bor = lambda plan=many, batch=2, lo=(1, 1), hi=(1, 1), **kw: \
      runtime.border_plan(plan, (40, 7), ('clamp', 'mirror'), lo, hi, 9,
                          batch=batch, **kw)
  assert per()[0]['padded'] == (48, 15) and bor()[0]['padded'] == (44, 9)
  for plan_fn in (per, bor):
    # the batch: 1..SODA_HIP_MAX_BATCH
    for batch in (0, -1, MAX_BATCH + 1):
      with pytest.raises(util.BackendError, match='invalid.*batch = '):
        plan_fn(batch=batch)
    assert plan_fn(batch=MAX_BATCH)[1]
    # a plan that is not batched: no loop in its place
    with pytest.raises(util.BackendError, match='invalid.*not batched'):
      plan_fn(plan=one)
    with pytest.raises(util.BackendError, match='invalid.*not batched'):
      plan_fn(plan=one, batch=1)
    # what the unbatched entries refuse
    with pytest.raises(util.BackendError, match='unsupported.*preserve'):
      plan_fn(preserve=True)
    with pytest.raises(util.BackendError, match='invalid.*last dimension'):
      plan_fn(lo=(4, 0))
    with pytest.raises(util.BackendError, match='invalid.*last dimension'):
      plan_fn(hi=(4, 0))
    with pytest.raises(util.BackendError, match='invalid'):
      plan_fn(lo=(-1, 4))
  with pytest.raises(util.BackendError, match='invalid.*mode'):
    runtime.border_plan(many, (40, 7), (1, 7), (1, 1), (1, 1), batch=2)
  with pytest.raises(util.BackendError, match='invalid.*refill'):
    bor(refill_every=2)
  # a plane above the 1 GiB window: per item, whatever the batch
  hplan = _plan(_stencil('heat3d.soda'), fuse=(2,), batch=True)
  with pytest.raises(util.BackendError, match='invalid'):
    runtime.border_plan(hplan, (32768, 16384, 4), 'clamp', (1, 1, 1),
                        (1, 1, 1), batch=2)
  # the unbatched entries still refuse a batched plan, and serve the other
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.periodic_plan(many, (40, 7), 0, (4, 4), (4, 4), 9)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.border_plan(many, (40, 7), 'clamp', (1, 1), (1, 1), 9)
  rl, rh, lo, hi = runtime.border_fused_ghosts(st, 'clamp', 4)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    runtime.border_fused_plan(many, (40, 7), 'clamp', 4, rl, rh, lo, hi, 9)
  assert runtime.periodic_plan(one, (40, 7), 0, (4, 4), (4, 4), 9)[1] == [
      4, 4, 1]


def test_null_arguments_are_refused_without_a_gpu(built):
  from soda_amd import runtime
  lib = runtime.library()
  for name in NEW:
    args = [0 if t is ctypes.c_int32 else None for t in runtime.API[name][1]]
    assert getattr(lib, name)(*args) == 1, name           # SODA_HIP_ERR_INVALID
    assert 'NULL argument' in runtime.last_error()


# ---------------------------------------------------------------------------
# CPU: the modules
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('dim', (1, 2, 3, 4))
def test_the_kernels_compile_without_scratch(built, dim):
  """The batched wrap and extend modules of every cell size and dimension
  count, for gfx950: one kernel each, no scratch, no LDS, plain C++ -- what
  the unbatched ones are held to."""
  from soda_amd import runtime, util
  from soda_amd.codegen.hip import extend, wrap
  for gen, resources, stem in ((wrap, runtime.wrap_resources, 'wrap'),
                               (extend, runtime.extend_resources, 'extend')):
    for elem in SIZES:
      _, res = resources(elem, dim, batch=True)
      name = gen.kernel_name(elem, dim, batch=True)
      assert name == 'soda_%s_e%d_d%d_bt' % (stem, elem, dim)
      assert sorted(res) == [name]
      assert res[name]['scratch'] == 0, res[name]
      assert res[name]['lds'] == 0 and 0 < res[name]['vgpr'] <= 64, res[name]
      text = gen.source(elem, dim, batch=True)
      own = text.split('soda_rt_%s.h' % stem, 1)[1]
      assert 'soda_rt_domain_batch.h' in own and 'blockIdx.z' in own
      assert 'asm' not in own and '__shared__' not in own
    with pytest.raises(util.SemanticError):
      gen.source(3, 2, batch=True)
    with pytest.raises(util.SemanticError):
      gen.source(4, 5, batch=True)


def test_existing_modules_are_untouched():
  """The unbatched wrap and extend modules are their runtime headers and one
  kernel line, with no word of the batch; the programs' modules are what they
  were; no LowerOptions field was added."""
  from soda_amd import runtime
  from soda_amd.codegen.hip import box, extend, lower, module, wrap
  fields = set(lower.LowerOptions.__dataclass_fields__)
  for elem in SIZES:
    for dim in (1, 2, 3, 4):
      batched = wrap.source(elem, dim, batch=True), \
          extend.source(elem, dim, batch=True)
      texts = {'wrap': wrap.source(elem, dim), 'extend': extend.source(elem, dim),
               'box': box.source(elem, dim)}
      assert texts['wrap'] == wrap.source(elem, dim, batch=False)
      assert texts['extend'] == extend.source(elem, dim, batch=False)
      for stem, text in texts.items():
        assert 'domain_batch' not in text and 'DOMAIN_BT' not in text
        assert '_bt' not in text and 'blockIdx.z' not in text, stem
      assert texts['wrap'].split('\n', 1)[1] == (
          module.runtime_text() + wrap.wrap_runtime_text() + '\n' +
          'SODA_WRAP_KERNEL(soda_wrap_e%d_d%d, uint%d_t, %d)\n' % (
              elem, dim, 8 * elem, dim))
      assert texts['extend'].split('\n', 1)[1] == (
          module.runtime_text() + extend.extend_runtime_text() + '\n' +
          'SODA_EXTEND_KERNEL(soda_extend_e%d_d%d, uint%d_t, %d)\n' % (
              elem, dim, 8 * elem, dim))
      # the batched text: the unbatched headers, the new one, another kernel
      assert batched[0].split('\n', 1)[1].startswith(
          module.runtime_text() + wrap.wrap_runtime_text())
      assert batched[1].split('\n', 1)[1].startswith(
          module.runtime_text() + extend.extend_runtime_text())
  for name, skw, okw in [('jacobi2d.soda', dict(iterate=13), dict(fuse=(4,))),
                         ('jacobi2d.soda', dict(iterate=13),
                          dict(fuse=(4,), batch=True)),
                         ('heat3d.soda', dict(iterate=4), dict(fuse=(2,))),
                         ('blur.soda', {}, dict(batch=True))]:
    stencil = _stencil(name, **skw)
    opts = runtime.resolve_options(stencil, _opts(**okw), None, probe=False)
    before = lower.lower(stencil, opts)
    wrap.source(4, stencil.dim, batch=True)
    extend.source(4, stencil.dim, batch=True)
    after = lower.lower(stencil, opts)
    assert before.source == after.source
    assert 'domain_batch' not in after.source and \
        'DOMAIN_BT' not in after.source and 'blockIdx.z' not in after.source
    assert bytes(runtime.make_plan(before)) == bytes(runtime.make_plan(after))
  assert set(lower.LowerOptions.__dataclass_fields__) == fields
  assert not any('domain' in f or 'wrap' in f or 'extend' in f or 'border' in f
                 for f in fields)


def test_abi_and_names(built):
  from soda_amd import runtime
  lib = runtime.library()
  assert lib.soda_hip_abi_version() == runtime.ABI_VERSION == 9
  assert lib.soda_hip_sizeof(15) == ctypes.sizeof(runtime.PeriodicDesc) == 60
  assert lib.soda_hip_sizeof(17) == ctypes.sizeof(runtime.BorderDesc) == 208
  header = open(os.path.join(ROOT, 'include', 'soda_hip.h')).read()
  for name in NEW:
    assert name in runtime.API and hasattr(lib, name), name
    assert name + '(' in header, name


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

BATCHES = (1, 2, 5)
# program name -> (stencil, LowerOptions keywords); all built with batch=True
PROGRAMS = {
    'jacobi2d': (lambda: _stencil('jacobi2d.soda', iterate=9),
                 dict(fuse=(4,))),
    'coupled2d': (lambda: _stencil('coupled2d.soda'), dict(fuse=(2,))),
    'heat3d': (lambda: _stencil('heat3d.soda', iterate=3), dict(fuse=(2,))),
    'blur': (lambda: _stencil('blur.soda'), {}),
    'ints2d': (lambda: _stencil('ints2d.soda'), {}),
    'heat4d': (lambda: _stencil('heat4d.soda', iterate=2),
               dict(strategy='direct')),
}
# case name -> (program, extent, iterate, modes -- None: a torus --, constants)
CASES = {
    'torus': ('jacobi2d', (40, 7), 9, None, None),          # chunks 4, 4, 1
    'clamp': ('jacobi2d', (40, 7), 9, 'clamp', None),
    'mirror101': ('jacobi2d', (40, 7), 9, 'mirror101', None),
    'wrap_constant': ('jacobi2d', (40, 7), 9, ('wrap', 'constant'), -3.5),
    # the ghosts of four iterations are wider than the domain
    'narrow_torus': ('jacobi2d', (12, 3), 9, None, None),
    # prod(N) is odd: dense items start off a 16-byte line
    'blur': ('blur', (37, 5), 1, ('mirror101', 'mirror'), None),
    'coupled2d': ('coupled2d', (32, 9), 3, 'constant', {'a': 1.5, 'b': -2.0}),
    'coupled2d_torus': ('coupled2d', (32, 9), 3, None, None),
    'heat3d': ('heat3d', (32, 6, 5), 3, ('mirror', 'clamp', 'wrap'), None),
    'heat3d_torus': ('heat3d', (32, 6, 5), 3, None, None),
    'heat4d': ('heat4d', (1, 1, 1, 1), 2, 'mirror101', None),
    'heat4d_torus': ('heat4d', (1, 1, 1, 1), 2, None, None),
    'ints2d': ('ints2d', (32, 6), 1, ('clamp', 'constant'), 201),
}

_PROGRAMS = {}
_EXPECTED = {}


@pytest.fixture(scope='module')
def programs(built):
  """Batched programs by name -- `name, False`: the same program built without
  `batch` --, made on first use, shared."""
  from soda_amd import runtime

  def get(name, batch=True):
    if (name, batch) not in _PROGRAMS:
      make, okw = PROGRAMS[name]
      _PROGRAMS[name, batch] = runtime.Program(make(),
                                               _opts(batch=batch, **okw))
    return _PROGRAMS[name, batch]
  yield get
  for prog in _PROGRAMS.values():
    prog.close()
  _PROGRAMS.clear()


def _want(stencil, ins, iterate, modes, cst):
  if modes is None:
    return periodic.expected(stencil, ins, iterate)
  return borders.expected(stencil, ins, iterate, modes, cst)


def _case(name, iterate=None, first=0):
  """(program name, stencil, extent, iterate, modes, constants, inputs,
  expected) for max(BATCHES) items, computed once: the input tensors and the
  expected outputs stacked [items, ...], item i from seed first + i alone; the
  param arrays are item 0's, shared."""
  key = (name, iterate, first)
  if key not in _EXPECTED:
    pname, extent, default, modes, cst = CASES[name]
    it = default if iterate is None else iterate
    stencil = PROGRAMS[pname][0]()
    items = [periodic.inputs(stencil, extent, first + i)
             for i in range(max(BATCHES))]
    params = {p.name: items[0][p.name] for p in stencil.param_stmts}
    wants = [_want(stencil, dict(item, **params), it, modes, cst)
             for item in items]
    ins = dict(params)
    for n in stencil.input_names:
      ins[n] = np.stack([item[n] for item in items])
      # a wrong item stride cannot pass: no two items are alike
      assert len({item[n].tobytes() for item in items}) == len(items) or \
          int(np.prod(extent)) == 1
    want = {o: np.stack([w[o] for w in wants]) for o in stencil.output_names}
    _EXPECTED[key] = (pname, stencil, extent, it, modes, cst, ins, want)
  return _EXPECTED[key]


def _first(arrays, stencil, batch):
  """The first `batch` items of the stacked tensors; param arrays whole."""
  params = {p.name for p in stencil.param_stmts}
  return {n: a if n in params else np.ascontiguousarray(a[:batch])
          for n, a in arrays.items()}


def _handle(prog, extent, modes, cst, batch, **kw):
  if modes is None:
    return prog.periodic(extent, batch=batch, **kw)
  return prog.bordered(extent, modes, cst, batch=batch, **kw)


def _dense(prog, dom, ins, iterate, stream=0):
  """The dense entry on device copies of `ins`; {output: array}."""
  st = prog.stencil
  shape = ins[st.input_names[0]].shape
  with periodic.Device(prog) as dev:
    d_in = [dev.upload(ins[n]) for n in st.input_names] + \
        [dev.upload(np.ascontiguousarray(ins[p.name]).reshape(-1))
         for p in st.param_stmts]
    d_out = [dev.alloc(int(np.prod(shape)) * np.dtype(t.np_name).itemsize)
             for t in st.output_types]
    dom.run_device(d_out, d_in, iterate, stream)
    return {n: dev.download(p, shape, np.dtype(t.np_name))
            for n, p, t in zip(st.output_names, d_out, st.output_types)}


def _assert_same(got, want, what):
  assert sorted(got) == sorted(want)
  for o in want:
    assert got[o].shape == want[o].shape, (what, o)
    per_item = [periodic.differing(g, w) for g, w in zip(got[o], want[o])] \
        if got[o].ndim > 1 else None
    assert periodic.same_bits(got[o], want[o]), \
        '%s: %d cells of %s differ in their bits (per item: %s)' % (
            what, periodic.differing(got[o], want[o]), o, per_item)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_dense_entry_against_the_padded_oracle(programs, name):
  """Batches of 1, 2 and 5: every cell of every item is what the oracle gives
  for that item alone, and the handle holds the scratch of one item times the
  batch."""
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  assert all(np.isfinite(w).all() for w in want.values() if w.dtype.kind == 'f')
  prog = programs(pname)
  assert prog.plan.batched == 1
  one_item = None
  for batch in BATCHES:
    with _handle(prog, extent, modes, cst, batch) as dom:
      info = dom.info()
      got = _dense(prog, dom, _first(ins, stencil, batch), iterate)
    _assert_same(got, _first(want, stencil, batch), '%s x %d' % (name, batch))
    one_item = one_item or info
    assert info == dict(one_item,
                        scratch_bytes=one_item['scratch_bytes'] * batch)
  if modes is not None and set(borders.per_dim(modes, stencil.dim)) != {'wrap'}:
    assert info['refill_every'] == 1
  if name == 'torus':
    assert info['refill_every'] == 4
  if name == 'narrow_torus':
    assert info['ghost_lo'][1] > extent[1] and info['ghost_hi'][1] > extent[1]
  if name == 'blur':
    assert int(np.prod(extent)) % 8          # items off the 16-byte lines
  # numpy in, numpy out
  if name in ('torus', 'coupled2d_torus'):
    _assert_same(prog.run_periodic_batch(_first(ins, stencil, 2), iterate),
                 _first(want, stencil, 2), 'run_periodic_batch')
  if name in ('wrap_constant', 'coupled2d', 'blur'):
    _assert_same(prog.run_bordered_batch(_first(ins, stencil, 2), modes, cst,
                                         iterate),
                 _first(want, stencil, 2), 'run_bordered_batch')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['torus', 'clamp', 'blur', 'heat3d'])
def test_every_item_is_the_unbatched_handle_on_it_alone(programs, name):
  """The parent's way -- the program built without `batch`, one handle, one
  call per item -- gives the same bits."""
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  batch = 3
  prog, alone = programs(pname), programs(pname, False)
  assert not alone.plan.batched
  with _handle(prog, extent, modes, cst, batch) as dom:
    got = _dense(prog, dom, _first(ins, stencil, batch), iterate)
  with _handle(alone, extent, modes, cst, None) as dom:
    for i in range(batch):
      item = {n: a[i] if n in stencil.input_names else a
              for n, a in ins.items()}
      mine = _dense(alone, dom, item, iterate)
      _assert_same({o: got[o][i] for o in got}, mine, '%s, item %d' % (name, i))
  _assert_same(got, _first(want, stencil, batch), name)


@pytest.mark.gpu
def test_refill_every_does_not_change_a_bit(programs):
  pname, stencil, extent, iterate, _, _, ins, want = _case('torus')
  prog = programs(pname)
  for k in (1, 2, 3, 4):
    with prog.periodic(extent, refill_every=k, batch=3) as per:
      assert per.info()['refill_every'] == k
      got = _dense(prog, per, _first(ins, stencil, 3), iterate)
    _assert_same(got, _first(want, stencil, 3), 'refill_every=%d' % k)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['torus', 'clamp', 'wrap_constant'])
def test_padded_entry_across_calls(programs, name):
  """Two run_padded calls of 4 and 5 iterations on device-resident padded
  state equal one run of 9; every item leaves wrapped or extended; the inputs
  are byte-identical afterwards."""
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  batch = 3
  after4 = _first(_case(name, iterate=4)[7], stencil, batch)
  prog = programs(pname)
  extended = lambda arr, lo, hi: periodic.wrap_pad(arr, lo, hi) \
      if modes is None else borders.pad(arr, lo, hi, modes, cst or 0)
  with _handle(prog, extent, modes, cst, batch) as dom, \
      periodic.Device(prog) as dev:
    info = dom.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    start = np.stack([extended(a, lo, hi) for a in ins['t1'][:batch]])
    assert start.shape == (batch,) + info['padded'][::-1]
    d0, d1, d2 = dev.upload(start), dev.alloc(start.nbytes), \
        dev.alloc(start.nbytes)
    dom.run_padded([d1], [d0], 4)
    dom.run_padded([d2], [d1], 5)
    mid = dev.download(d1, start.shape, start.dtype)
    end = dev.download(d2, start.shape, start.dtype)
    assert periodic.same_bits(dev.download(d0, start.shape, start.dtype),
                              start)
  inner = lambda arr: np.stack([periodic.interior(a, info) for a in arr])
  _assert_same({'t0': inner(mid)}, after4, 'padded 4')
  _assert_same({'t0': inner(end)}, _first(want, stencil, batch),
               'padded 4 + 5')
  for arr in (mid, end):                     # the ghosts of every item: current
    form = np.stack([extended(periodic.interior(a, info), lo, hi)
                     for a in arr])
    assert periodic.same_bits(arr, form), periodic.differing(arr, form)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['torus', 'clamp', 'wrap_constant',
                                  'narrow_torus', 'blur', 'heat3d', 'heat4d'])
def test_fill_writes_ghost_cells_only(programs, name):
  """A planted pattern of [3, P]: in every item the interior keeps every byte
  and every ghost cell takes what the item's own interior gives -- at an
  address that is aligned to the cell only."""
  pname, stencil, extent, _, modes, cst, _, _ = _case(name)
  prog = programs(pname)
  batch = 3
  dtype = np.dtype(stencil.output_types[0].np_name)
  cst = borders.constants_of(stencil, cst)[stencil.input_names[0]]
  with _handle(prog, extent, modes, cst, batch) as dom, \
      periodic.Device(prog) as dev:
    info = dom.info()
    lo, hi = info['ghost_lo'], info['ghost_hi']
    shape = (batch,) + info['padded'][::-1]
    cells_n = int(np.prod(shape))
    rng = np.random.default_rng(11)
    for lead in (0, 1, 3):                       # cells behind a 16-byte line
      raw = rng.integers(0, 256, size=(lead + cells_n + 5) * dtype.itemsize,
                         dtype=np.uint8)
      base = dev.upload(raw)
      dom.fill([base + lead * dtype.itemsize])
      back = dev.download(base, raw.shape, np.uint8)
      cells = lambda b: b[lead * dtype.itemsize:
                          (lead + cells_n) * dtype.itemsize].view(
                              dtype).reshape(shape)
      before, after = cells(raw), cells(back)
      for i in range(batch):
        assert periodic.same_bits(periodic.interior(after[i], info),
                                  periodic.interior(before[i], info)), i
        inner = periodic.interior(before[i], info)
        form = periodic.wrap_pad(inner, lo, hi) if modes is None else \
            borders.closed_form(inner, lo, hi, modes, cst)
        assert periodic.same_bits(after[i], form), (
            i, periodic.differing(after[i], form))
      # no byte in front of or behind the arrays
      n = lead * dtype.itemsize
      assert (back[:n] == raw[:n]).all()
      assert (back[-5 * dtype.itemsize:] == raw[-5 * dtype.itemsize:]).all()


class _DenseEntry:
  """The dense entry with run_device's call shape, for tests/guarded.py."""

  def __init__(self, prog, dom):
    self.device, self.dom = prog.device, dom

  def run_device(self, outputs, inputs, extent, iterate=None, **kw):
    self.dom.run_device(outputs, inputs, iterate, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['torus', 'wrap_constant', 'coupled2d',
                                  'heat3d', 'blur'])
def test_dense_entry_between_guard_bands(programs, name):
  """The [batch, ...] arrays in one arena between guards: the inputs and the
  param arrays keep every byte, no byte outside the outputs changes."""
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  prog = programs(pname)
  batch = 3
  with _handle(prog, extent, modes, cst, batch) as dom:
    # (the arena's tensors: the items are its slowest axis)
    got, violation, _ = guarded.run(_DenseEntry(prog, dom), stencil,
                                    tuple(extent) + (batch,),
                                    _first(ins, stencil, batch), iterate)
  assert violation is None, violation
  _assert_same(got, _first(want, stencil, batch), name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['mirror101', 'heat3d_torus'])
def test_dense_entry_captured_and_replayed(programs, name):
  """One capture of run_device on a single stream, after an eager call: the
  replay equals the eager result, on changed inputs too; nothing grows."""
  import torch
  pname, stencil, extent, iterate, modes, cst, ins, want = _case(name)
  batch = 2
  ins2, want2 = _case(name, first=7)[6:]
  ins, want, ins2, want2 = [_first(a, stencil, batch)
                            for a in (ins, want, ins2, want2)]
  prog = programs(pname)
  i_name, o_name = stencil.input_names[0], stencil.output_names[0]
  S = torch.cuda.Stream()
  with _handle(prog, extent, modes, cst, batch) as dom:
    t_in = asyncrun._bytes(ins[i_name])
    t_out = asyncrun._bytes(asyncrun.poison_like(want[o_name]))
    read = lambda: t_out.cpu().numpy().view(np.float32).reshape(
        want[o_name].shape)
    call = lambda: dom.run_device([t_out.data_ptr()], [t_in.data_ptr()],
                                  iterate, stream=S.cuda_stream)
    torch.cuda.synchronize()
    call()                                        # eager: sizes the scratch
    S.synchronize()
    _assert_same({o_name: read()}, want, name + ', eager')
    warm, held = prog.scratch(), dom.info()['scratch_bytes']
    t_out.copy_(asyncrun._bytes(asyncrun.poison_like(want[o_name])))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
      call()
    assert np.isnan(read()).all()                 # capture records only
    g.replay()
    torch.cuda.synchronize()
    _assert_same({o_name: read()}, want, name + ', replay')
    t_in.copy_(asyncrun._bytes(ins2[i_name]))     # changed inputs
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_same({o_name: read()}, want2, name + ', replay on new inputs')
    assert prog.scratch() == warm and dom.info()['scratch_bytes'] == held
    del g


@pytest.mark.gpu
def test_refusals_launch_nothing_and_allocate_nothing(programs, built):
  from soda_amd import runtime, util
  pname, stencil, extent, iterate, modes, cst, ins, want = _case('clamp')
  prog, alone = programs(pname), programs(pname, False)
  # a program that is not batched: no loop of launches in its place
  with alone.bordered(extent, modes) as bor:
    _dense(alone, bor, {'t1': ins['t1'][0]}, iterate)
  before = alone.last_launches(), alone.scratch()
  for make in (lambda: alone.bordered(extent, modes, batch=2),
               lambda: alone.periodic(extent, batch=2),
               lambda: alone.bordered(extent, modes, batch=1)):
    with pytest.raises(util.BackendError, match='invalid.*not batched'):
      make()
  with pytest.raises(util.BackendError, match='invalid.*not batched'):
    alone.run_bordered_batch(_first(ins, stencil, 2), modes)
  with pytest.raises(util.BackendError, match='invalid.*not batched'):
    alone.run_periodic_batch(_first(ins, stencil, 2))
  assert (alone.last_launches(), alone.scratch()) == before
  assert alone._periodic == []
  # the batched program
  with prog.bordered(extent, modes, batch=2) as bor:
    got = _dense(prog, bor, _first(ins, stencil, 2), iterate)
  _assert_same(got, _first(want, stencil, 2), 'clamp x 2')
  before = prog.last_launches(), prog.scratch()
  # a batch out of range
  for batch in (0, -3, MAX_BATCH + 1):
    with pytest.raises(util.BackendError, match='invalid.*batch = '):
      prog.bordered(extent, modes, batch=batch)
    with pytest.raises(util.BackendError, match='invalid.*batch = '):
      prog.periodic(extent, batch=batch)
  # the unbatched entries and the fused handle keep refusing a batched plan
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    prog.bordered(extent, modes)
  with pytest.raises(util.BackendError, match='unsupported.*batched'):
    prog.periodic(extent)
  for depth in (0, 4):
    with pytest.raises(util.BackendError, match='unsupported.*batched'):
      prog.bordered(extent, modes, depth=depth, batch=2)
  with pytest.raises(util.InputError, match='shape'):
    prog.run_bordered_batch({'t1': ins['t1'][0]}, modes)
  assert (prog.last_launches(), prog.scratch()) == before
  assert prog._periodic == []
  # residual, norms and until on a batched handle: no byte written
  batch = 2
  for handle_of in (lambda: prog.bordered(extent, modes, batch=batch),
                    lambda: prog.periodic(extent, batch=batch)):
    with handle_of() as dom, periodic.Device(prog) as dev:
      info = dom.info()
      shape = (batch,) + info['padded'][::-1]
      planted = np.full(shape, 0xA5A5A5A5, np.uint32)
      p_out, p_in = dev.upload(planted), dev.upload(np.zeros(shape, np.float32))
      dense = np.full((batch,) + extent[::-1], 0xA5A5A5A5, np.uint32)
      d_out, d_in = dev.upload(dense), dev.upload(ins['t1'][:batch])
      acc = dev.upload(np.zeros(64, np.uint8))
      held = prog.last_launches(), prog.scratch(), info['scratch_bytes']
      with pytest.raises(util.BackendError, match='unsupported.*batched'):
        dom.run_padded([p_out], [p_in], 1, residual=acc)
      with pytest.raises(util.BackendError, match='unsupported.*batched'):
        dom.run_padded([p_out], [p_in], 1, norms=acc)
      with pytest.raises(util.BackendError, match='unsupported.*batched'):
        dom.run_until([d_out], [d_in], 1e-3, 8)
      with pytest.raises(util.BackendError, match='unsupported.*batched'):
        dom.run_until([d_out], [d_in], 1e-3, 8, norm='l2')
      # the contract holds on the whole arrays: item 1 of the output is an
      # input
      with pytest.raises(util.BackendError, match='overlaps an input'):
        dom.run_padded([p_out], [p_out + planted.nbytes // batch], 1)
      assert periodic.same_bits(dev.download(p_out, shape, np.uint32), planted)
      assert periodic.same_bits(
          dev.download(d_out, dense.shape, np.uint32), dense)
      assert (prog.last_launches(), prog.scratch(),
              dom.info()['scratch_bytes']) == held
