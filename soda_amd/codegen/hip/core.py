"""The HIP backend's plug-in surface: `add_arguments` + `print_code`.

Every backend of the reference is a module with exactly these two functions,
registered and invoked by the driver (reference src/soda/sodac.py:99-102,
198-200; src/soda/codegen/frt/core.py:10-27; src/soda/codegen/xilinx/
opencl.py:55-142).  This module slots into the same place:

  --hip-kernel FILE   print the generated HIP source ('-' = stdout), the
                      counterpart of --xocl-kernel;
  --hip-host FILE     print the C++ host: soda::app::<app>() with the reference's
                      --frt-host signature, on libsoda_hip.so (host.py);
  --hip-backend       JIT-build the kernels for gfx950 and RUN the program on
                      the GPU with the reference harness's inputs, checking
                      nothing by itself (the oracle lives in tests/); prints
                      one JSON line with timing.  --hip-periodic: on a torus.
                      --hip-border MODE[,MODE...]: with a border mode per
                      dimension, LOW/HIGH for one per face;
                      --hip-border-values V[/V][,V[/V]...]: the constants per
                      dimension and side; --hip-border-depth T: fused away
                      from the walls.
"""
import argparse
import json
import shutil
import sys
import tempfile
import time

from soda_amd import core, util
from soda_amd.codegen.hip import lower


def parse_border(text: str, dim: int):
  """--hip-border's MODE[,MODE...]: one name, or a list with one entry per
  dimension (one for all), an entry LOW/HIGH a pair of names."""
  entries = [m.strip() for m in text.split(',')]
  entries = [tuple(f.strip() for f in m.split('/')) if '/' in m else m
             for m in entries]
  if len(entries) == 1:
    return entries[0] if isinstance(entries[0], str) else entries * dim
  return entries


def parse_border_values(text: str, dim: int):
  """--hip-border-values' V[/V][,V[/V]...]: one entry per dimension (one for
  all), an entry LOW/HIGH a pair of values."""
  try:
    entries = [tuple(float(v) for v in e.split('/')) if '/' in e else float(e)
               for e in text.split(',')]
  except ValueError:
    raise util.InputError('--hip-border-values: numbers, V or LOW/HIGH per '
                          'dimension')
  return entries * dim if len(entries) == 1 else entries


def add_arguments(parser) -> None:
  parser.add_argument('--hip-kernel', type=str, dest='hip_kernel',
                      metavar='file', help='HIP kernel code for gfx950')
  parser.add_argument('--hip-host', type=str, dest='hip_host', metavar='file',
                      help='C++ host: soda::app::<app>() with the signature '
                      'of --frt-host, on libsoda_hip.so')
  parser.add_argument('--hip-wire-kernel', type=str, dest='hip_wire_kernel',
                      metavar='file', help='C++ definition of extern "C" '
                      '<app>_kernel(banks..., coalesced_data_num) -- the '
                      "reference kernel's ABI on its tiled, banked streams -- "
                      'on libsoda_hip.so: links under the unmodified '
                      '--frt-host output built with -DSODA_CPP_BINDING')
  parser.add_argument('--hip-backend', action='store_true', dest='hip_backend',
                      help='JIT-build the HIP kernels and run them on the GPU')
  parser.add_argument('--hip-strategy', type=str, dest='hip_strategy',
                      choices=lower.STRATEGIES, default='auto',
                      help='kernel family: register-marching wavefront strips '
                      '(2-D / 3-D programs), the LDS window ring (2-D), the '
                      'direct kernels, or tile3d: LDS-tiled 3-D kernels that '
                      'fuse every depth of --hip-fuse (never picked by auto)')
  parser.add_argument('--hip-fuse', type=int, nargs='*', dest='hip_fuse',
                      metavar='T', default=list(lower.DEFAULT_FUSE),
                      help='temporal blocking: the numbers of iterations a '
                      'launch may fuse; the library mixes them per extent '
                      '(default: %s; depths that do not fit the registers ' %
                      ' '.join(map(str, lower.DEFAULT_FUSE)) +
                      'are dropped, 3-D programs fuse at most 2 unless '
                      '--hip-strategy tile3d)')
  parser.add_argument('--hip-vec', type=int, dest='hip_vec', metavar='V',
                      help='cells per lane per row (default: 16 bytes worth)')
  parser.add_argument('--hip-chunk-rows', type=int, dest='hip_chunk_rows',
                      default=None, help='rows one wavefront marches over '
                      '(default: sized at load time so the grid fills the GPU '
                      'in one round of waves)')
  parser.add_argument('--hip-prefetch', type=int, dest='hip_prefetch',
                      default=None, help='input rows loaded ahead of use')
  parser.add_argument('--hip-tile-rows', type=int, dest='hip_tile_rows',
                      default=None, help='3-D: output rows held per wavefront')
  parser.add_argument('--hip-extent', type=int, nargs='+', dest='hip_extent',
                      metavar='N', help='grid size for --hip-backend')
  parser.add_argument('--hip-waves', type=str, dest='hip_waves', default='1x1',
                      metavar='XxY', help='wavefronts per block along '
                      'dimension 0 and 1')
  parser.add_argument('--hip-pipe', type=int, dest='hip_pipe', default=None,
                      metavar='W', help='split the fused iterations of a 2-D '
                      'kernel over W wavefronts of a block (rows handed on '
                      'through LDS); the fusion depth must be a multiple '
                      '(default 1)')
  parser.add_argument('--hip-xshare-block', type=int, dest='hip_xshare_block',
                      default=None, metavar='B', help='fused kernels on blocks '
                      'of B wavefronts (2..16) side by side on a segment of '
                      'the row, x-halos shared through LDS inside the block: '
                      'any row length, none needed at build time (default: '
                      'not used)')
  parser.add_argument('--hip-batch', action='store_true', dest='hip_batch',
                      help='batched kernels (names end in _bt): a launch runs '
                      'many independent grids of one extent, blockIdx.y is '
                      'the item (soda_hip_run_device_batch)')
  parser.add_argument('--hip-residual', action='store_true',
                      dest='hip_residual',
                      help='residual kernels: twins of the marching kernels '
                      '(names end in _rs) and <app>_residual, which report how '
                      'much the last iteration of a run changed the grid '
                      '(soda_hip_run_device_residual / _until)')
  parser.add_argument('--hip-until', type=float, dest='hip_until',
                      default=None, metavar='TOL',
                      help='--hip-backend: iterate until the largest change of '
                      'a cell in one iteration is <= TOL (at most `iterate` '
                      'iterations); implies --hip-residual; prints the '
                      'iterations and the residual; with --hip-gpus N on the '
                      'slabs (soda_hip_group_run_until)')
  parser.add_argument('--hip-norm', choices=('max', 'l1', 'l2'),
                      dest='hip_norm', default='max',
                      help='with --hip-until: what TOL bounds -- the largest '
                      'change of a cell (max, the default), or the exact sum '
                      'of |change| (l1) or root of the sum of squares (l2) '
                      'over the grid (soda_hip_run_device_until_norm; one GPU)')
  parser.add_argument('--hip-check-every', type=int, dest='hip_check_every',
                      default=8, metavar='K',
                      help='with --hip-until: iterations between two looks at '
                      'the residual (default 8)')
  parser.add_argument('--hip-periodic', action='store_true',
                      dest='hip_periodic',
                      help='--hip-backend: run on a torus -- cell N is cell 0 '
                      'in every dimension, every cell of the outputs is '
                      'defined; the ghost frame is refilled on the GPU '
                      '(soda_hip_periodic_run_device; one GPU, no --hip-until)')
  parser.add_argument('--hip-refill-every', type=int, dest='hip_refill_every',
                      default=None, metavar='K',
                      help='with --hip-periodic: iterations between two '
                      'refills of the ghost frame (default: the deepest '
                      'fusion depth)')
  parser.add_argument('--hip-border', dest='hip_border', default=None,
                      metavar='MODE[,MODE...]',
                      help='--hip-backend: run with borders -- every iteration '
                      'sees its inputs extended by wrap, clamp, mirror, '
                      'mirror101 or constant (one mode for all dimensions or '
                      'one per dimension, dimension 0 first; LOW/HIGH in any '
                      'position gives the two faces of a dimension a mode '
                      'each), every cell of '
                      'the outputs is defined (soda_hip_border_run_device; one '
                      'GPU, no --hip-until, no --hip-periodic)')
  parser.add_argument('--hip-border-value', type=float,
                      dest='hip_border_value', default=0.0, metavar='V',
                      help='with --hip-border: the value outside the grid in a '
                      '`constant` dimension (default 0)')
  parser.add_argument('--hip-border-values', dest='hip_border_values',
                      default=None, metavar='V[/V][,V[/V]...]',
                      help='with --hip-border: the values outside the grid per '
                      'dimension, dimension 0 first, LOW/HIGH for one per '
                      'face (one entry for all dimensions or one per '
                      'dimension; one list for all inputs; instead of '
                      '--hip-border-value: a value other than 0 there is '
                      'refused beside this option)')
  parser.add_argument('--hip-border-depth', type=int,
                      dest='hip_border_depth', default=None, metavar='T',
                      help='with --hip-border: fuse away from the walls in '
                      'chunks of T iterations, 0 for the deepest fusion depth '
                      '(soda_hip_border_fused_run_device; the same bits; '
                      'default 1: one iteration per launch)')
  parser.add_argument('--hip-nt-store', action='store_true',
                      dest='hip_nt_store',
                      help='non-temporal instead of plain output stores')
  parser.add_argument('--hip-no-nt-load', action='store_true',
                      dest='hip_no_nt_load',
                      help='plain instead of non-temporal input loads')
  parser.add_argument('--hip-no-xcd-swizzle', action='store_true',
                      dest='hip_no_xcd_swizzle',
                      help='do not remap blocks so neighbours share an XCD')
  parser.add_argument('--hip-device', type=int, dest='hip_device', default=0)
  parser.add_argument('--hip-no-probe', action='store_true',
                      dest='hip_no_probe',
                      help='--hip-kernel / --hip-host: do not size the peeled '
                      'warm-up by trial compilations (needs libsoda_hip.so + '
                      'hiprtc); the emitted text is then the same on every '
                      'box and toolchain')
  parser.add_argument('--hip-gpus', type=int, dest='hip_gpus', default=1,
                      metavar='N', help='--hip-backend / --hip-host: cut the '
                      'grid into N slabs along the streamed dimension, one '
                      'per GPU, halo exchange by peer copies '
                      '(soda_hip_group_*)')
  parser.add_argument('--hip-exchange-every', type=int, default=0,
                      dest='hip_exchange_every', metavar='K',
                      help='with --hip-gpus N: iterations between halo '
                      'exchanges (default 0: the library picks)')
  parser.add_argument('--hip-virtual', action='store_true', dest='hip_virtual',
                      help='with --hip-gpus N: all N slabs on --hip-device '
                      '(the whole schedule on one GPU)')


def options_from_args(args: argparse.Namespace) -> lower.LowerOptions:
  wx, wy = (int(v) for v in args.hip_waves.lower().split('x'))
  return lower.LowerOptions(strategy=args.hip_strategy,
                            fuse=tuple(args.hip_fuse or ()),
                            vec=args.hip_vec,
                            chunk_rows=args.hip_chunk_rows,
                            prefetch=args.hip_prefetch, waves_x=wx, waves_y=wy,
                            nt_store=True if args.hip_nt_store else None,
                            nt_load=False if args.hip_no_nt_load else None,
                            tile_rows=args.hip_tile_rows,
                            xcd_swizzle=not args.hip_no_xcd_swizzle,
                            pipe=args.hip_pipe,
                            xshare_block=args.hip_xshare_block,
                            batch=bool(getattr(args, 'hip_batch', False)),
                            residual=bool(
                                getattr(args, 'hip_residual', False) or
                                getattr(args, 'hip_until', None) is not None))


def print_code(stencil: core.Stencil, args: argparse.Namespace) -> None:
  if not isinstance(stencil, core.Stencil):
    # called from the reference's own driver with ITS Stencil (expression tree
    # in the un-vendored haoda): both print the same DSL normal form
    # (reference src/soda/core.py:157-166, src/tests/test_grammar.py:24-61), so
    # re-read it
    stencil = core.from_text(str(stencil))
  if args.hip_kernel is not None:
    from soda_amd import runtime
    opts = runtime.resolve_options(stencil, options_from_args(args), None,
                                   probe=not getattr(args, 'hip_no_probe',
                                                     False))
    with tempfile.TemporaryFile(mode='w+') as tmp:
      tmp.write(lower.lower(stencil, opts).source)
      tmp.seek(0)
      if args.hip_kernel == '-':
        shutil.copyfileobj(tmp, sys.stdout)
      else:
        with open(args.hip_kernel, 'w') as f:
          shutil.copyfileobj(tmp, f)
  if getattr(args, 'hip_host', None) is not None:
    from soda_amd.codegen.hip import host
    text = host.print_host(stencil, options_from_args(args), args.hip_extent,
                           gpus=max(1, int(getattr(args, 'hip_gpus', 1) or 1)),
                           probe=not getattr(args, 'hip_no_probe', False))
    if args.hip_host == '-':
      sys.stdout.write(text)
    else:
      with open(args.hip_host, 'w') as f:
        f.write(text)
  if getattr(args, 'hip_wire_kernel', None) is not None:
    from soda_amd.codegen.hip import wire
    text = wire.print_wire_kernel(stencil)
    if args.hip_wire_kernel == '-':
      sys.stdout.write(text)
    else:
      with open(args.hip_wire_kernel, 'w') as f:
        f.write(text)
  if args.hip_backend:
    run(stencil, args)


def default_extent(stencil: core.Stencil):
  """The reference harness's default problem size: tile sizes, and one more
  than the stencil's height in the streamed dimension (frt/host.py:454-461)."""
  dims = list(stencil.tile_size[:-1])
  dims.append(stencil.stencil_dim[-1] + 1)
  return dims


def run(stencil: core.Stencil, args: argparse.Namespace) -> None:
  import numpy as np
  from soda_amd import runtime
  extent = list(args.hip_extent or default_extent(stencil))
  if len(extent) != stencil.dim:
    raise util.InputError('--hip-extent needs %d values' % stencil.dim)
  shape = tuple(extent[::-1])
  rng = np.random.default_rng(0)
  inputs = {}
  for name, t in zip(stencil.input_names, stencil.input_types):
    if t.is_float:
      inputs[name] = rng.random(shape, dtype=np.float64).astype(t.np_name)
    else:  # p + q (+ r): the reference harness's integer init
      grids = np.indices(shape).sum(axis=0)
      inputs[name] = grids.astype(t.np_name)
  for pstmt in stencil.param_stmts:
    # the reference harness's param init: the sum of the indices
    # (frt/host.py:530-541)
    size = pstmt.size or (1,)
    inputs[pstmt.name] = np.indices(size).sum(axis=0).astype(
        pstmt.haoda_type.np_name)
  gpus = max(1, int(getattr(args, 'hip_gpus', 1) or 1))
  extra = {}
  periodic = bool(getattr(args, 'hip_periodic', False))
  if periodic and (gpus > 1 or getattr(args, 'hip_until', None) is not None
                   or getattr(args, 'hip_residual', False)):
    raise util.InputError('--hip-periodic runs on one GPU, without --hip-until '
                          'or --hip-residual (slabs, groups and residuals are '
                          'not served on a torus yet)')
  border = getattr(args, 'hip_border', None)
  if border is not None and (
      periodic or gpus > 1 or getattr(args, 'hip_until', None) is not None
      or getattr(args, 'hip_residual', False)):
    raise util.InputError('--hip-border runs on one GPU, without --hip-periodic, '
                          '--hip-until or --hip-residual (slabs, groups and '
                          'residuals are not served on a bordered domain yet)')
  if border is None and getattr(args, 'hip_border_depth', None) is not None:
    raise util.InputError('--hip-border-depth needs --hip-border')
  border_values = getattr(args, 'hip_border_values', None)
  if border is None and border_values is not None:
    raise util.InputError('--hip-border-values needs --hip-border')
  if border_values is not None and getattr(args, 'hip_border_value', 0.0):
    raise util.InputError('--hip-border-value or --hip-border-values, not '
                          'both')
  if border is not None:
    border = parse_border(border, stencil.dim)
    if isinstance(border, str):
      border = [border] * stencil.dim
    runtime._border_faces(border, stencil.dim)     # an InputError, before any
                                                   # kernel is built
    border_values = getattr(args, 'hip_border_value', 0.0) \
        if border_values is None else parse_border_values(border_values,
                                                          stencil.dim)
  if gpus > 1:
    # one host thread, N GPUs: slabs along the streamed dimension
    devices = ([args.hip_device] * gpus if getattr(args, 'hip_virtual', False)
               else list(range(gpus)))
    prog = runtime.Group(stencil, extent, devices, options_from_args(args),
                         exchange_every=int(getattr(args, 'hip_exchange_every',
                                                    0) or 0))
    t0 = time.time()
    res = None
    if getattr(args, 'hip_norm', 'max') != 'max':
      raise util.InputError('--hip-norm l1 / l2 runs on one GPU (the slabs\' '
                            'norms are not served yet)')
    if getattr(args, 'hip_until', None) is not None:
      # the one-GPU form's loop on the slabs (soda_hip_group_run_until)
      prog.load(inputs)
      done, res = prog.run_until(
          args.hip_until, stencil.iterate,
          check_every=max(1, int(args.hip_check_every)))
      outputs = prog.store(done)
      extra = {'until': args.hip_until, 'iterations': done}
    elif getattr(args, 'hip_residual', False):
      prog.load(inputs)
      prog.run(residual=True)
      res = prog.residual()
      outputs = prog.store()
    else:
      outputs = prog.run_host(inputs)
    seconds = time.time() - t0
    st = prog.stats()
    if res is not None:
      extra['residual'] = {'changed': res.changed, 'unordered': res.unordered,
                           'max_float': res.max_float, 'max_int': res.max_int}
    extra.update({'gpus': gpus, 'devices': devices,
                  'exchange_every': st['exchange_every'],
                  'exchanges': st['exchanges'],
                  'split_passes': st['split_passes']})
  else:
    prog = runtime.Program(stencil, options_from_args(args),
                           device=args.hip_device, extent=extent)
    t0 = time.time()
    norm = getattr(args, 'hip_norm', 'max')
    if getattr(args, 'hip_until', None) is not None and norm != 'max':
      outputs, done, acc = prog.run_until(
          inputs, args.hip_until, stencil.iterate,
          check_every=max(1, int(args.hip_check_every)), norm=norm)
      extra = {'until': args.hip_until, 'norm': norm, 'iterations': done,
               'norms': {'count': int(acc.count),
                         'unordered': int(acc.unordered),
                         'infinite': int(acc.infinite),
                         'l1': runtime.norms_value(acc, 'l1'),
                         'l2_squared': runtime.norms_value(acc, 'l2')}}
    elif getattr(args, 'hip_until', None) is not None:
      outputs, done, res = prog.run_until(
          inputs, args.hip_until, stencil.iterate,
          check_every=max(1, int(args.hip_check_every)))
      extra = {'until': args.hip_until, 'iterations': done,
               'residual': {'changed': res.changed, 'unordered': res.unordered,
                            'max_float': res.max_float,
                            'max_int': res.max_int}}
    elif periodic:
      k = getattr(args, 'hip_refill_every', None)
      outputs = prog.run_periodic(inputs, refill_every=k)
      extra = {'periodic': True, 'refill_every': k or max(
          p.fused_iters for p in prog.module.passes)}
    elif border is not None:
      depth = getattr(args, 'hip_border_depth', None)
      outputs = prog.run_bordered(inputs, border, border_values,
                                  depth=1 if depth is None else depth)
      extra = {'border': border, 'border_depth': 1 if depth is None else depth}
    else:
      outputs = prog.run(inputs)
    seconds = time.time() - t0
  cells = float(np.prod(extent)) * stencil.iterate
  print(json.dumps({
      'kernel': stencil.app_name, 'extent': extent,
      'iterate': stencil.iterate, 'seconds_incl_copies': seconds,
      'cells_iters_per_s_incl_copies': cells / seconds, **extra,
      'kernels': [k.name for k in prog.module.kernels],
      'checksum': {n: float(np.asarray(v, dtype=np.float64).sum())
                   for n, v in outputs.items()},
  }))
