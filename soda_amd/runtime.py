"""ctypes binding of libsoda_hip.so and the JIT driver on top of it.

The Python side of the drop-in boundary (include/soda_hip.h).  The reference's
host reaches its kernel either linked directly or through the FRT runtime
(`fpga::Instance(bitstream)`, SetArg/WriteToDevice/Exec/ReadFromDevice/Finish;
reference src/soda/codegen/frt/host.py:97-113,288-322).  `Program` is that
object for a GPU: built from HIP source text instead of a bitstream, it owns
the loaded code object and runs it on host or device arrays.

There is no CPU fallback: a missing library, a failed JIT or a missing GPU
raises `util.BackendError`.
"""
import contextlib
import ctypes
import dataclasses
import functools
import hashlib
import os
import sys
from typing import Dict, Optional, Sequence

from soda_amd import core, util
from soda_amd.codegen.hip import lower

_HERE = os.path.dirname(os.path.abspath(__file__))
# SODA_HIP_LIBRARY: another build of the same sources -- the sanitizer builds
# of `make -C soda_amd/csrc asan tsan` (tools/sanitize.sh), never a substitute
LIB_PATH = os.environ.get('SODA_HIP_LIBRARY') or \
    os.path.join(_HERE, 'libsoda_hip.so')
CACHE_DIR = os.environ.get('SODA_HIP_CACHE',
                           os.path.join(_HERE, '_jit_cache'))
ARCH = 'gfx950'
# -ffp-contract=off: bit-identical fp32 results to the CPU oracle (no FMA).
# -fno-slp-vectorize: hipcc would otherwise pair neighbouring cells into
#   v_pk_add_f32/v_pk_mul_f32; on gfx950 those issue at half the rate of the
#   scalar forms and need v_mov shuffles to line registers up (measured: same
#   instruction count, ~25 % more cycles, 19 more VGPRs on jacobi2d T=8).
# * `-fwrapv`: signed integer arithmetic wraps.  The reference's kernel is
#   hardware (ap_int arithmetic: two's complement, no undefined behaviour);
#   without the flag hipcc may and does compile an overflowing int32 product
#   to something else than its wrapped value (tools/fuzz_scan.py, programs
#   2184 / 3775: 10^4-10^5 cells away from gcc's result), and the two sides of
#   a parity test would be comparing undefined behaviours.  The oracle's C is
#   built with the same flag.  Cost: within run-to-run noise on every corpus
#   program (profiles/r03_wrapv.json).
COMPILE_OPTIONS = ('--offload-arch=%s' % ARCH, '-O3', '-ffp-contract=off',
                   '-fno-slp-vectorize', '-fwrapv', '-std=c++17') + tuple(
                       os.environ.get('SODA_HIP_EXTRA_FLAGS', '').split())

MAX_DIM = 4
MAX_TENSORS = 16
MAX_KERNELS = 32
MAX_PASSES = 8
MAX_PASS_KERNELS = 16
MAX_PARAMS = 8
MAX_SLABS = 64
NAME_LEN = 96
MAX_RES_PAIRS = 8     # SODA_HIP_MAX_RES_PAIRS
GROUP_NO_OVERLAP = 1
GROUP_CALIBRATE = 2
GROUP_THREADS = 4
ABI_VERSION = 9
MAX_BATCH = 65535      # SODA_HIP_MAX_BATCH: gridDim.y


class KernelDesc(ctypes.Structure):
  _fields_ = [('name', ctypes.c_char * NAME_LEN),
              ('block', ctypes.c_int32 * 3),
              ('tile', ctypes.c_int32 * MAX_DIM),
              ('lds_bytes', ctypes.c_int32),
              ('vec', ctypes.c_int32),
              ('march_dim', ctypes.c_int32),
              ('waves_along', ctypes.c_int32),
              ('warm', ctypes.c_int32),
              ('window_extra', ctypes.c_int32),
              ('max_elem', ctypes.c_int32),
              ('vgprs', ctypes.c_int32),
              ('pipe', ctypes.c_int32),
              ('chunk_fixed', ctypes.c_int32),
              ('step_ns', ctypes.c_float),
              ('warm_saved', ctypes.c_float),
              ('bytes_per_cell', ctypes.c_float),
              ('lane_redundancy', ctypes.c_float),
              ('max_extent0', ctypes.c_int32),
              ('twin', ctypes.c_int32)]


class PassDesc(ctypes.Structure):
  _fields_ = [('fused_iters', ctypes.c_int32),
              ('num_kernels', ctypes.c_int32),
              ('kernel', ctypes.c_int32 * MAX_PASS_KERNELS),
              ('cost', ctypes.c_float)]


class ResidualStruct(ctypes.Structure):
  """Mirror of soda_hip_residual_t: the 32 device bytes a residual run fills."""
  _fields_ = [('changed', ctypes.c_uint64), ('unordered', ctypes.c_uint64),
              ('max_float_bits', ctypes.c_uint64), ('max_int', ctypes.c_uint64)]


class ResBox(ctypes.Structure):
  """Mirror of soda_hip_resbox_t."""
  _fields_ = [('lo', (ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS),
              ('hi', (ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS)]


class ResidualPlan(ctypes.Structure):
  """Mirror of soda_hip_residual_plan_t."""
  _fields_ = [('present', ctypes.c_int32), ('kernel', ctypes.c_int32),
              ('zero_kernel', ctypes.c_int32), ('whole', ctypes.c_int32),
              ('base_lo', (ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS),
              ('base_hi', (ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS),
              ('dep_lo', ((ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS) *
               MAX_RES_PAIRS),
              ('dep_hi', ((ctypes.c_int32 * MAX_DIM) * MAX_RES_PAIRS) *
               MAX_RES_PAIRS)]


NORMS_L1_WORDS, NORMS_L2_WORDS = 34, 67
NORMS_L1, NORMS_L2 = 1, 2      # SODA_HIP_NORMS_WHICH_*


class NormsStruct(ctypes.Structure):
  """Mirror of soda_hip_norms_t: the exact sums of |d| and d^2 as wide
  integers (include/soda_hip.h has the definition and the units)."""
  _fields_ = [('kind', ctypes.c_uint32), ('reserved', ctypes.c_uint32),
              ('count', ctypes.c_uint64), ('unordered', ctypes.c_uint64),
              ('infinite', ctypes.c_uint64),
              ('l1', ctypes.c_uint64 * NORMS_L1_WORDS),
              ('l2', ctypes.c_uint64 * NORMS_L2_WORDS)]

  def l1_int(self) -> int:
    """The sum of |d| as a Python integer, in the kind's units."""
    return sum(int(w) << (64 * i) for i, w in enumerate(self.l1))

  def l2_int(self) -> int:
    return sum(int(w) << (64 * i) for i, w in enumerate(self.l2))


@dataclasses.dataclass(frozen=True)
class Residual:
  """soda_hip_residual_t decoded: how much the last iteration of a run changed
  the grid (include/soda_hip.h has the definition)."""
  changed: int
  unordered: int
  max_float: float
  max_int: int

  @classmethod
  def from_struct(cls, raw: 'ResidualStruct') -> 'Residual':
    import struct
    return cls(int(raw.changed), int(raw.unordered),
               struct.unpack('<d', struct.pack('<Q', raw.max_float_bits))[0],
               int(raw.max_int))


class Plan(ctypes.Structure):
  _fields_ = [('abi_version', ctypes.c_int32), ('dim', ctypes.c_int32),
              ('num_inputs', ctypes.c_int32), ('num_outputs', ctypes.c_int32),
              ('num_locals', ctypes.c_int32),
              ('num_params', ctypes.c_int32),
              ('param_elems', ctypes.c_int32 * MAX_PARAMS),
              ('elem_size', ctypes.c_int32 * MAX_TENSORS),
              ('num_kernels', ctypes.c_int32),
              ('kernels', KernelDesc * MAX_KERNELS),
              ('num_passes', ctypes.c_int32),
              ('passes', PassDesc * MAX_PASSES),
              ('has_reach', ctypes.c_int32), ('reach_lo', ctypes.c_int32),
              ('reach_hi', ctypes.c_int32), ('batched', ctypes.c_int32),
              ('residual', ResidualPlan)]


class StreamDesc(ctypes.Structure):
  """Mirror of soda_hip_stream_desc_t (the wire-format kernel, stream.py)."""
  _fields_ = [('dim', ctypes.c_int32), ('num_inputs', ctypes.c_int32),
              ('num_outputs', ctypes.c_int32), ('iterate', ctypes.c_int32),
              ('tile', ctypes.c_int32 * MAX_DIM),
              ('stencil_distance', ctypes.c_int32),
              ('banks', ctypes.c_int32 * MAX_TENSORS),
              ('elem_size', ctypes.c_int32 * MAX_TENSORS),
              ('elems_per_cycle', ctypes.c_int32 * MAX_TENSORS),
              ('shift', ctypes.c_int32 * MAX_TENSORS),
              ('num_linear', ctypes.c_int32),
              ('linear_vec', ctypes.c_int32 * 4)]


class SlabRun(ctypes.Structure):
  """Mirror of soda_hip_slab_run_t: a run between two halo exchanges."""
  _fields_ = [('keep_lo', ctypes.c_int32), ('keep_hi', ctypes.c_int32),
              ('reach_lo', ctypes.c_int32), ('reach_hi', ctypes.c_int32),
              ('ghost_lo', ctypes.c_int32), ('ghost_hi', ctypes.c_int32),
              ('send_lo', ctypes.c_int32), ('send_hi', ctypes.c_int32),
              ('ghosts_ready', ctypes.c_void_p),
              ('sendable', ctypes.c_void_p)]


class LaunchInfo(ctypes.Structure):
  """Mirror of soda_hip_launch_info_t."""
  _fields_ = [(n, ctypes.c_int32) for n in (
      'fused_iters', 'lo', 'hi', 'wait', 'record', 'split', 'chunk', 'chunks',
      'bnd_lo', 'bnd_hi')]


class GroupDesc(ctypes.Structure):
  """Mirror of soda_hip_group_desc_t."""
  _fields_ = [('num_slabs', ctypes.c_int32),
              ('device', ctypes.c_int32 * MAX_SLABS),
              ('extent', ctypes.c_int32 * MAX_DIM),
              ('reach_lo', ctypes.c_int32), ('reach_hi', ctypes.c_int32),
              ('iterate', ctypes.c_int32),
              ('exchange_every', ctypes.c_int32),
              ('flags', ctypes.c_int32)]


class SlabInfo(ctypes.Structure):
  """Mirror of soda_hip_slab_info_t."""
  _fields_ = [('device', ctypes.c_int32),
              ('begin', ctypes.c_int32), ('end', ctypes.c_int32),
              ('own_begin', ctypes.c_int32), ('own_end', ctypes.c_int32),
              ('ghost_lo', ctypes.c_int32), ('ghost_hi', ctypes.c_int32),
              ('extent', ctypes.c_int32 * MAX_DIM),
              ('inputs', ctypes.c_void_p * MAX_TENSORS),
              ('outputs', ctypes.c_void_p * MAX_TENSORS)]


class GroupStats(ctypes.Structure):
  """Mirror of soda_hip_group_stats_t."""
  _fields_ = [('exchange_every', ctypes.c_int32),
              ('intervals', ctypes.c_int32), ('exchanges', ctypes.c_int32),
              ('copies', ctypes.c_int32), ('copy_bytes', ctypes.c_int64),
              ('launches', ctypes.c_int32), ('split_passes', ctypes.c_int32),
              ('enqueue_ms', ctypes.c_float)]


class HostTensor(ctypes.Structure):
  _fields_ = [('ptr', ctypes.c_void_p),
              ('extent', ctypes.POINTER(ctypes.c_int32)),
              ('stride', ctypes.POINTER(ctypes.c_int32)),
              ('min', ctypes.POINTER(ctypes.c_int32))]


class PeriodicDesc(ctypes.Structure):
  """Mirror of soda_hip_periodic_desc_t: a torus and its ghost frame."""
  _fields_ = [('extent', ctypes.c_int32 * MAX_DIM),
              ('refill_every', ctypes.c_int32),
              ('ghost_lo', ctypes.c_int32 * MAX_DIM),
              ('ghost_hi', ctypes.c_int32 * MAX_DIM),
              ('preserve', ctypes.c_int32),
              ('not_iterable', ctypes.c_int32)]


class PeriodicInfo(ctypes.Structure):
  """Mirror of soda_hip_periodic_info_t: what a periodic handle uses."""
  _fields_ = [('refill_every', ctypes.c_int32),
              ('ghost_lo', ctypes.c_int32 * MAX_DIM),
              ('ghost_hi', ctypes.c_int32 * MAX_DIM),
              ('padded', ctypes.c_int32 * MAX_DIM),
              ('reserved', ctypes.c_int32),
              ('scratch_bytes', ctypes.c_int64)]


class BorderDesc(ctypes.Structure):
  """Mirror of soda_hip_border_desc_t: a domain, a mode per dimension, a
  constant per input tensor."""
  _fields_ = [('domain', PeriodicDesc),
              ('mode', ctypes.c_int32 * MAX_DIM),
              ('reserved', ctypes.c_int32),
              ('constant', ctypes.c_uint64 * MAX_TENSORS)]


class BorderFaces(ctypes.Structure):
  """Mirror of soda_hip_border_faces_t: the high face's mode per dimension
  (BorderDesc.mode becomes the low face's) and a constant per input tensor,
  dimension and side."""
  _fields_ = [('mode_hi', ctypes.c_int32 * MAX_DIM),
              ('per_face_constants', ctypes.c_int32),
              ('reserved', ctypes.c_int32 * 3),
              ('constant', ((ctypes.c_uint64 * 2) * MAX_DIM) * MAX_TENSORS)]


class BorderFusedDesc(ctypes.Structure):
  """Mirror of soda_hip_border_fused_desc_t: a bordered request, the fusion
  depth, what one iteration reaches."""
  _fields_ = [('border', BorderDesc),
              ('depth', ctypes.c_int32),
              ('reach_lo', ctypes.c_int32 * MAX_DIM),
              ('reach_hi', ctypes.c_int32 * MAX_DIM),
              ('reserved', ctypes.c_int32)]


class BorderStrip(ctypes.Structure):
  """Mirror of soda_hip_border_strip_t: the strip of one wall dimension."""
  _fields_ = [('dim', ctypes.c_int32),
              ('lo', ctypes.c_int32),
              ('hi', ctypes.c_int32),
              ('take_lo', ctypes.c_int32),
              ('take_hi', ctypes.c_int32),
              ('reserved', ctypes.c_int32),
              ('extent', ctypes.c_int32 * MAX_DIM),
              ('info', PeriodicInfo)]


class BorderFusedInfo(ctypes.Structure):
  """Mirror of soda_hip_border_fused_info_t."""
  _fields_ = [('main', PeriodicInfo),
              ('depth', ctypes.c_int32),
              ('num_strips', ctypes.c_int32),
              ('strip', BorderStrip * MAX_DIM),
              ('scratch_bytes', ctypes.c_int64)]


class BorderRims(ctypes.Structure):
  """Mirror of soda_hip_border_rims_t."""
  _fields_ = [('dim', ctypes.c_int32),
              ('reserved', ctypes.c_int32),
              ('lo', (ctypes.c_int32 * MAX_DIM) * 2),
              ('hi', (ctypes.c_int32 * MAX_DIM) * 2)]


class BorderFusedBoxes(ctypes.Structure):
  """Mirror of soda_hip_border_fused_boxes_t."""
  _fields_ = [('depth', ctypes.c_int32),
              ('num_strips', ctypes.c_int32),
              ('trusted_lo', ctypes.c_int32 * MAX_DIM),
              ('trusted_hi', ctypes.c_int32 * MAX_DIM),
              ('strip', BorderRims * MAX_DIM)]


# every symbol include/soda_hip.h declares: name -> (restype, argtypes)
_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_pvp = ctypes.POINTER(ctypes.c_void_p)
_pi32 = ctypes.POINTER(ctypes.c_int32)
API = {
    'soda_hip_abi_version': (ctypes.c_int, []),
    'soda_hip_status_string': (ctypes.c_char_p, [ctypes.c_int]),
    'soda_hip_last_error': (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    'soda_hip_device_count': (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    'soda_hip_sizeof': (ctypes.c_size_t, [ctypes.c_int]),
    'soda_hip_compile': (ctypes.c_int, [
        ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), _i32,
        _pvp, ctypes.POINTER(ctypes.c_size_t)
    ]),
    'soda_hip_free_code': (None, [_vp]),
    'soda_hip_compiler_version': (ctypes.c_int, [_pi32, _pi32]),
    'soda_hip_plan_geometry': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _pi32, ctypes.POINTER(ctypes.c_float)
    ]),
    'soda_hip_plan_schedule': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, _pi32
    ]),
    'soda_hip_plan_geometry_batch': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, _pi32,
        ctypes.POINTER(ctypes.c_float)
    ]),
    'soda_hip_plan_schedule_batch': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, _i32, _pi32
    ]),
    'soda_hip_program_create': (ctypes.c_int, [
        _vp, ctypes.c_size_t, ctypes.POINTER(Plan), _i32, _pvp
    ]),
    'soda_hip_program_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_run_device': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32, _i32, _vp]),
    'soda_hip_run_device_batch': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32, _i32,
                                                 _i32, _vp]),
    'soda_hip_run_device_residual': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32,
                                                    _i32, _vp, _vp]),
    'soda_hip_run_device_until': (ctypes.c_int, [
        _vp, _pvp, _pvp, _pi32, _i32, _i32, ctypes.c_double, ctypes.c_uint64,
        ctypes.POINTER(ResidualStruct), _pi32, _vp
    ]),
    'soda_hip_plan_residual_box': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, _pi32, _pi32
    ]),
    'soda_hip_last_residual': (ctypes.c_int, [_vp, _pi32, _pi32]),
    'soda_hip_plan_residual_slab_box': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _pi32, _pi32, _i32, _i32, _i32, _pi32,
        _pi32
    ]),
    'soda_hip_run_device_slab_residual': (ctypes.c_int, [
        _vp, _pvp, _pvp, _pi32, _pi32, _pi32, _i32, _i32,
        ctypes.POINTER(SlabRun), _vp, _vp
    ]),
    'soda_hip_plan_launches_residual': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, ctypes.POINTER(SlabRun), _i32,
        ctypes.POINTER(LaunchInfo), _pi32, _pi32
    ]),
    'soda_hip_group_run_residual': (ctypes.c_int, [_vp, _i32]),
    'soda_hip_group_residual': (ctypes.c_int, [
        _vp, ctypes.POINTER(ResidualStruct), ctypes.POINTER(ResidualStruct)
    ]),
    'soda_hip_group_last_residual': (ctypes.c_int, [_vp, _i32, _pi32, _pi32]),
    'soda_hip_group_run_until': (ctypes.c_int, [
        _vp, _i32, _i32, ctypes.c_double, ctypes.c_uint64,
        ctypes.POINTER(ResidualStruct), _pi32
    ]),
    'soda_hip_norms_kind_of': (ctypes.c_int, [_i32, _pi32]),
    'soda_hip_norms_fold': (ctypes.c_int, [ctypes.POINTER(NormsStruct),
                                           ctypes.POINTER(NormsStruct)]),
    'soda_hip_norms_value': (ctypes.c_int, [ctypes.POINTER(NormsStruct), _i32,
                                            ctypes.POINTER(ctypes.c_double)]),
    'soda_hip_norms_host': (ctypes.c_int, [_vp, _vp, _i32, _i32, _pi32, _pi32,
                                           _pi32, ctypes.POINTER(NormsStruct)]),
    'soda_hip_norms_create': (ctypes.c_int, [_vp, ctypes.c_size_t, _i32, _i32,
                                             _i32, _pvp]),
    'soda_hip_norms_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_norms_zero': (ctypes.c_int, [_vp, _vp, _vp]),
    'soda_hip_norms_accumulate': (ctypes.c_int, [_vp, _vp, _vp, _pi32, _pi32,
                                                 _pi32, _vp, _vp]),
    'soda_hip_run_device_norms': (ctypes.c_int, [_vp, _vp, _pvp, _pvp, _pi32,
                                                 _i32, _vp, _vp]),
    'soda_hip_run_device_until_norm': (ctypes.c_int, [
        _vp, _vp, _pvp, _pvp, _pi32, _i32, _i32, _i32, ctypes.c_double,
        ctypes.POINTER(NormsStruct), _pi32, _vp
    ]),
    'soda_hip_wrap_host': (ctypes.c_int, [_vp, _i32, _i32, _pi32, _pi32,
                                          _pi32]),
    'soda_hip_periodic_plan': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(PeriodicDesc), _i32,
        ctypes.POINTER(PeriodicInfo), _i32, _pi32, _pi32
    ]),
    'soda_hip_periodic_create': (ctypes.c_int, [
        _vp, ctypes.POINTER(PeriodicDesc), _pvp,
        ctypes.POINTER(ctypes.c_size_t), _pvp
    ]),
    'soda_hip_periodic_info': (ctypes.c_int, [_vp,
                                              ctypes.POINTER(PeriodicInfo)]),
    'soda_hip_periodic_fill': (ctypes.c_int, [_vp, _pvp, _i32, _vp]),
    'soda_hip_extend_host': (ctypes.c_int, [_vp, _i32, _i32, _pi32, _pi32,
                                            _pi32, _pi32, ctypes.c_uint64]),
    'soda_hip_border_plan': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderDesc), _i32,
        ctypes.POINTER(PeriodicInfo), _i32, _pi32, _pi32
    ]),
    'soda_hip_border_create': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderDesc), _pvp,
        ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_vp)
    ]),
    'soda_hip_border_info': (ctypes.c_int, [_vp,
                                            ctypes.POINTER(PeriodicInfo)]),
    'soda_hip_border_fill': (ctypes.c_int, [_vp, _pvp, _i32, _vp]),
    'soda_hip_periodic_plan_batch': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(PeriodicDesc), _i32, _i32,
        ctypes.POINTER(PeriodicInfo), _i32, _pi32, _pi32
    ]),
    'soda_hip_periodic_create_batch': (ctypes.c_int, [
        _vp, ctypes.POINTER(PeriodicDesc), _i32, _pvp,
        ctypes.POINTER(ctypes.c_size_t), _pvp
    ]),
    'soda_hip_border_plan_batch': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderDesc), _i32, _i32,
        ctypes.POINTER(PeriodicInfo), _i32, _pi32, _pi32
    ]),
    'soda_hip_border_create_batch': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderDesc), _i32, _pvp,
        ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_vp)
    ]),
    'soda_hip_box_host': (ctypes.c_int, [_vp, _pi32, _vp, _pi32, _i32, _i32,
                                         _i32, _pi32, _pi32, _pi32]),
    'soda_hip_border_fused_plan': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderFusedDesc), _i32,
        ctypes.POINTER(BorderFusedInfo), _i32, _pi32, _pi32
    ]),
    'soda_hip_border_fused_create': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderFusedDesc), _pvp,
        ctypes.POINTER(ctypes.c_size_t), _pvp, ctypes.POINTER(ctypes.c_size_t),
        ctypes.POINTER(_vp)
    ]),
    'soda_hip_border_fused_info': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderFusedInfo)
    ]),
    'soda_hip_border_fused_move': (ctypes.c_int, [_vp, _i32, _i32, _pvp, _pvp,
                                                  _i32, _vp]),
    'soda_hip_border_fused_residual_boxes': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderFusedDesc),
        ctypes.POINTER(BorderFusedBoxes)
    ]),
    'soda_hip_extend_faces_host': (ctypes.c_int, [
        _vp, _i32, _i32, _pi32, _pi32, _pi32, _pi32, _pi32,
        ctypes.POINTER(ctypes.c_uint64)
    ]),
    'soda_hip_border_plan_faces': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderDesc),
        ctypes.POINTER(BorderFaces), _i32, ctypes.POINTER(PeriodicInfo), _i32,
        _pi32, _pi32
    ]),
    'soda_hip_border_plan_batch_faces': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderDesc),
        ctypes.POINTER(BorderFaces), _i32, _i32, ctypes.POINTER(PeriodicInfo),
        _i32, _pi32, _pi32
    ]),
    'soda_hip_border_create_faces': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderDesc), ctypes.POINTER(BorderFaces), _pvp,
        ctypes.POINTER(ctypes.c_size_t), _pvp, ctypes.POINTER(ctypes.c_size_t),
        ctypes.POINTER(_vp)
    ]),
    'soda_hip_border_create_batch_faces': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderDesc), ctypes.POINTER(BorderFaces), _i32,
        _pvp, ctypes.POINTER(ctypes.c_size_t), _pvp,
        ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_vp)
    ]),
    'soda_hip_border_fused_plan_faces': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderFusedDesc),
        ctypes.POINTER(BorderFaces), _i32, ctypes.POINTER(BorderFusedInfo),
        _i32, _pi32, _pi32
    ]),
    'soda_hip_border_fused_create_faces': (ctypes.c_int, [
        _vp, ctypes.POINTER(BorderFusedDesc), ctypes.POINTER(BorderFaces),
        _pvp, ctypes.POINTER(ctypes.c_size_t), _pvp,
        ctypes.POINTER(ctypes.c_size_t), _pvp,
        ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(_vp)
    ]),
    'soda_hip_border_fused_residual_boxes_faces': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(BorderFusedDesc),
        ctypes.POINTER(BorderFaces), ctypes.POINTER(BorderFusedBoxes)
    ]),
    **{
        'soda_hip_%s_%s' % (handle, name): (ctypes.c_int, argtypes)
        for handle in ('periodic', 'border', 'border_fused')
        for name, argtypes in (
            ('destroy', [_vp]),
            ('run_padded', [_vp, _pvp, _pvp, _i32, _vp]),
            ('run_device', [_vp, _pvp, _pvp, _i32, _vp]),
            ('run_padded_residual', [_vp, _pvp, _pvp, _i32, _vp, _vp]),
            ('run_padded_norms', [_vp, _vp, _pvp, _pvp, _i32, _vp, _vp]),
            ('run_until', [_vp, _pvp, _pvp, _i32, _i32, ctypes.c_double,
                           ctypes.c_uint64, ctypes.POINTER(ResidualStruct),
                           _pi32, _vp]),
            ('run_until_norm', [_vp, _vp, _pvp, _pvp, _i32, _i32, _i32,
                                ctypes.c_double, ctypes.POINTER(NormsStruct),
                                _pi32, _vp]),
        )
    },
    'soda_hip_run_device_window': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32, _pi32,
                                                  _pi32, _i32, _vp]),
    'soda_hip_run_device_cone': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32, _pi32,
                                                _pi32, _i32, _i32, _i32, _i32,
                                                _i32, _vp]),
    'soda_hip_run_device_slab': (ctypes.c_int, [_vp, _pvp, _pvp, _pi32, _pi32,
                                                _pi32, _i32,
                                                ctypes.POINTER(SlabRun), _vp]),
    'soda_hip_plan_launches': (ctypes.c_int, [
        ctypes.POINTER(Plan), _pi32, _i32, ctypes.POINTER(SlabRun), _i32,
        ctypes.POINTER(LaunchInfo), _pi32
    ]),
    'soda_hip_last_rows': (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    'soda_hip_last_split': (ctypes.c_int, [_vp, _pi32]),
    'soda_hip_program_scratch': (ctypes.c_int, [
        _vp, ctypes.POINTER(ctypes.c_int64), _pi32
    ]),
    'soda_hip_group_create': (ctypes.c_int, [
        _vp, ctypes.c_size_t, ctypes.POINTER(Plan), ctypes.POINTER(GroupDesc),
        _pvp
    ]),
    'soda_hip_group_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_group_slab': (ctypes.c_int, [_vp, _i32,
                                           ctypes.POINTER(SlabInfo)]),
    'soda_hip_group_plan': (ctypes.c_int, [
        ctypes.POINTER(Plan), ctypes.POINTER(GroupDesc), _pi32
    ]),
    'soda_hip_group_load': (ctypes.c_int, [_vp, ctypes.POINTER(HostTensor)]),
    'soda_hip_group_loaded': (ctypes.c_int, [_vp]),
    'soda_hip_group_run': (ctypes.c_int, [_vp, _i32]),
    'soda_hip_group_synchronize': (ctypes.c_int, [_vp]),
    'soda_hip_group_store': (ctypes.c_int, [_vp, ctypes.POINTER(HostTensor),
                                            _pi32, _pi32]),
    'soda_hip_group_run_host': (ctypes.c_int, [
        _vp, ctypes.POINTER(HostTensor), ctypes.POINTER(HostTensor), _i32,
        _pi32, _pi32
    ]),
    'soda_hip_group_last_stats': (ctypes.c_int, [
        _vp, ctypes.POINTER(GroupStats)
    ]),
    'soda_hip_memcpy_d2d': (ctypes.c_int, [_vp, _i32, _vp, _i32,
                                           ctypes.c_size_t, _vp]),
    'soda_hip_run_host': (ctypes.c_int, [
        _vp, ctypes.POINTER(HostTensor), ctypes.POINTER(HostTensor), _i32
    ]),
    'soda_hip_run_host_box': (ctypes.c_int, [
        _vp, ctypes.POINTER(HostTensor), ctypes.POINTER(HostTensor), _i32,
        _pi32, _pi32
    ]),
    'soda_hip_host_copy_box': (ctypes.c_int, [
        _vp, _pi32, _vp, _pi32, _pi32, _pi32, _i32, _i32, _i32, _i32, _i32
    ]),
    'soda_hip_host_weave_banks': (ctypes.c_int, [
        ctypes.POINTER(ctypes.c_void_p), _i32, _vp, ctypes.c_int64,
        ctypes.c_int64, _i32, _i32, _i32
    ]),
    'soda_hip_host_register': (ctypes.c_int, [_vp, ctypes.c_size_t]),
    'soda_hip_host_unregister': (ctypes.c_int, [_vp]),
    'soda_hip_last_launches': (ctypes.c_int, [_vp, _pi32, _pi32]),
    'soda_hip_program_set_debug_buffer': (ctypes.c_int, [_vp, _vp]),
    'soda_hip_program_calibrate': (ctypes.c_int, [_vp, _pi32, _i32, _vp]),
    'soda_hip_program_set_auto_calibrate': (ctypes.c_int, [_vp, ctypes.c_int]),
    'soda_hip_program_schedule': (ctypes.c_int, [_vp, _pi32, _i32, _pi32]),
    'soda_hip_program_pass_times': (ctypes.c_int, [
        _vp, _pi32, ctypes.POINTER(ctypes.c_float), _pi32
    ]),
    'soda_hip_program_calibrate_batch': (ctypes.c_int, [_vp, _pi32, _i32, _i32,
                                                        _vp]),
    'soda_hip_program_schedule_batch': (ctypes.c_int, [_vp, _pi32, _i32, _i32,
                                                       _pi32]),
    'soda_hip_program_pass_times_batch': (ctypes.c_int, [
        _vp, _pi32, _i32, ctypes.POINTER(ctypes.c_float), _pi32
    ]),
    'soda_hip_stream_create': (ctypes.c_int, [
        ctypes.POINTER(StreamDesc), _vp, _pvp, _pvp, _pvp, _pvp
    ]),
    'soda_hip_stream_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_stream_run_device': (ctypes.c_int, [
        _vp, _pvp, _pvp, ctypes.c_uint64, _vp
    ]),
    'soda_hip_stream_run_host': (ctypes.c_int, [_vp, _pvp, _pvp,
                                                ctypes.c_uint64]),
    'soda_hip_stream_last_mode': (ctypes.c_int, [_vp]),
    'soda_hip_stream_set_device_dense_min_tile': (ctypes.c_int, [_vp, _i32]),
    'soda_hip_stream_set_banked': (ctypes.c_int, [_vp, _vp, _pi32]),
    'soda_hip_stream_set_banked_pair': (ctypes.c_int, [_vp, _vp, _vp]),
    'soda_hip_malloc': (ctypes.c_int, [_i32, ctypes.c_size_t, _pvp]),
    'soda_hip_free': (ctypes.c_int, [_i32, _vp]),
    'soda_hip_memcpy_h2d': (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    'soda_hip_memcpy_d2h': (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    'soda_hip_memset': (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_size_t, _vp]),
    'soda_hip_stream_synchronize': (ctypes.c_int, [_vp]),
    'soda_hip_event_create': (ctypes.c_int, [_pvp]),
    'soda_hip_event_record': (ctypes.c_int, [_vp, _vp]),
    'soda_hip_event_elapsed_ms': (ctypes.c_int, [
        _vp, _vp, ctypes.POINTER(ctypes.c_float)
    ]),
    'soda_hip_event_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_event_handle': (ctypes.c_int, [_vp, _pvp]),
    'soda_hip_hipstream_create': (ctypes.c_int, [_i32, _pvp]),
    'soda_hip_hipstream_destroy': (ctypes.c_int, [_vp]),
    'soda_hip_hipstream_wait_event': (ctypes.c_int, [_vp, _vp]),
}

_lib = None


def library() -> ctypes.CDLL:
  """Loads libsoda_hip.so once; fails loudly if it was not built."""
  global _lib
  if _lib is None:
    if not os.path.exists(LIB_PATH):
      raise util.BackendError(
          '%s is missing: build it with `python -c "import __graft_entry__ as '
          'g; g.build()"` (hipcc). There is no CPU fallback.' % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own
    # libamdhip64/libhiprtc (same SONAMEs as /opt/rocm's).  Two copies in one
    # process cannot both open the GPU, so when torch is installed it is
    # loaded FIRST and libsoda_hip.so binds to the copy torch brought in.
    if not os.environ.get('SODA_HIP_NO_TORCH'):
      try:
        import torch  # noqa: F401
      except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in API.items():
      fn = getattr(lib, name)
      fn.restype = restype
      fn.argtypes = argtypes
    if lib.soda_hip_abi_version() != ABI_VERSION:
      raise util.BackendError('libsoda_hip.so has ABI version %d, expected %d' %
                              (lib.soda_hip_abi_version(), ABI_VERSION))
    for which, mirror in ((1, KernelDesc), (2, PassDesc), (3, Plan),
                          (4, HostTensor), (5, StreamDesc), (6, SlabRun),
                          (7, GroupDesc), (8, SlabInfo), (9, GroupStats),
                          (10, LaunchInfo), (11, ResidualStruct),
                          (12, ResBox), (14, NormsStruct),
                          (15, PeriodicDesc), (16, PeriodicInfo),
                          (17, BorderDesc), (18, BorderFusedDesc),
                          (19, BorderStrip), (20, BorderFusedInfo),
                          (21, BorderFusedBoxes)):
      if lib.soda_hip_sizeof(which) != ctypes.sizeof(mirror):
        raise util.BackendError(
            'struct layout mismatch between libsoda_hip.so and runtime.py '
            '(%s: %d vs %d bytes); rebuild the library' %
            (mirror.__name__, lib.soda_hip_sizeof(which),
             ctypes.sizeof(mirror)))
    _lib = lib
  return _lib


def last_error() -> str:
  lib = library()
  n = lib.soda_hip_last_error(None, 0)
  buf = ctypes.create_string_buffer(n + 1)
  lib.soda_hip_last_error(buf, n + 1)
  return buf.value.decode(errors='replace')


def check(status: int, what: str) -> None:
  if status != 0:
    lib = library()
    raise util.BackendError(
        '%s: %s: %s' % (what, lib.soda_hip_status_string(status).decode(),
                        last_error()))


def device_count() -> int:
  n = ctypes.c_int(0)
  if library().soda_hip_device_count(ctypes.byref(n)) != 0:
    return 0
  return n.value


_compiler = None


def compiler_version() -> str:
  """'hiprtc <major>.<minor>' of the library that JIT-compiles, or 'unknown'
  when it cannot be asked (no library built): part of every cache key, since
  another compiler gives the same source other registers and code sizes."""
  global _compiler
  if _compiler is None:
    try:
      a, b = ctypes.c_int32(), ctypes.c_int32()
      if library().soda_hip_compiler_version(ctypes.byref(a),
                                             ctypes.byref(b)) == 0:
        _compiler = 'hiprtc %d.%d' % (a.value, b.value)
      else:
        _compiler = 'unknown'
    except (util.SodaError, OSError):
      _compiler = 'unknown'
  return _compiler


def source_key(source: str, options: Sequence[str] = COMPILE_OPTIONS) -> str:
  """Content hash of a kernel module as it is built: compiler version, compile
  options, source text.  Names the code object in the JIT cache, and ties a
  measurement (profiles/traffic.json) to the kernels it was taken on."""
  return hashlib.sha256(
      (compiler_version() + '\0' + '\0'.join(options) + '\0' +
       source).encode()).hexdigest()[:24]


def compile_source(source: str, name: str = 'soda.hip',
                   options: Sequence[str] = COMPILE_OPTIONS,
                   cache_dir: Optional[str] = None) -> bytes:
  """HIP text -> gfx950 code object, cached on disk by content hash.  Runs
  without a GPU (hiprtc), so `build()` can pre-compile on the CPU box."""
  cache_dir = CACHE_DIR if cache_dir is None else cache_dir
  key = source_key(source, options)
  path = os.path.join(cache_dir, '%s_%s.hsaco' % (name.replace('.', '_'), key))
  if os.path.exists(path):
    with open(path, 'rb') as f:
      return f.read()
  lib = library()
  opts = [o.encode() for o in options]
  arr = (ctypes.c_char_p * len(opts))(*opts)
  code = ctypes.c_void_p()
  size = ctypes.c_size_t()
  check(
      lib.soda_hip_compile(source.encode(), name.encode(), arr, len(opts),
                           ctypes.byref(code), ctypes.byref(size)),
      'JIT of %s' % name)
  try:
    blob = ctypes.string_at(code, size.value)
  finally:
    lib.soda_hip_free_code(code)
  try:
    os.makedirs(cache_dir, exist_ok=True)
    tmp = '%s.%d.tmp' % (path, os.getpid())
    with open(tmp, 'wb') as f:
      f.write(blob)
    os.replace(tmp, path)
  except OSError:
    pass  # read-only tree: run uncached
  return blob


# ns of SIMD issue time per vector instruction of a marching kernel's row step,
# fitted with the other constants of the library's time model (soda_hip.cpp
# "Constants of the launch-time model", tools/fit_model.py); the fused kernels
# sustain 3.2-3.8 cycles per wave64 instruction at ~2.3 GHz with their lane
# shifts (profiles/)
NS_PER_VALU_OP = 1.28
# ... of a kernel whose lane shifts are split between DPP and ds_swizzle
MIXH_FACTOR = 0.849


def make_plan(mod: lower.Module,
              resources: Optional[Dict[str, dict]] = None) -> Plan:
  """The launch plan of a lowered module.  `resources` (kernel_resources of
  the compiled code) supplies the register counts the library sizes chunks
  from; without it chunks stay at their defaults."""
  st = mod.stencil
  table = st.symbol_table
  io_bytes = float(sum(table[n].size_in_bytes for n in st.input_names) +
                   sum(table[n].size_in_bytes for n in st.output_names))
  plan = Plan()
  plan.abi_version = ABI_VERSION
  plan.dim = st.dim
  # (a tensor the kernels address bank by bank -- Module.banks -- is as many
  # tensors to the library, which only passes pointers on)
  banks = mod.banks
  plan.num_inputs = sum(banks.get(n, 1) for n in st.input_names)
  plan.num_outputs = sum(banks.get(n, 1) for n in st.output_names)
  plan.num_locals = len(st.local_names)
  if len(st.param_stmts) > MAX_PARAMS:
    raise util.SemanticError('more than %d param arrays' % MAX_PARAMS)
  plan.num_params = len(st.param_stmts)
  for i, pstmt in enumerate(st.param_stmts):
    plan.param_elems[i] = st.param_elems(pstmt)
  if len(mod.elem_size) > MAX_TENSORS:
    raise util.SemanticError('more than %d tensors' % MAX_TENSORS)
  for i, s in enumerate(mod.elem_size):
    plan.elem_size[i] = s
  if len(mod.kernels) > MAX_KERNELS:
    raise util.SemanticError('more than %d kernels' % MAX_KERNELS)
  plan.num_kernels = len(mod.kernels)
  for i, k in enumerate(mod.kernels):
    if len(k.name) >= NAME_LEN:
      raise util.SemanticError('kernel name too long: %s' % k.name)
    plan.kernels[i].name = k.name.encode()
    for d in range(3):
      plan.kernels[i].block[d] = k.block[d]
    for d in range(MAX_DIM):
      plan.kernels[i].tile[d] = k.tile[d]
    plan.kernels[i].lds_bytes = k.lds_bytes
    d = plan.kernels[i]
    d.window_extra = -1
    tune = k.tune or {}
    d.vec = int(tune.get('vec') or 0)
    if 'axis' in tune:                     # a marching kernel
      d.march_dim = tune['axis'] + 1
      d.waves_along = int(tune.get('waves_along') or 1)
      d.warm = int(tune.get('warm') or 0)
      extra = tune.get('window_extra')
      d.window_extra = -1 if extra is None else int(extra)
      d.max_elem = int(tune.get('max_elem') or 0)
      d.pipe = int(tune.get('pipe') or 1)
      d.chunk_fixed = 1 if tune.get('fixed') else 0
      d.vgprs = int((resources or {}).get(k.name, {}).get('vgpr') or 0)
      d.step_ns = float(tune.get('step_ops') or 0.0) * NS_PER_VALU_OP * (
          MIXH_FACTOR if tune.get('lane_shift') == 'mixh' else 1.0)
      d.warm_saved = float(tune.get('warm_saved') or 0.0)
      # (a kernel the time model has no constants for stays unmodelled: the
      # scheduler then goes deepest first until the clock has timed the passes)
      d.bytes_per_cell = 0.0 if tune.get('unmodelled') else io_bytes
      d.lane_redundancy = float(tune.get('lane_redundancy') or 1.0)
      d.max_extent0 = int(tune.get('max_extent0') or 0)
    d.twin = int(k.twin)
    if d.twin >= 0 and resources:
      # a twin whose extra window made the compiler spill where the plain
      # kernel does not is dropped: the library then ends such a run in the
      # one-iteration pass and `<app>_residual`
      mine = resources.get(k.name, {}).get('scratch') or 0
      its = resources.get(mod.kernels[d.twin].name, {}).get('scratch') or 0
      if its > mine:
        d.twin = -1
  passes = mod.sorted_passes()
  if len(passes) > MAX_PASSES:
    raise util.SemanticError('more than %d passes' % MAX_PASSES)
  plan.num_passes = len(passes)
  for i, p in enumerate(passes):
    plan.passes[i].fused_iters = p.fused_iters
    if len(p.kernels) > MAX_PASS_KERNELS:
      raise util.SemanticError(
          'a pass of %d kernels exceeds the limit of %d' %
          (len(p.kernels), MAX_PASS_KERNELS))
    plan.passes[i].num_kernels = len(p.kernels)
    plan.passes[i].cost = 0.0    # marching passes carry a time model instead
    for j, k in enumerate(p.kernels):
      plan.passes[i].kernel[j] = k
  plan.has_reach = 1
  plan.reach_lo, plan.reach_hi = st.reach_along(st.dim - 1)
  plan.batched = 1 if mod.batch else 0
  if mod.residual:
    from soda_amd.codegen.hip import residual as _residual
    rec = _residual.box_recurrence(st)
    r = plan.residual
    r.present, r.kernel, r.whole = 1, mod.residual_kernel, int(rec['whole'])
    r.zero_kernel = mod.residual_zero_kernel
    for o in range(len(st.output_names)):
      for d in range(MAX_DIM):
        r.base_lo[o][d] = rec['base_lo'][o][d]
        r.base_hi[o][d] = rec['base_hi'][o][d]
        for i in range(len(st.input_names)):
          r.dep_lo[o][i][d] = rec['dep_lo'][o][i][d]
          r.dep_hi[o][i][d] = rec['dep_hi'][o][i][d]
  return plan


def kernel_resources(code: bytes) -> Dict[str, dict]:
  """Per-kernel register/LDS use read from the code object's AMDGPU metadata
  note (msgpack): {kernel name: {'vgpr': n, 'sgpr': n, 'lds': bytes,
  'scratch': bytes, 'code': bytes of machine code}}.  Returns {} if the note
  cannot be read."""
  import struct
  try:
    import msgpack
    if code[:4] != b'\x7fELF':
      return {}
    try:
      sizes = _function_sizes(code)
    except Exception:
      sizes = {}
    shoff, = struct.unpack_from('<Q', code, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', code, 0x3A)
    for i in range(shnum):
      off = shoff + i * shentsize
      sh_type, = struct.unpack_from('<I', code, off + 4)
      if sh_type != 7:       # SHT_NOTE
        continue
      sec_off, sec_size = struct.unpack_from('<QQ', code, off + 0x18)
      pos, end = sec_off, sec_off + sec_size
      while pos + 12 <= end:
        namesz, descsz, ntype = struct.unpack_from('<III', code, pos)
        pos += 12
        name = code[pos:pos + namesz].rstrip(b'\0')
        pos += (namesz + 3) & ~3
        desc = code[pos:pos + descsz]
        pos += (descsz + 3) & ~3
        if name == b'AMDGPU' and ntype == 32:     # NT_AMDGPU_METADATA
          meta = msgpack.unpackb(desc, raw=False, strict_map_key=False)
          out = {}
          for k in meta.get('amdhsa.kernels', []):
            out[k['.name']] = dict(
                vgpr=k.get('.vgpr_count', 0) + 0, sgpr=k.get('.sgpr_count', 0),
                agpr=k.get('.agpr_count', 0),
                lds=k.get('.group_segment_fixed_size', 0),
                scratch=k.get('.private_segment_fixed_size', 0),
                code=sizes.get(k['.name'], 0))
          return out
  except Exception:
    return {}
  return {}


def _function_sizes(code: bytes) -> Dict[str, int]:
  """{function symbol: bytes of machine code} from the ELF symbol table."""
  import struct
  out: Dict[str, int] = {}
  shoff, = struct.unpack_from('<Q', code, 0x28)
  shentsize, shnum = struct.unpack_from('<HH', code, 0x3A)
  heads = [struct.unpack_from('<IIQQQQIIQQ', code, shoff + i * shentsize)
           for i in range(shnum)]
  for h in heads:
    if h[1] != 2:                     # SHT_SYMTAB
      continue
    str_off = heads[h[6]][4]          # sh_link -> its string table
    for pos in range(h[4], h[4] + h[5], 24):
      st_name, st_info, _, _, _, st_size = struct.unpack_from('<IBBHQQ', code, pos)
      if st_info & 0xF == 2:          # STT_FUNC
        end = code.index(b'\0', str_off + st_name)
        out[code[str_off + st_name:end].decode()] = st_size
  return out


NUM_CUS = 256          # MI355X: 8 XCDs x 32 CUs, 4 SIMDs each
MAX_WAVES_PER_SIMD = 8


def waves_per_simd(vgprs: int) -> int:
  """Occupancy the register file allows (MI355X_MICROARCH.md, Register
  files: 512 VGPRs per lane per SIMD, allocation granule 8)."""
  alloc = max(8, -(-vgprs // 8) * 8)
  return max(1, min(MAX_WAVES_PER_SIMD, 512 // alloc))


def _extent_array(extent: Sequence[int], fill: int = 1):
  """`extent` as the int32[MAX_DIM] the library takes, the dimensions the
  program does not have at `fill`."""
  return (ctypes.c_int32 * MAX_DIM)(
      *(list(extent) + [fill] * (MAX_DIM - len(extent))))


def plan_geometry(plan: Plan, extent: Sequence[int]):
  """(tile of every kernel, modelled ns of every pass) the library would use
  for `extent` -- soda_hip_plan_geometry; no GPU needed.  Raises BackendError
  if a kernel of the plan cannot run this extent."""
  return _plan_geometry(plan, extent, None)


def plan_geometry_batch(plan: Plan, extent: Sequence[int], batch: int):
  """plan_geometry for ONE launch over `batch` grids of `extent`
  (soda_hip_plan_geometry_batch): the chunk lengths and the pass times of the
  whole launch.  batch = 1 is plan_geometry."""
  return _plan_geometry(plan, extent, batch)


def _plan_geometry(plan: Plan, extent: Sequence[int], batch: Optional[int]):
  """plan_geometry (batch None: the one-grid entry) and plan_geometry_batch."""
  lib = library()
  ext = _extent_array(extent)
  tiles = (ctypes.c_int32 * (MAX_DIM * plan.num_kernels))()
  ns = (ctypes.c_float * plan.num_passes)()
  if batch is None:
    check(lib.soda_hip_plan_geometry(ctypes.byref(plan), ext, tiles, ns),
          'launch geometry for extent %s' % (tuple(extent),))
  else:
    check(lib.soda_hip_plan_geometry_batch(ctypes.byref(plan), ext, batch,
                                           tiles, ns),
          'launch geometry for %d x extent %s' % (batch, tuple(extent)))
  return ([tuple(tiles[k * MAX_DIM:(k + 1) * MAX_DIM])
           for k in range(plan.num_kernels)], list(ns))


def plan_schedule_batch(plan: Plan, extent: Sequence[int], batch: int,
                        iterate: int):
  """plan_schedule for launches over `batch` grids of `extent`."""
  return _plan_schedule(plan, extent, batch, iterate)


def plan_schedule(plan: Plan, extent: Sequence[int], iterate: int):
  """How many times each pass runs for `iterate` iterations on `extent`."""
  return _plan_schedule(plan, extent, None, iterate)


def _plan_schedule(plan: Plan, extent: Sequence[int], batch: Optional[int],
                   iterate: int):
  """plan_schedule (batch None: the one-grid entry) and plan_schedule_batch."""
  lib = library()
  ext = _extent_array(extent)
  count = (ctypes.c_int32 * plan.num_passes)()
  if batch is None:
    check(lib.soda_hip_plan_schedule(ctypes.byref(plan), ext, iterate, count),
          'schedule of %d iterations' % iterate)
  else:
    check(lib.soda_hip_plan_schedule_batch(ctypes.byref(plan), ext, batch,
                                           iterate, count),
          'schedule of %d iterations on a batch of %d' % (iterate, batch))
  return list(count)


def plan_launches(plan: Plan, extent: Sequence[int], iterate: int,
                  run: Optional[SlabRun] = None, residual: bool = False):
  """The launches a run on `extent` would issue (soda_hip_plan_launches): a
  list of dicts, one per launch, in order.  No GPU needed.  `residual`: those
  of a run that takes a residual (soda_hip_plan_launches_residual) -- returns
  (launches, 'twin' | 'generic'): the last entry is the pass that takes it."""
  lib = library()
  ext = _extent_array(extent)
  n = ctypes.c_int32(0)
  cap = 4096
  arr = (LaunchInfo * cap)()
  run_p = ctypes.byref(run) if run is not None else None
  mode = ctypes.c_int32(0)
  if residual:
    check(lib.soda_hip_plan_launches_residual(ctypes.byref(plan), ext, iterate,
                                              run_p, cap, arr, ctypes.byref(n),
                                              ctypes.byref(mode)),
          'launches of %d iterations with a residual' % iterate)
  else:
    check(lib.soda_hip_plan_launches(ctypes.byref(plan), ext, iterate, run_p,
                                     cap, arr, ctypes.byref(n)),
          'launches of %d iterations' % iterate)
  out = [{name: getattr(arr[i], name) for name, _ in LaunchInfo._fields_}
         for i in range(min(n.value, cap))]
  return (out, {1: 'twin', 2: 'generic'}[mode.value]) if residual else out


def plan_residual_box(plan: Plan, extent: Sequence[int], iterate: int,
                      origin: Optional[Sequence[int]] = None,
                      global_extent: Optional[Sequence[int]] = None,
                      keep: Optional[Sequence[int]] = None):
  """[(lo, hi)] per output: the cells a residual over `iterate` iterations
  counts on `extent` (soda_hip_plan_residual_box) or, with any of `origin` /
  `global_extent` / `keep`, on that slab of a larger grid
  (soda_hip_plan_residual_slab_box).  No GPU needed."""
  dim, n = plan.dim, plan.num_outputs
  ext = _extent_array(extent)
  lo, hi = (ctypes.c_int32 * (n * dim))(), (ctypes.c_int32 * (n * dim))()
  if origin is None and global_extent is None and keep is None:
    check(library().soda_hip_plan_residual_box(ctypes.byref(plan), ext,
                                               iterate, lo, hi),
          'residual_box')
  else:
    org = _extent_array(origin or [0] * dim, fill=0)
    gext = _extent_array(global_extent or extent)
    keep = keep if keep is not None else (0, extent[dim - 1])
    check(library().soda_hip_plan_residual_slab_box(
        ctypes.byref(plan), gext, org, ext, int(keep[0]), int(keep[1]),
        iterate, lo, hi), 'residual_box of a slab')
  return [(tuple(lo[o * dim:(o + 1) * dim]), tuple(hi[o * dim:(o + 1) * dim]))
          for o in range(n)]


def pick_vec(stencil: core.Stencil, extent: Optional[Sequence[int]]) -> int:
  """Cells per lane per row: 16 bytes' worth, reduced until it divides the
  row length (rows must stay 16-byte aligned for the vector loads)."""
  vec = lower.default_vec(stencil)
  if extent is not None:
    while vec > 1 and extent[0] % vec:
      vec //= 2
  return vec


ICACHE_BYTES = 60 * 1024   # instruction cache a kernel's loop should stay in


def _compiled_resources(stencil: core.Stencil, mod: lower.Module):
  """kernel_resources of `mod` as compiled (JIT, cached; no GPU needed)."""
  return kernel_resources(compile_source(mod.source,
                                         '%s.hip' % stencil.app_name))


def _trial(stencil: core.Stencil, opts: 'lower.LowerOptions'):
  """(module, its compiled kernels' resources) of `stencil` under `opts`."""
  mod = lower.lower(stencil, opts)
  return mod, _compiled_resources(stencil, mod)


def _fused_kernel(mod: lower.Module, depth: int, marching_only: bool = False):
  """The first kernel of `mod` that fuses `depth` iterations (with
  `marching_only`: the first marching one), or None."""
  return next((k for k in mod.kernels
               if k.tune and k.tune.get('fused') == depth and
               (not marching_only or 'axis' in k.tune)), None)


def _memo(name: str, compute, encode=lambda value: value,
          decode=lambda stored: stored):
  """`compute()`, remembered as JSON in the file `name` of the kernel cache:
  decode(what the file holds) if it can be read -- a missing or corrupt file
  is a miss -- else the value computed, written as encode(value) through a
  temporary file.  A cache that cannot be written is no error."""
  import json
  path = os.path.join(CACHE_DIR, name)
  try:
    with open(path) as f:
      return decode(json.load(f))
  except (OSError, ValueError):
    pass
  value = compute()
  try:
    os.makedirs(CACHE_DIR, exist_ok=True)
    tmp = '%s.%d.tmp' % (path, os.getpid())
    with open(tmp, 'w') as f:
      json.dump(encode(value), f)
    os.replace(tmp, path)
  except OSError:
    pass
  return value


def select_peel(stencil: core.Stencil, opts: 'lower.LowerOptions',
                extent: Optional[Sequence[int]] = None) -> Dict[int, int]:
  """{fusion depth: trips of the loop whose warm-up to peel} for the marching
  kernels of `stencil` under `opts` (MarchConfig.peel).  Peeling skips stages
  that do not matter yet -- less work per chunk -- but the late, nearly full
  trips buy little and the straight-line code can need more registers than the
  loop.  Occupancy decides: per depth, the largest trip count whose COMPILED
  kernel keeps the waves per SIMD of the unpeeled kernel and spills nothing
  (jacobi2d T=12: 2 of 4 trips, 158 VGPRs; all 4 would take 231).  Code size
  decides too: the peeled steps are whole trips of the unrolled loop, and a
  3-D kernel's trip is big -- heat3d T=2: 42 KB of code unpeeled, 73 KB with
  its one trip peeled, past the instruction cache, 220-230 us against 202-205
  on 512^3.  Where chunks are long (>= 8x the warm-up, judged by the library's
  geometry for `extent`) the warm-up is a few percent and the smaller code
  wins; on a thin slab (80 planes: chunks of 8-10) peeling wins, 38 against
  69 us, also because the peeled kernel happens to need fewer registers.
  Trials are JIT-compiled (no GPU needed) and remembered in the kernel
  cache."""
  import copy
  plain = copy.copy(opts)
  plain.peel = 0
  mod0 = lower.lower(stencil, plain)
  todo = {}
  for k in mod0.kernels:
    if k.tune and k.tune.get('peel_trips_max'):
      todo[k.tune['fused']] = k.tune['peel_trips_max']
  if not todo:
    return {}
  # long chunks on this extent?  (geometry of the unpeeled kernels)
  long_chunks = {}
  res0 = _compiled_resources(stencil, mod0)
  if extent is not None:
    try:
      tiles, _ = plan_geometry(make_plan(mod0, res0), extent)
      for k, tile in zip(mod0.kernels, tiles):
        if k.tune and k.tune.get('fused') in todo:
          long_chunks[k.tune['fused']] = \
              tile[k.tune['axis']] >= 8 * max(1, k.tune.get('warm') or 1)
    except util.SodaError:
      pass
  key = hashlib.sha256(('peel3\0' + compiler_version() + '\0' +
                        '\0'.join(COMPILE_OPTIONS) + '\0' +
                        repr(sorted(long_chunks.items())) + '\0' +
                        mod0.source).encode()).hexdigest()[:24]

  def probe(depth: int, trips: int):
    if trips == 0:
      mod, res = mod0, res0
    else:
      one = copy.copy(opts)
      one.fuse = (depth,) if depth > 1 else ()
      one.peel = trips
      mod, res = _trial(stencil, one)
    k = _fused_kernel(mod, depth)
    r = res.get(k.name) if k else None
    return None if not r else (waves_per_simd(r['vgpr']), r['scratch'],
                               r.get('code', 0))

  def choose():
    chosen = {}
    for depth, most in todo.items():
      base = probe(depth, 0)
      chosen[depth] = 0
      if base is None:
        continue
      for trips in range(most, 0, -1):
        got = probe(depth, trips)
        if got is None or got[0] < base[0] or got[1] > base[1]:
          continue
        if long_chunks.get(depth) and got[2] > ICACHE_BYTES >= base[2]:
          # the warm-up is small change here; keep the code small
          continue
        chosen[depth] = trips
        break
    return chosen

  return _memo('peel_%s.json' % key, choose,
               decode=lambda got: {int(t): int(v) for t, v in got.items()})


def select_shape(stencil: core.Stencil, opts: 'lower.LowerOptions',
                 extent: Optional[Sequence[int]] = None):
  """(cells per lane, prefetch depth) for programs whose register windows the
  shape ladder of lower() (lower._one_iteration_shape) OVER-estimates, or None
  to leave its choice alone.
  The ladder counts a register per cell held; 16-bit cells are packed two to a
  register, so for tall windows of narrow integers (erosion and xcorr hold 19
  rows of int16 plus their partial-window tensors) it retreats to 2 cells per
  lane -- 8-byte loads, 129 us on 8192^2 -- where 8 cells per lane COMPILE to
  243-247 registers without spilling and run in 60-67 us
  (profiles/r03_windows_sweep.jsonl).  So, like select_peel, ask the compiler:
  the widest shape above the ladder's choice whose compiled one-iteration
  kernel fits the register file -- at most 512 registers per lane, accumulation
  registers included: one wave per SIMD (xcorr at 8 cells per lane: 314, still
  faster than 4 cells per lane at 160) -- and needs no scratch.  Trials are
  JIT-compiled (no GPU) and remembered in the kernel cache."""
  import copy
  if opts.strategy not in ('auto', 'march') or stencil.iterate > 1:
    return None
  # (the over-estimate comes from packed narrow cells only: a program of
  # 32-bit cells is left to the ladder -- and spared the trial compilations,
  # minutes for a 197-tap program like contrast)
  if min(t.size_in_bytes for t in stencil.symbol_table.values()) >= 4:
    return None
  base = copy.copy(opts)
  base.peel = 0
  mod0 = lower.lower(stencil, base)
  one = _fused_kernel(mod0, 1, marching_only=True)
  if one is None:
    return None
  chosen = int(one.tune.get('vec') or 1)
  want = int(opts.vec or lower.default_vec(stencil))
  if chosen >= want:
    return None
  key = hashlib.sha256(('shape2\0' + compiler_version() + '\0' +
                        '\0'.join(COMPILE_OPTIONS) + '\0%d\0' % want +
                        mod0.source).encode()).hexdigest()[:24]

  def widest():
    vec = want
    while vec > chosen:
      for pf in (2, 1):
        trial = copy.copy(base)
        trial.vec, trial.prefetch, trial.reg_budget = vec, pf, 1 << 20
        try:
          mod, res = _trial(stencil, trial)
        except util.SodaError:
          continue
        k = _fused_kernel(mod, 1)
        if k is None or int(k.tune.get('vec') or 0) != vec:
          continue
        r = res.get(k.name)
        # (the count includes accumulation registers used as spill space: up
        # to 512 a wave still runs, alone on its SIMD -- xcorr at 8 cells per
        # lane: 314, 60.7 us on 8192^2, against 84.7 us at 4 cells and 160)
        if r and r['scratch'] == 0 and 0 < r['vgpr'] <= 512:
          return vec, pf
      vec //= 2
    return None

  return _memo('shape_%s.json' % key, widest,
               encode=lambda found: list(found) if found else [],
               decode=lambda got: tuple(got) if got else None)


def resolve_options(stencil: core.Stencil,
                    opts: Optional['lower.LowerOptions'],
                    extent: Optional[Sequence[int]],
                    probe: bool = True) -> 'lower.LowerOptions':
  """A private copy of the caller's options with everything this module
  decides filled in: the vector width for `extent`, the peel depths.  The peel
  depths come from trial compilations (select_peel), which need the library
  and hiprtc: with probe=False, or where they are not to be had (a text-only
  use such as `sodac --hip-kernel` on a box without the library), the warm-up
  is not peeled -- deterministic, correct, a few percent slower."""
  import copy
  out = copy.copy(opts) if opts is not None else lower.LowerOptions()
  if out.vec is None:
    out.vec = pick_vec(stencil, extent)
    if out.prefetch is None and out.strategy in ('auto', 'march') and \
        lower.prefers_narrow_strips(stencil):
      # arithmetic-heavy one-iteration 2-D fp32 program: occupancy over width
      out.vec, out.prefetch = min(out.vec, 2), 4
  if out.row_cells is None and extent is not None:
    out.row_cells = int(extent[0])   # lets blocks cover whole rows (xshare)
  probing = probe and not os.environ.get('SODA_HIP_NO_PROBE')
  marchable = lower.march_supported(stencil) is None
  if probing and marchable and out.prefetch is None and \
      out.reg_budget is None and out.strategy in ('auto', 'march'):
    try:
      shape = select_shape(stencil, out, extent)
    except (util.SodaError, OSError):
      shape = None
    if shape:
      out.vec, out.prefetch = shape
      out.reg_budget = 1 << 20
  if marchable and out.peel is None and \
      out.strategy in ('auto', 'march', 'tile3d'):
    if not probing:
      out.peel = 0
    else:
      asked = out
      if out.strategy == 'tile3d':
        # its one marching kernel is the one-iteration pass `auto` builds:
        # probe that one, without compiling the tile3d kernels per trial
        asked = copy.copy(out)
        asked.strategy, asked.fuse = 'auto', ()
      try:
        out.peel = select_peel(stencil, asked, extent)
      except (util.SodaError, OSError):
        out.peel = 0
  return out


def clipped_box(box, extent: Sequence[int]):
  """A valid box (lo, hi) as the library takes it: inside the array, hi >= lo.
  An EMPTY box may come with lo beyond the array -- a program that reaches one
  way only loses `iterate x reach` cells at one end, more than a small grid
  has -- or with hi below lo; the library refuses a box outside the array."""
  lo = [min(max(l, 0), e) for l, e in zip(box[0], extent)]
  hi = [min(max(h, l), e) for l, h, e in zip(lo, box[1], extent)]
  return lo, hi


# -- exact L1 / L2 norms of a residual -----------------------
def norms_value(acc: NormsStruct, which: str) -> float:
  """The correctly rounded double of the sum of |d| (`which` = 'l1') or of d^2
  ('l2') an accumulator holds (soda_hip_norms_value; no GPU needed): +inf
  above the double range or when a delta was infinite."""
  out = ctypes.c_double()
  check(library().soda_hip_norms_value(
      ctypes.byref(acc), {'l1': NORMS_L1, 'l2': NORMS_L2}[which],
      ctypes.byref(out)), 'norms_value')
  return out.value


def norms_fold(dst: NormsStruct, src: NormsStruct) -> NormsStruct:
  """dst += src, exactly (soda_hip_norms_fold; no GPU needed): how the shares
  of bands, slabs or pairs become the norms of the whole.  Returns dst."""
  check(library().soda_hip_norms_fold(ctypes.byref(dst), ctypes.byref(src)),
        'norms_fold (kinds must match)')
  return dst


def _norms_cell(c_type: str):
  from soda_amd.codegen.hip import norms as _norms
  if c_type not in _norms.CELLS:
    raise util.InputError('norms: no kernels for cells of type `%s`' % c_type)
  return _norms.CELLS[c_type]


def norms_empty(c_type: str) -> NormsStruct:
  """A zeroed accumulator of the kind of `c_type` cells."""
  acc = NormsStruct()
  acc.kind = _norms_cell(c_type)[2]
  return acc


def norms_host(cur, prev, lo: Sequence[int], hi: Sequence[int],
               acc: Optional[NormsStruct] = None) -> NormsStruct:
  """The reduction in plain C++ on numpy arrays (soda_hip_norms_host; no GPU
  needed): the cells [lo, hi) -- dimension 0, the fastest, first -- of `cur`
  against `prev`, added to `acc` (default: a fresh one)."""
  import numpy as np
  cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
  if cur.dtype != prev.dtype or cur.shape != prev.shape:
    raise util.InputError('norms_host: two arrays of one dtype and shape')
  c_type = {'float32': 'float', 'float64': 'double'}.get(
      cur.dtype.name, cur.dtype.name + '_t')
  cell = _norms_cell(c_type)[0]
  acc = norms_empty(c_type) if acc is None else acc
  dim = cur.ndim
  ext = (ctypes.c_int32 * dim)(*cur.shape[::-1])
  check(library().soda_hip_norms_host(
      cur.ctypes.data, prev.ctypes.data, cell, dim, ext,
      (ctypes.c_int32 * dim)(*lo), (ctypes.c_int32 * dim)(*hi),
      ctypes.byref(acc)), 'norms_host')
  return acc


def norms_resources(c_type: str, dim: int):
  """(code object, kernel_resources of it) of the norms module of a cell type
  and dimension count: JIT-built like every module, cached like them; needs
  no GPU."""
  from soda_amd.codegen.hip import norms as _norms
  code = compile_source(_norms.source(c_type, dim),
                        'norms_%s_%dd.hip' % (c_type, dim))
  return code, kernel_resources(code)


class Norms:
  """The norms kernels of one cell type and dimension count on one GPU
  (soda_hip_norms_create): zero / accumulate / fetch on a caller's 840 device
  bytes.  Independent of any Program; `Program.norms()` makes the one that
  fits a program."""

  def __init__(self, c_type: str, dim: int, device: int = 0):
    self.c_type, self.dim, self.device = c_type, dim, device
    self.cell, self.elem, self.kind = _norms_cell(c_type)
    self.code, self.resources = norms_resources(c_type, dim)
    self._lib = library()
    self._handle = ctypes.c_void_p()
    check(self._lib.soda_hip_norms_create(self.code, len(self.code), self.cell,
                                          dim, device,
                                          ctypes.byref(self._handle)),
          'loading the norms kernels (%s, %d-D) on GPU %d' % (c_type, dim,
                                                              device))

  def close(self) -> None:
    if getattr(self, '_handle', None):
      self._lib.soda_hip_norms_destroy(self._handle)
      self._handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def zero(self, acc: int, stream: int = 0) -> None:
    """Zeroes the struct at device address `acc` (a kernel on `stream`)."""
    check(self._lib.soda_hip_norms_zero(self._handle, ctypes.c_void_p(acc),
                                        ctypes.c_void_p(stream)), 'norms: zero')

  def accumulate(self, cur: int, prev: int, extent: Sequence[int],
                 lo: Sequence[int], hi: Sequence[int], acc: int,
                 stream: int = 0) -> None:
    """Adds the cells [lo, hi) of the dense device arrays `cur` against `prev`
    to the struct at `acc`; asynchronous on `stream`, never allocates, does
    not zero (soda_hip_norms_accumulate)."""
    n = self.dim
    if len(extent) != n or len(lo) != n or len(hi) != n:
      raise util.InputError('norms: extent, lo and hi must have %d entries' % n)
    check(self._lib.soda_hip_norms_accumulate(
        self._handle, ctypes.c_void_p(cur), ctypes.c_void_p(prev),
        (ctypes.c_int32 * n)(*extent), (ctypes.c_int32 * n)(*lo),
        (ctypes.c_int32 * n)(*hi), ctypes.c_void_p(acc),
        ctypes.c_void_p(stream)), 'norms: accumulate')

  def fetch(self, acc: int, stream: int = 0) -> NormsStruct:
    """The struct at device address `acc`: copied on `stream`, waited for."""
    raw = NormsStruct()
    check(self._lib.soda_hip_memcpy_d2h(ctypes.byref(raw), ctypes.c_void_p(acc),
                                        ctypes.sizeof(raw),
                                        ctypes.c_void_p(stream)),
          'norms: copy out')
    check(self._lib.soda_hip_stream_synchronize(ctypes.c_void_p(stream)),
          'norms: synchronize')
    return raw


# -- periodic domains: a program on a torus ------------------
def _frame_args(arr, ghost_lo: Sequence[int], ghost_hi: Sequence[int],
                who: str, domain: str):
  """What soda_hip_wrap_host and soda_hip_extend_host take first -- address,
  cell size, dimension count, extent, ghost_lo, ghost_hi -- of the padded numpy
  array `arr`, checked; `who` and `domain` (what the ghosts leave) for the
  refusals."""
  import numpy as np
  if not isinstance(arr, np.ndarray) or not arr.flags['C_CONTIGUOUS'] or \
      not arr.flags['WRITEABLE']:
    raise util.InputError('%s: a writable C-contiguous numpy array' % who)
  dim = arr.ndim
  if len(ghost_lo) != dim or len(ghost_hi) != dim:
    raise util.InputError('%s: %d ghost widths per side' % (who, dim))
  padded = arr.shape[::-1]
  extent = [p - l - h for p, l, h in zip(padded, ghost_lo, ghost_hi)]
  if arr.dtype.itemsize not in (1, 2, 4, 8) or not 1 <= dim <= MAX_DIM or \
      min(extent) < 1 or min(ghost_lo) < 0 or min(ghost_hi) < 0:
    raise util.InputError(
        '%s: cells of 1, 2, 4 or 8 bytes, 1 to %d dimensions, ghosts '
        '>= 0 that leave %s of at least one cell' % (who, MAX_DIM, domain))
  return (arr.ctypes.data, arr.dtype.itemsize, dim,
          (ctypes.c_int32 * dim)(*extent), (ctypes.c_int32 * dim)(*ghost_lo),
          (ctypes.c_int32 * dim)(*ghost_hi))


def wrap_host(arr, ghost_lo: Sequence[int], ghost_hi: Sequence[int]):
  """Refills the ghost frame of the padded numpy array `arr` IN PLACE from its
  interior, every ghost cell taking the interior cell it mirrors on the torus
  (soda_hip_wrap_host, plain C++; no GPU needed).  `ghost_lo` / `ghost_hi`:
  ghost cells below / above the torus per dimension, dimension 0 (the fastest,
  the LAST numpy axis) first.  Returns `arr`."""
  args = _frame_args(arr, ghost_lo, ghost_hi, 'wrap_host', 'a torus')
  check(library().soda_hip_wrap_host(*args), 'wrap_host')
  return arr


def periodic_ghosts(stencil: core.Stencil, refill_every: int):
  """(ghost_lo, ghost_hi) a frame must have to carry `refill_every` iterations
  of `stencil`: the most `Stencil.window_bounds(refill_every)` reaches below /
  above over ALL outputs (one-sided programs get one-sided ghosts, coupled
  outputs the widest), and along the last dimension at least `refill_every`
  times the per-iteration reach the plan carries -- the library refuses
  less."""
  boxes = stencil.window_bounds(refill_every)
  dim = stencil.dim
  lo = [max(0, max(-boxes[o][0][d] for o in stencil.output_names))
        for d in range(dim)]
  hi = [max(0, max(boxes[o][1][d] for o in stencil.output_names))
        for d in range(dim)]
  rl, rh = stencil.reach_along(dim - 1)
  lo[-1] = max(lo[-1], refill_every * rl)
  hi[-1] = max(hi[-1], refill_every * rh)
  return lo, hi


def _periodic_desc(dim: int, extent: Sequence[int], refill_every: int,
                   ghost_lo: Sequence[int], ghost_hi: Sequence[int],
                   preserve: bool, not_iterable: bool = False
                   ) -> PeriodicDesc:
  if len(extent) != dim or len(ghost_lo) != dim or len(ghost_hi) != dim:
    raise util.InputError('periodic: extent and ghosts must have %d entries' %
                          dim)
  desc = PeriodicDesc()
  for d in range(dim):
    desc.extent[d] = extent[d]
    desc.ghost_lo[d], desc.ghost_hi[d] = ghost_lo[d], ghost_hi[d]
  desc.refill_every = refill_every
  desc.preserve = 1 if preserve else 0
  desc.not_iterable = 1 if not_iterable else 0
  return desc


def _periodic_info(raw: PeriodicInfo, dim: int) -> dict:
  return {'refill_every': raw.refill_every,
          'ghost_lo': tuple(raw.ghost_lo[:dim]),
          'ghost_hi': tuple(raw.ghost_hi[:dim]),
          'padded': tuple(raw.padded[:dim]),
          'scratch_bytes': int(raw.scratch_bytes)}


def periodic_plan(plan: Plan, extent: Sequence[int], refill_every: int,
                  ghost_lo: Sequence[int], ghost_hi: Sequence[int],
                  iterate: int = 0, preserve: bool = False,
                  not_iterable: bool = False, batch: Optional[int] = None):
  """(info, chunks) a periodic handle over `plan` would use for a torus of
  `extent` (soda_hip_periodic_plan; no GPU needed): info as Periodic.info(),
  chunks the iterations of every chunk of a run of `iterate`.  Refuses what
  the handle refuses (BackendError).  `batch` = N: of a batched handle over N
  tori (soda_hip_periodic_plan_batch)."""
  desc = _periodic_desc(plan.dim, extent, refill_every, ghost_lo, ghost_hi,
                        preserve, not_iterable)
  raw, chunks = _plan_call('periodic_plan', plan, desc, PeriodicInfo(),
                           iterate, batch)
  return _periodic_info(raw, plan.dim), chunks


def _plan_call(what: str, plan: Plan, desc, raw, iterate: int,
               batch: Optional[int] = None, faces=None):
  """The plan entry soda_hip_<what> on `desc` -- `batch` an integer:
  soda_hip_<what>_batch; `faces` a BorderFaces: the `_faces` twin of either
  -- : (`raw`, the info struct, filled; the iterations of every chunk of a run
  of `iterate`)."""
  cap = max(1, iterate)
  chunks = (ctypes.c_int32 * cap)()
  n = ctypes.c_int32()
  if batch is not None:
    what += '_batch'
  if faces is not None:
    what += '_faces'
  fn = getattr(library(), 'soda_hip_' + what)
  head = (ctypes.byref(plan), ctypes.byref(desc)) + (
      () if faces is None else (ctypes.byref(faces),)) + (
          () if batch is None else (int(batch),))
  check(fn(*head, iterate, ctypes.byref(raw), cap, chunks, ctypes.byref(n)),
        what)
  return raw, list(chunks[:n.value])


def _helper_resources(module, stem: str, elem: int, dim: int,
                      batch: bool = False):
  """(code object, kernel_resources of it) of a helper module (wrap, extend,
  box) of a cell size and dimension count: `module`.source is its text,
  `stem` names its file.  `batch`: the batched module (wrap, extend)."""
  if batch:
    code = compile_source(module.source(elem, dim, batch=True),
                          '%s_bt_e%d_%dd.hip' % (stem, elem, dim))
  else:
    code = compile_source(module.source(elem, dim),
                          '%s_e%d_%dd.hip' % (stem, elem, dim))
  return code, kernel_resources(code)


def wrap_resources(elem: int, dim: int, batch: bool = False):
  """(code object, kernel_resources of it) of the wrap module of a cell size
  and dimension count -- `batch`: of the batched one --
  JIT-built like every module, cached like them; needs no GPU."""
  from soda_amd.codegen.hip import wrap as _wrap
  return _helper_resources(_wrap, 'wrap', elem, dim, batch)


class Periodic:
  """A program on a torus of ONE extent (soda_hip_periodic_create): the state
  lives in padded arrays whose ghost frame carries `refill_every` iterations
  of the program's ordinary kernels and is refilled on the GPU in between.
  Made by `Program.periodic`; close it before its program."""

  _entry = 'soda_hip_periodic_'    # the library's entries of this handle
  _what = 'periodic'

  def _fn(self, name):
    return getattr(self._lib, self._entry + name)

  def _codes_of(self, *resources):
    """[codes, sizes, ...] for the create entry, a pair per function of
    `resources`: the code object `resources[j](elem, dim)` gives for every
    cell size among the inputs and outputs."""
    st = self.prog.stencil
    self._codes = []                # (the buffers, kept alive with the handle)
    args = []
    for resource in resources:
      codes = (ctypes.c_void_p * 4)()
      sizes = (ctypes.c_size_t * 4)()
      if resource is None:          # (a module the request never looks at)
        pass
      elif not st.preserve_border:  # (refused by create: nothing to build for)
        sizes_needed = {t.size_in_bytes
                        for t in list(st.input_types) + list(st.output_types)}
        for elem in sorted(sizes_needed & {1, 2, 4, 8}):
          code, _ = resource(elem, st.dim)
          buf = ctypes.create_string_buffer(code, len(code))
          self._codes.append(buf)
          i = elem.bit_length() - 1
          codes[i] = ctypes.cast(buf, ctypes.c_void_p)
          sizes[i] = len(code)
      args += [codes, sizes]
    return args

  def _begin(self, prog: 'Program', extent: Sequence[int], modes=None,
             batch: Optional[int] = None) -> bool:
    """What every constructor starts with: the extent checked and kept, the
    `modes` of a bordered domain kept one name per dimension, `batch` (None:
    an unbatched handle; N: one over N domains).  Returns the
    `not_iterable` of the desc."""
    st = prog.stencil
    self.prog, self.extent = prog, tuple(int(e) for e in extent)
    self.batch = None if batch is None else int(batch)
    prog._check_extent(self.extent)
    if modes is not None:
      self.modes = _mode_names(modes, st.dim)
    return list(st.input_types) != list(st.output_types)

  def _create(self, desc, resources, where: str, faces=None) -> None:
    """What every constructor ends with: the handle made by the library's
    create entry from `desc` and the code objects of `resources`, and
    registered with its program.  `where`: the domain, for a refusal.
    `faces`: a BorderFaces, and the `_faces` twin of the entry -- with the
    faces modules behind the others and without the extend modules, which
    such a request never looks at."""
    self._lib = library()
    self._handle = ctypes.c_void_p()
    head, twin = (ctypes.byref(desc),), ''
    if faces is not None:
      resources = [None if r is extend_resources else r
                   for r in resources] + [faces_resources]
      head, twin = (ctypes.byref(desc), ctypes.byref(faces)), '_faces'
    if self.batch is None:
      args = self._codes_of(*resources)
      status = self._fn('create' + twin)(self.prog._handle, *head, *args,
                                         ctypes.byref(self._handle))
    else:                           # the batched modules, the _batch entry
      args = self._codes_of(*[r and functools.partial(r, batch=True)
                              for r in resources])
      status = self._fn('create_batch' + twin)(
          self.prog._handle, *head, self.batch, *args,
          ctypes.byref(self._handle))
      where = '%d x %s' % (self.batch, where)
    check(status, '`%s` on %s' % (self.prog.stencil.app_name, where))
    self.prog._periodic.append(self)

  def __init__(self, prog: 'Program', extent: Sequence[int],
               refill_every: Optional[int] = None,
               ghosts: Optional[Sequence[Sequence[int]]] = None,
               batch: Optional[int] = None):
    """`refill_every`: iterations between two refills (default: the deepest
    fusion depth of the program, so that a chunk is one launch).  `ghosts` =
    (lo, hi): the frame, for callers that size it themselves (default:
    periodic_ghosts).  `batch` = N: a handle over N tori of `extent`, every
    array [N, ...] (soda_hip_periodic_create_batch)."""
    not_iterable = self._begin(prog, extent, batch=batch)
    st = prog.stencil
    k = int(refill_every or 0)
    if k < 0:
      raise util.InputError('periodic: refill_every < 0')
    if not k:
      k = max(p.fused_iters for p in prog.module.passes)
    lo, hi = ghosts if ghosts is not None else periodic_ghosts(st, k)
    desc = _periodic_desc(st.dim, self.extent, k, lo, hi, st.preserve_border,
                          not_iterable)
    self._create(desc, [wrap_resources],
                 'a torus of %s' % 'x'.join(map(str, self.extent)))

  def close(self) -> None:
    if getattr(self, '_handle', None):
      self._fn('destroy')(self._handle)
      self._handle = None
      if self in self.prog._periodic:
        self.prog._periodic.remove(self)

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def info(self) -> dict:
    """{'refill_every', 'ghost_lo', 'ghost_hi', 'padded', 'scratch_bytes'}:
    what the library chose (ghost_hi[0] rounded up until padded[0] is a
    multiple of the program's vector width) and holds."""
    raw = PeriodicInfo()
    check(self._fn('info')(self._handle, ctypes.byref(raw)),
          '%s: info' % self._what)
    return _periodic_info(raw, self.prog.stencil.dim)

  def fill(self, arrays: Sequence[int], stream: int = 0) -> None:
    """Refills the ghost frame of padded device arrays in place (array i: the
    cells of output i); asynchronous on `stream`."""
    arr = (ctypes.c_void_p * max(1, len(arrays)))(*arrays)
    check(self._fn('fill')(self._handle, arr, len(arrays),
                           ctypes.c_void_p(stream)), '%s: fill' % self._what)

  def _check_counts(self, what, outputs, inputs):
    st = self.prog.stencil
    if len(outputs) != len(st.output_names) or \
        len(inputs) != len(st.input_names) + len(st.param_stmts):
      raise util.InputError('%s: %d outputs, %d inputs and param arrays' % (
          what, len(st.output_names),
          len(st.input_names) + len(st.param_stmts)))

  def _run(self, fn, what, outputs, inputs, iterate, stream):
    st = self.prog.stencil
    iterate = st.iterate if iterate is None else iterate
    self._check_counts(what, outputs, inputs)
    outs = (ctypes.c_void_p * len(outputs))(*outputs)
    ins = (ctypes.c_void_p * len(inputs))(*inputs)
    check(fn(self._handle, outs, ins, iterate, ctypes.c_void_p(stream)),
          '%s of `%s`' % (what, st.app_name))

  def run_padded(self, outputs: Sequence[int], inputs: Sequence[int],
                 iterate: Optional[int] = None, stream: int = 0,
                 residual: Optional[int] = None,
                 norms: Optional[int] = None) -> None:
    """`iterate` iterations on PADDED device arrays of info()['padded']: the
    inputs (then the param arrays) arrive wrapped, the outputs leave wrapped,
    the inputs are never written (soda_hip_periodic_run_padded).
    `residual` = the device address of 32 bytes / `norms` = of a
    soda_hip_norms_t (8-byte aligned, one of the two): the run also leaves
    there how much its LAST iteration changed the DOMAIN, all of its cells and
    no ghost cell (soda_hip_periodic_run_padded_residual / _norms; DESIGN.md
    4.14; `Program.residual(ptr)` / `Program.norms().fetch(ptr)` read them).
    The struct is zeroed on `stream` inside the call, which stays asynchronous
    and capturable.  Needs a program built with LowerOptions.residual."""
    if residual is None and norms is None:
      return self._run(self._fn('run_padded'), '%s run_padded' % self._what,
                       outputs, inputs, iterate, stream)
    if residual is not None and norms is not None:
      raise util.InputError('%s run_padded: residual or norms, not both' %
                            self._what)
    if residual is not None:
      fn = self._fn('run_padded_residual')
      entry = lambda h, outs, ins, n, on: fn(h, outs, ins, n,
                                             ctypes.c_void_p(residual), on)
    else:
      fn, nh = self._fn('run_padded_norms'), self.prog.norms()._handle
      entry = lambda h, outs, ins, n, on: fn(h, nh, outs, ins, n,
                                             ctypes.c_void_p(norms), on)
    self._run(entry, '%s run_padded with %s' % (
        self._what, 'a residual' if norms is None else 'norms'),
              outputs, inputs, iterate, stream)

  def run_until(self, outputs: Sequence[int], inputs: Sequence[int],
                tol: float, max_iterate: int, check_every: int = 8,
                int_tol: int = 0, norm: Optional[str] = None,
                stream: int = 0):
    """Iterates on DENSE device arrays of the domain's extent until converged
    (soda_hip_periodic_run_until / _until_norm; synchronous): `check_every`
    iterations at a time on the handle's padded scratch, the stop rules of
    `Program.run_until` on the residual of the whole domain (`norm` = 'l1' |
    'l2': on that exact norm).  Returns (iterations done, Residual -- or the
    NormsStruct of the last chunk)."""
    if norm not in (None, 'l1', 'l2'):
      raise util.InputError("run_until: norm is None, 'l1' or 'l2'")
    st = self.prog.stencil
    self._check_counts('%s run_until' % self._what, outputs, inputs)
    outs = (ctypes.c_void_p * len(outputs))(*outputs)
    ins = (ctypes.c_void_p * len(inputs))(*inputs)
    done = ctypes.c_int32(0)
    on = ctypes.c_void_p(stream)
    if norm is None:
      raw = ResidualStruct()
      check(self._fn('run_until')(
          self._handle, outs, ins, int(max_iterate), int(check_every),
          float(tol), int(int_tol), ctypes.byref(raw), ctypes.byref(done), on),
            '%s: running `%s` until converged' % (self._what, st.app_name))
      return done.value, Residual.from_struct(raw)
    raw = NormsStruct()
    check(self._fn('run_until_norm')(
        self._handle, self.prog.norms()._handle, outs, ins, int(max_iterate),
        int(check_every), {'l1': NORMS_L1, 'l2': NORMS_L2}[norm], float(tol),
        ctypes.byref(raw), ctypes.byref(done), on),
          '%s: running `%s` until its %s norm is small' % (
              self._what, st.app_name, norm))
    return done.value, raw

  def run_device(self, outputs: Sequence[int], inputs: Sequence[int],
                 iterate: Optional[int] = None, stream: int = 0) -> None:
    """The same on DENSE device arrays of the torus's extent: padded into the
    handle's scratch, run, cropped (soda_hip_periodic_run_device)."""
    self._run(self._fn('run_device'), '%s run_device' % self._what,
              outputs, inputs, iterate, stream)


# -- bordered domains: a border mode per dimension -----------
def _face_pair(entry):
  """[low, high] of one dimension's entry of `modes`: one name (or number) for
  both faces, a (low, high) pair, or the string 'low/high'."""
  if isinstance(entry, str):
    pair = entry.split('/') if '/' in entry else [entry, entry]
  elif isinstance(entry, (tuple, list)):
    pair = list(entry)
  else:
    pair = [entry, entry]
  if len(pair) != 2:
    raise util.InputError('border: a dimension takes one mode or a (low, high) '
                          'pair of modes, not %r' % (entry,))
  return pair


def _border_faces(modes, dim: int):
  """(low, high): SODA_HIP_BORDER_* of the two faces per dimension of `modes`
  -- one entry for all dimensions or one per dimension, dimension 0 first, an
  entry one name for both faces, a (low, high) pair of names or the string
  'low/high' (DESIGN.md 4.16).  `wrap` comes as the pair (wrap, wrap) only."""
  from soda_amd.codegen.hip import extend as _extend
  names = [modes] * dim if isinstance(modes, str) else list(modes)
  if len(names) != dim:
    raise util.InputError('border: one mode, or one per dimension (%d)' % dim)
  low, high = [], []
  for entry in names:
    pair = _face_pair(entry)
    for m in pair:
      if not isinstance(m, str) or m not in _extend.MODES:
        raise util.InputError('border: unknown mode %r (one of %s)' % (
            m, ', '.join(sorted(_extend.MODES))))
    if (pair[0] == 'wrap') != (pair[1] == 'wrap'):
      raise util.InputError('border: a dimension wraps on both faces or on '
                            'none, not %s/%s' % tuple(pair))
    low.append(_extend.MODES[pair[0]])
    high.append(_extend.MODES[pair[1]])
  return low, high


def _border_modes(modes, dim: int):
  """SODA_HIP_BORDER_* per dimension of `modes` (_border_faces): of the LOW
  faces, which say as much as both about which dimensions wrap."""
  return _border_faces(modes, dim)[0]


def _mode_names(modes, dim: int):
  """`modes` one string per dimension, a pair as 'low/high'."""
  names = [modes] * dim if isinstance(modes, str) else list(modes)
  return tuple(m if isinstance(m, str) else '/'.join(map(str, m))
               for m in names)


def _cell_bits(value, np_name: str) -> int:
  """The bit pattern of `value` as a cell of a numpy type, in a uint64."""
  import numpy as np
  cell = np.asarray(value).astype(np.dtype(np_name)).reshape(1)
  return int.from_bytes(cell.tobytes(), sys.byteorder)


def _border_constants(stencil: core.Stencil, constants):
  """One uint64 per input of `stencil`: `constants` is None (zero), a scalar
  for every input or {input: scalar}."""
  if constants is None:
    constants = {}
  if not isinstance(constants, dict):
    constants = {n: constants for n in stencil.input_names}
  unknown = sorted(set(constants) - set(stencil.input_names))
  if unknown:
    raise util.InputError('border: constants for %s, which are no inputs' %
                          ', '.join(unknown))
  return [_cell_bits(constants.get(n, 0), t.np_name)
          for n, t in zip(stencil.input_names, stencil.input_types)]


def _per_face(spec, dim: int, what: str):
  """[[low, high]] * dim of the constants of one tensor: `spec` a scalar (every
  face), or a sequence of `dim` entries, each a scalar (both faces of the
  dimension) or a (low, high) pair; None where `spec` is a scalar."""
  if not isinstance(spec, (list, tuple)):
    return None
  if len(spec) != dim:
    raise util.InputError('%s: constants per face come one entry per '
                          'dimension (%d), each a scalar or a (low, high) '
                          'pair' % (what, dim))
  out = []
  for entry in spec:
    pair = list(entry) if isinstance(entry, (list, tuple)) else [entry, entry]
    if len(pair) != 2:
      raise util.InputError('%s: a dimension takes one constant or a (low, '
                            'high) pair, not %r' % (what, entry))
    out.append(pair)
  return out


def _border_face_constants(stencil: core.Stencil, constants):
  """Per input of `stencil` the bits of its constants [dimension][side], or
  None where every input takes one constant on every face (_border_constants
  has those): `constants` as for _border_constants, or in a scalar's place a
  sequence of `dim` entries, each a scalar or a (low, high) pair."""
  if constants is None:
    return None
  if not isinstance(constants, dict):
    constants = {n: constants for n in stencil.input_names}
  dim = stencil.dim
  specs = {n: _per_face(c, dim, 'border') for n, c in constants.items()}
  if all(s is None for s in specs.values()):
    return None
  unknown = sorted(set(constants) - set(stencil.input_names))
  if unknown:
    raise util.InputError('border: constants for %s, which are no inputs' %
                          ', '.join(unknown))
  table = []
  for n, t in zip(stencil.input_names, stencil.input_types):
    spec = specs.get(n) or [[constants.get(n, 0)] * 2] * dim
    table.append([[_cell_bits(v, t.np_name) for v in pair] for pair in spec])
  return table


def _faces_forced() -> bool:
  """SODA_HIP_FACES_FORCE=1 (A/B runs, tools/faces_ab.py): a symmetric
  request goes through the `_faces` entries with the faces modules too."""
  return os.environ.get('SODA_HIP_FACES_FORCE') == '1'


def _shown_constants(low, high, rows):
  """The constants of one tensor ([dimension][side]) on the faces whose mode
  is `constant` (SODA_HIP_BORDER_CONSTANT), the only ones that ever show."""
  return [c for d, pair in enumerate(rows)
          for m, c in zip((low[d], high[d]), pair) if m == 4]


def _border_faces_struct(low, high, table=None, force: bool = False):
  """The BorderFaces of a request with the faces `low` / `high` and the
  constants `table` (_border_face_constants), or None where it is the request
  of the low faces alone: pairs alike, every tensor one constant on the faces
  that show one (those whose mode is `constant`)."""
  uneven = table is not None and any(
      len(set(_shown_constants(low, high, rows))) > 1 for rows in table)
  if list(low) == list(high) and not uneven and not force:
    return None
  faces = BorderFaces()
  for d, m in enumerate(high):
    faces.mode_hi[d] = m
  if table is not None:
    faces.per_face_constants = 1
    for i, rows in enumerate(table):
      for d, pair in enumerate(rows):
        faces.constant[i][d][0], faces.constant[i][d][1] = pair
  return faces


def extend_host(arr, ghost_lo: Sequence[int], ghost_hi: Sequence[int], modes,
                constant=0):
  """wrap_host with a border mode per dimension: refills the ghost frame of the
  padded numpy array `arr` IN PLACE from its interior (soda_hip_extend_host,
  plain C++; no GPU needed).  `modes`: one name or one per dimension,
  dimension 0 (the LAST numpy axis) first; `constant`: the value of a ghost
  cell outside in a `constant` dimension, converted to the cell type.  A
  dimension's mode may be a (low, high) pair or 'low/high', and `constant` a
  sequence of one entry per dimension, each a scalar or a (low, high) pair
  (soda_hip_extend_faces_host).  Returns `arr`."""
  import numpy as np
  args = _frame_args(arr, ghost_lo, ghost_hi, 'extend_host', 'a domain')
  dim = arr.ndim
  low, high = _border_faces(modes, dim)
  per_face = _per_face(constant, dim, 'extend_host')

  def cell(value):
    bits = value if isinstance(value, (bytes, bytearray)) else \
        np.asarray(value).astype(arr.dtype).tobytes()
    if len(bits) != arr.dtype.itemsize:
      raise util.InputError('extend_host: a constant of one cell')
    return int.from_bytes(bits, sys.byteorder)
  if per_face is None and low == high:
    check(library().soda_hip_extend_host(
        *args, (ctypes.c_int32 * dim)(*low), cell(constant)), 'extend_host')
    return arr
  flat = [cell(v) for pair in per_face or [[constant] * 2] * dim for v in pair]
  check(library().soda_hip_extend_faces_host(
      *args, (ctypes.c_int32 * dim)(*low), (ctypes.c_int32 * dim)(*high),
      (ctypes.c_uint64 * (2 * dim))(*flat)), 'extend_host')
  return arr


def border_ghosts(stencil: core.Stencil, modes):
  """(ghost_lo, ghost_hi) of a bordered domain: with a mode other than `wrap`
  the frame of ONE iteration (periodic_ghosts(stencil, 1): the most
  window_bounds(1) reaches over all outputs, along the last dimension at
  least the plan's reach) -- it is refilled after every iteration."""
  _border_modes(modes, stencil.dim)
  return periodic_ghosts(stencil, 1)


def _border_desc(domain: PeriodicDesc, modes,
                 constants: Sequence[int]) -> BorderDesc:
  desc = BorderDesc()
  desc.domain = domain
  for d, m in enumerate(modes):
    desc.mode[d] = m
  for i, c in enumerate(constants):
    desc.constant[i] = c
  return desc


def border_plan(plan: Plan, extent: Sequence[int], modes,
                ghost_lo: Sequence[int], ghost_hi: Sequence[int],
                iterate: int = 0, refill_every: int = 0,
                preserve: bool = False, not_iterable: bool = False,
                batch: Optional[int] = None):
  """periodic_plan for a bordered domain (soda_hip_border_plan; no GPU
  needed): (info, chunks).  `modes`: names, or raw SODA_HIP_BORDER_* numbers
  (which reach the library unchecked).  With a mode other than `wrap`,
  `refill_every` must be 0 or 1 and every chunk is one iteration; with all
  `wrap` this is periodic_plan.  `batch` = N: of a batched handle over N
  domains (soda_hip_border_plan_batch)."""
  raw_modes, faces = _raw_faces(modes, plan.dim)
  desc = _border_desc(_periodic_desc(
      plan.dim, extent, refill_every, ghost_lo, ghost_hi, preserve,
      not_iterable), raw_modes, ())
  raw, chunks = _plan_call('border_plan', plan, desc, PeriodicInfo(), iterate,
                           batch, faces)
  return _periodic_info(raw, plan.dim), chunks


def _raw_modes(modes, dim: int, *reaches):
  """SODA_HIP_BORDER_* per dimension for a plan entry: `modes` as names
  (_border_modes), or as raw numbers, which pass unchecked.  `reaches`: the
  reach_lo and reach_hi of a fused request, which need `dim` entries too."""
  raw = list(modes) if not isinstance(modes, str) and all(
      isinstance(m, int) for m in modes) else _border_modes(modes, dim)
  if any(len(v) != dim for v in (raw,) + reaches):
    raise util.InputError('border: one mode%s per dimension (%d)' % (
        ' and one reach per side' if reaches else '', dim))
  return raw


def _raw_faces(modes, dim: int, *reaches):
  """(the low faces as _raw_modes gives them, the BorderFaces of the `_faces`
  twin of a plan entry or None where every pair is alike): `modes` as names
  (_border_faces), or as raw numbers -- a number or a (low, high) pair of
  numbers per dimension -- which pass unchecked."""
  entries = [modes] * dim if isinstance(modes, str) else list(modes)
  pairs = [_face_pair(m) for m in entries]
  if entries and all(isinstance(f, int) for p in pairs for f in p):
    low, high = [p[0] for p in pairs], [p[1] for p in pairs]    # raw numbers
  else:                           # names: checked, a mixed list among them
    low, high = _border_faces(modes, dim)
  _raw_modes(low, dim, *reaches)  # one per dimension, the reaches too
  return low, _border_faces_struct(low, high)


def _border_request(stencil: core.Stencil, modes, constants):
  """What a bordered handle is made from: (the low faces' SODA_HIP_BORDER_*,
  the BorderFaces of the `_faces` create entry or None where the request is
  one of soda_hip_border_create, a constant per input for the desc)."""
  low, high = _border_faces(modes, stencil.dim)
  table = _border_face_constants(stencil, constants)
  flat = [(_shown_constants(low, high, rows) or [rows[0][0]])[0]
          for rows in table] if table is not None else \
      _border_constants(stencil, constants)
  return low, _border_faces_struct(low, high, table, _faces_forced()), flat


def extend_resources(elem: int, dim: int, batch: bool = False):
  """(code object, kernel_resources of it) of the extend module of a cell size
  and dimension count -- `batch`: of the batched one --
  JIT-built like every module, cached like them; needs no GPU."""
  from soda_amd.codegen.hip import extend as _extend
  return _helper_resources(_extend, 'extend', elem, dim, batch)


def faces_resources(elem: int, dim: int, batch: bool = False):
  """(code object, kernel_resources of it) of the faces module of a cell size
  and dimension count (a border mode per face) -- `batch`: of
  the batched one -- JIT-built like every module, cached like them; needs no
  GPU."""
  from soda_amd.codegen.hip import faces as _faces
  return _helper_resources(_faces, 'faces', elem, dim, batch)


class Bordered(Periodic):
  """A program on a domain of ONE extent with a border mode per dimension
  (soda_hip_border_create): Periodic's padded arrays and entries, the ghost
  frame refilled under the modes after every iteration -- or, with every
  dimension `wrap`, the torus of Periodic at its default refill interval.
  Made by `Program.bordered`; close it before its program."""

  _entry = 'soda_hip_border_'
  _what = 'border'

  def __init__(self, prog: 'Program', extent: Sequence[int], modes,
               constants=None, batch: Optional[int] = None):
    """`modes`: one name for all dimensions or one per dimension, dimension 0
    first, of wrap / clamp / mirror / mirror101 / constant.  `constants`: a
    scalar or {input: scalar}, converted to the cell type's bits (default
    zero); an output's ghost takes the constant of the input it replaces.
    `batch` = N: a handle over N domains of `extent`, every array [N, ...]
    (soda_hip_border_create_batch).
    A mode and a constant per FACE: a dimension's entry of
    `modes` may be a (low, high) pair of names or 'low/high' (`wrap` as the
    pair of both only); a constant may be a sequence of one entry per
    dimension, each a scalar or a (low, high) pair.  A request whose pairs
    are alike and whose constants are one per tensor is the request above,
    with its kernels; any other fills with the faces kernels
    (soda_hip_border_create_faces)."""
    not_iterable = self._begin(prog, extent, modes, batch)
    st = prog.stencil
    raw_modes, faces, flat = _border_request(st, modes, constants)
    k = 1
    if not any(raw_modes):          # a torus: Periodic's default
      k = max(p.fused_iters for p in prog.module.passes)
    lo, hi = periodic_ghosts(st, k)
    desc = _border_desc(_periodic_desc(
        st.dim, self.extent, k, lo, hi, st.preserve_border, not_iterable),
                        raw_modes, flat)
    self._create(desc, [extend_resources], '%s with borders %s' % (
        'x'.join(map(str, self.extent)), ', '.join(self.modes)), faces)


# -- bordered domains, fused away from the walls -------------
def box_host(dst, src, boxes):
  """Copies boxes between two C-contiguous numpy arrays of one cell type and
  dimension count but different shapes (soda_hip_box_host, plain C++; no GPU
  needed).  `boxes`: (dst_origin, src_origin, size) each, dimension 0 (the LAST
  numpy axis) first; a box with a size of 0 is empty.  Returns `dst`."""
  import numpy as np
  for arr, write in ((dst, True), (src, False)):
    if not isinstance(arr, np.ndarray) or not arr.flags['C_CONTIGUOUS'] or \
        (write and not arr.flags['WRITEABLE']):
      raise util.InputError('box_host: C-contiguous numpy arrays, the '
                            'destination writable')
  dim = dst.ndim
  if src.ndim != dim or src.dtype != dst.dtype or not 1 <= dim <= MAX_DIM or \
      dst.dtype.itemsize not in (1, 2, 4, 8) or not dst.size or not src.size:
    raise util.InputError(
        'box_host: two arrays of one cell type of 1, 2, 4 or 8 bytes and of '
        '1 to %d dimensions' % MAX_DIM)
  if np.shares_memory(dst, src):
    raise util.InputError('box_host: the arrays overlap')
  boxes = [tuple(tuple(int(v) for v in part) for part in box) for box in boxes]
  if any(len(box) != 3 or any(len(part) != dim for part in box)
         for box in boxes):
    raise util.InputError('box_host: a box is (dst_origin, src_origin, size), '
                          '%d entries each' % dim)
  flat = lambda k: (ctypes.c_int32 * max(1, len(boxes) * dim))(
      *[v for box in boxes for v in box[k]])
  check(library().soda_hip_box_host(
      dst.ctypes.data, (ctypes.c_int32 * dim)(*dst.shape[::-1]),
      src.ctypes.data, (ctypes.c_int32 * dim)(*src.shape[::-1]),
      dst.dtype.itemsize, dim, len(boxes), flat(0), flat(1), flat(2)),
        'box_host')
  return dst


def box_resources(elem: int, dim: int):
  """(code object, kernel_resources of it) of the box module of a cell size
  and dimension count: JIT-built like every module, cached like them; needs
  no GPU."""
  from soda_amd.codegen.hip import box as _box
  return _helper_resources(_box, 'box', elem, dim)


def border_fused_ghosts(stencil: core.Stencil, modes, depth: int):
  """(reach_lo, reach_hi, ghost_lo, ghost_hi) of a fused bordered domain at
  `depth` >= 1: the reach of ONE iteration (periodic_ghosts(stencil, 1)), and
  a frame that wide in a wall dimension, `depth` times as wide in a `wrap`
  dimension.  Refuses (InputError) a program whose window of `depth`
  iterations exceeds `depth` times the window of one: the widths of the strips
  rest on that bound.  (Coupled outputs may reach less: the most over all
  outputs bounds every one of them.)"""
  raw = _border_modes(modes, stencil.dim)
  if depth < 1:
    raise util.InputError('border: depth < 1')
  rlo, rhi = periodic_ghosts(stencil, 1)
  for k in sorted({depth, 2}):
    klo, khi = periodic_ghosts(stencil, k)
    if any(a > k * r for a, r in zip(klo + khi, rlo + rhi)):
      raise util.InputError(
          'border: %d iterations of `%s` reach more than %d times what one '
          'reaches; fused borders are not served (depth=1 is)' % (
              k, stencil.app_name, k))
  lo = [r if m else depth * r for r, m in zip(rlo, raw)]
  hi = [r if m else depth * r for r, m in zip(rhi, raw)]
  return rlo, rhi, lo, hi


def _border_fused_desc(border: BorderDesc, depth: int, reach_lo,
                       reach_hi) -> BorderFusedDesc:
  desc = BorderFusedDesc()
  desc.border = border
  desc.depth = depth
  for d, (l, h) in enumerate(zip(reach_lo, reach_hi)):
    desc.reach_lo[d], desc.reach_hi[d] = l, h
  return desc


def _border_fused_info(raw: BorderFusedInfo, dim: int) -> dict:
  out = _periodic_info(raw.main, dim)
  out['depth'] = raw.depth
  out['scratch_bytes'] = int(raw.scratch_bytes)
  out['strips'] = []
  for s in raw.strip[:raw.num_strips]:
    strip = _periodic_info(s.info, dim)
    del strip['refill_every']
    strip.update(dim=s.dim, lo=s.lo, hi=s.hi, take_lo=s.take_lo,
                 take_hi=s.take_hi, extent=tuple(s.extent[:dim]))
    out['strips'].append(strip)
  return out


def border_fused_plan(plan: Plan, extent: Sequence[int], modes, depth: int,
                      reach_lo: Sequence[int], reach_hi: Sequence[int],
                      ghost_lo: Sequence[int], ghost_hi: Sequence[int],
                      iterate: int = 0, refill_every: int = 0,
                      preserve: bool = False, not_iterable: bool = False):
  """border_plan for the fused form (soda_hip_border_fused_plan; no GPU
  needed): (info, chunks), info as BorderedFused.info().  `depth` 0: the
  plan's deepest pass."""
  raw_modes, faces = _raw_faces(modes, plan.dim, reach_lo, reach_hi)
  desc = _border_fused_desc(_border_desc(_periodic_desc(
      plan.dim, extent, refill_every, ghost_lo, ghost_hi, preserve,
      not_iterable), raw_modes, ()), depth, reach_lo, reach_hi)
  raw, chunks = _plan_call('border_fused_plan', plan, desc, BorderFusedInfo(),
                           iterate, faces=faces)
  return _border_fused_info(raw, plan.dim), chunks


def border_fused_residual_boxes(plan: Plan, extent: Sequence[int], modes,
                                depth: int, reach_lo: Sequence[int],
                                reach_hi: Sequence[int],
                                ghost_lo: Sequence[int],
                                ghost_hi: Sequence[int],
                                preserve: bool = False,
                                not_iterable: bool = False) -> dict:
  """The partition of the domain by which a fused bordered handle counts a
  residual (soda_hip_border_fused_residual_boxes; no GPU needed; arguments as
  border_fused_plan): {'depth' as resolved, 'trusted': (lo, hi) in the padded
  coordinates of the domain, 'strips': [{'dim', 'low': (lo, hi), 'high': (lo,
  hi)}] in each strip's own padded coordinates}, dimension 0 first.  At depth
  1 and on a torus there are no strips and the trusted box is the domain."""
  raw_modes, faces = _raw_faces(modes, plan.dim, reach_lo, reach_hi)
  desc = _border_fused_desc(_border_desc(_periodic_desc(
      plan.dim, extent, 0, ghost_lo, ghost_hi, preserve, not_iterable),
                                         raw_modes, ()), depth, reach_lo,
                            reach_hi)
  raw = BorderFusedBoxes()
  if faces is None:
    status = library().soda_hip_border_fused_residual_boxes(
        ctypes.byref(plan), ctypes.byref(desc), ctypes.byref(raw))
  else:
    status = library().soda_hip_border_fused_residual_boxes_faces(
        ctypes.byref(plan), ctypes.byref(desc), ctypes.byref(faces),
        ctypes.byref(raw))
  check(status, 'border_fused_residual_boxes')
  dim = plan.dim
  box = lambda lo, hi: (tuple(lo[:dim]), tuple(hi[:dim]))
  return {'depth': raw.depth,
          'trusted': box(raw.trusted_lo, raw.trusted_hi),
          'strips': [{'dim': s.dim, 'low': box(s.lo[0], s.hi[0]),
                      'high': box(s.lo[1], s.hi[1])}
                     for s in raw.strip[:raw.num_strips]]}


class BorderedFused(Bordered):
  """Bordered, fused away from the walls (soda_hip_border_fused_create;
  DESIGN.md 4.13): a chunk of up to `depth` iterations is one fused run of the
  padded domain, mended along every wall by a narrow strip that advances one
  iteration at a time.  The bits are Bordered's, whatever the depth.  Made by
  `Program.bordered(..., depth=)`; close it before its program."""

  _entry = 'soda_hip_border_fused_'
  _what = 'border_fused'

  def __init__(self, prog: 'Program', extent: Sequence[int], modes,
               constants=None, depth: int = 0):
    """`depth`: iterations of a chunk; 0: the deepest fusion depth of the
    program, so that the interior of a chunk is one launch.  A program that
    fuses little gains little and may lose: the strips cost `depth` small
    launches and fills per wall dimension and chunk whatever the program fuses
    (DESIGN.md 4.13 has heat3d at depth 2).  info()['depth'] is the depth as
    resolved: 1, and Bordered's loop, where the program cannot iterate or a
    wall dimension is narrower than the two parts of its strip."""
    not_iterable = self._begin(prog, extent, modes)
    st = prog.stencil
    raw_modes, faces, flat = _border_request(st, modes, constants)
    depth = int(depth)
    if depth < 0:
      raise util.InputError('border: depth < 0')
    if not depth:
      depth = max(p.fused_iters for p in prog.module.passes)
    rlo, rhi, lo, hi = border_fused_ghosts(st, modes, depth)
    desc = _border_fused_desc(_border_desc(_periodic_desc(
        st.dim, self.extent, 0, lo, hi, st.preserve_border, not_iterable),
                                           raw_modes, flat),
                              depth, rlo, rhi)
    self._create(desc, [extend_resources, box_resources],
                 '%s with borders %s, fused %d deep' % (
                     'x'.join(map(str, self.extent)), ', '.join(self.modes),
                     depth), faces)

  def info(self) -> dict:
    """Bordered.info() of the handle on the domain, and: 'depth' as resolved,
    'strips' (per strip: dim, lo, hi, take_lo, take_hi, extent, ghost_lo,
    ghost_hi, padded, scratch_bytes), 'scratch_bytes' of all of them."""
    raw = BorderFusedInfo()
    check(self._fn('info')(self._handle, ctypes.byref(raw)),
          '%s: info' % self._what)
    return _border_fused_info(raw, self.prog.stencil.dim)

  def fill(self, arrays: Sequence[int], stream: int = 0) -> None:
    raise util.InputError('border_fused: no fill entry; Bordered has one')

  def _move(self, strip, gather, main_arrays, strip_arrays, stream):
    if len(main_arrays) != len(strip_arrays):
      raise util.InputError('border_fused: one strip array per main array')
    n = len(main_arrays)
    check(self._fn('move')(
        self._handle, strip, gather,
        (ctypes.c_void_p * max(1, n))(*main_arrays),
        (ctypes.c_void_p * max(1, n))(*strip_arrays), n,
        ctypes.c_void_p(stream)), '%s: move' % self._what)

  def gather(self, strip: int, strip_arrays: Sequence[int],
             main_arrays: Sequence[int], stream: int = 0) -> None:
    """The two rims of padded device arrays of info()['padded'] along the
    dimension of strip `strip` into the domain of padded arrays of the
    strip's extent (pair i: the cells of output i); asynchronous on
    `stream` (soda_hip_border_fused_move)."""
    self._move(strip, 1, main_arrays, strip_arrays, stream)

  def scatter(self, strip: int, main_arrays: Sequence[int],
              strip_arrays: Sequence[int], stream: int = 0) -> None:
    """The strip's rims, take_lo and take_hi cells wide, back into the two
    rims of the domain's padded arrays."""
    self._move(strip, 0, main_arrays, strip_arrays, stream)


class Program:
  """A SODA program JIT-built for gfx950 and loaded on one GPU."""

  def __init__(self, stencil: core.Stencil,
               opts: Optional[lower.LowerOptions] = None, device: int = 0,
               extent: Optional[Sequence[int]] = None,
               calibrate: Optional[bool] = None,
               source_prefix: str = ''):
    """`calibrate`: True -- time the passes on `extent` now; None (default) --
    the library does it by itself on the first run of an extent (a few ms,
    once; soda_hip_program_set_auto_calibrate); False -- never: runs are
    scheduled by the model.  `source_prefix`: text compiled in front of the
    module (diagnostic builds only: tests/test_compiler_pins.py switches a
    compiler-fault workaround of soda_rt.h off with a #define)."""
    self.stencil = stencil
    self._periodic = []         # Periodic handles over this program
    self.opts = resolve_options(stencil, opts, extent)   # never the caller's
    self.device = device
    self.module = lower.lower(stencil, self.opts)
    self.code = compile_source(source_prefix + self.module.source,
                               '%s.hip' % stencil.app_name)
    self.resources = kernel_resources(self.code)
    # launch geometry (chunk lengths, pass schedule) is the library's, decided
    # per run from the extent it is given and the register counts in the plan
    self.plan = make_plan(self.module, self.resources)
    if extent is not None:
      self.geometry(extent)            # fail early if it cannot run
    self._lib = library()
    self._handle = ctypes.c_void_p()
    check(
        self._lib.soda_hip_program_create(self.code, len(self.code),
                                          ctypes.byref(self.plan), device,
                                          ctypes.byref(self._handle)),
        'loading `%s` on GPU %d' % (stencil.app_name, device))
    if calibrate is False:
      check(self._lib.soda_hip_program_set_auto_calibrate(self._handle, 0),
            'set_auto_calibrate')
    if calibrate and extent is not None:
      self.calibrate(extent)

  # -- launch geometry ------------------------------------------------------
  def geometry(self, extent: Sequence[int], batch: int = 1):
    """What a run on `extent` -- on `batch` grids of it in one launch -- uses:
    ({kernel name: tile}, {fused iterations of a pass: modelled
    microseconds})."""
    if batch == 1:
      tiles, ns = plan_geometry(self.plan, extent)
    else:
      tiles, ns = plan_geometry_batch(self.plan, extent, batch)
    passes = self.module.sorted_passes()
    return ({k.name: t[:self.stencil.dim]
             for k, t in zip(self.module.kernels, tiles)},
            {p.fused_iters: v / 1e3 for p, v in zip(passes, ns)})

  def calibrate(self, extent: Sequence[int], launches: int = 4,
                stream: int = 0, batch: int = 1) -> Dict[int, float]:
    """Times one launch of every pass on `extent` -- on `batch` grids of it --
    on the GPU (a few ms, once) so that such runs are scheduled by the clock;
    returns {fused iterations: microseconds}."""
    ext = (ctypes.c_int32 * MAX_DIM)(*(list(extent) +
                                        [1] * (MAX_DIM - len(extent))))
    check(self._lib.soda_hip_program_calibrate_batch(self._handle, ext, batch,
                                                     launches,
                                                     ctypes.c_void_p(stream)),
          'calibrating `%s`' % self.stencil.app_name)
    return self.pass_times(extent, batch)[0]

  def pass_times(self, extent: Sequence[int], batch: int = 1):
    """({fused iterations: microseconds per launch}, measured?)"""
    ext = (ctypes.c_int32 * MAX_DIM)(*(list(extent) +
                                        [1] * (MAX_DIM - len(extent))))
    ns = (ctypes.c_float * self.plan.num_passes)()
    measured = ctypes.c_int32(0)
    check(self._lib.soda_hip_program_pass_times_batch(self._handle, ext, batch,
                                                      ns,
                                                      ctypes.byref(measured)),
          'pass_times')
    return ({p.fused_iters: v / 1e3
             for p, v in zip(self.module.sorted_passes(), ns)},
            bool(measured.value))

  def schedule(self, extent: Sequence[int], iterate: int,
               batch: int = 1) -> Dict[int, int]:
    """{fused iterations of a pass: launches} for `iterate` iterations (on
    `batch` grids per launch)."""
    ext = (ctypes.c_int32 * MAX_DIM)(*(list(extent) +
                                        [1] * (MAX_DIM - len(extent))))
    count = (ctypes.c_int32 * self.plan.num_passes)()
    check(self._lib.soda_hip_program_schedule_batch(self._handle, ext, batch,
                                                    iterate, count),
          'schedule')
    return {p.fused_iters: c
            for p, c in zip(self.module.sorted_passes(), count) if c}

  # -- lifecycle -----------------------------------------------------------
  def close(self) -> None:
    for per in list(getattr(self, '_periodic', ())):
      per.close()               # a handle goes before its program
    if getattr(self, '_norms', None) is not None:
      self._norms.close()
      self._norms = None
    if getattr(self, '_handle', None):
      self._lib.soda_hip_program_destroy(self._handle)
      self._handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  # -- checks shared by both entry points ----------------------------------
  def _check_extent(self, extent: Sequence[int]) -> None:
    if len(extent) != self.stencil.dim:
      raise util.InputError('extent must have %d entries' % self.stencil.dim)
    # (vector width and buffer-window limits are the library's to check:
    # soda_hip_plan_geometry, also behind every run entry of the C ABI)

  # -- device-resident arrays (the <app>_kernel analogue) ------------------
  def run_device(self, outputs: Sequence[int], inputs: Sequence[int],
                 extent: Sequence[int], iterate: Optional[int] = None,
                 stream: int = 0, origin: Optional[Sequence[int]] = None,
                 global_extent: Optional[Sequence[int]] = None,
                 keep: Optional[Sequence[int]] = None,
                 ghosts: Optional[Sequence[int]] = None,
                 sends: Optional[Sequence[int]] = None,
                 ghosts_ready: int = 0, sendable: int = 0,
                 batch: Optional[int] = None,
                 residual: Optional[int] = None,
                 box_iterate: Optional[int] = None,
                 norms: Optional[int] = None) -> None:
    """`outputs` / `inputs` are device addresses (e.g. tensor.data_ptr()) of
    dense dim-0-fastest arrays; asynchronous on `stream`.  `inputs` holds the
    input tensors followed by the program's `param` arrays (C order).
    The addresses must keep the device entry contract (include/soda_hip.h):
    no output overlaps an input, a param array or another output, and every
    input and output is aligned to min(16, vec x cell size) bytes -- `vec` the
    widest cells-per-lane of the module's kernels (tune['vec'], follows
    extent[0]: 4 float cells and 16 bytes where the row length allows, one cell
    and 4 bytes for an odd one) -- a param array to its cell size.  A call that
    breaks either is refused (BackendError, "nothing was launched"); a view or
    slice of a torch tensor has to be checked against this, `.contiguous()` is
    not enough for one that starts mid-row.  For a
    slab of a larger grid pass where its cell 0 sits (`origin`) and the size of
    the whole grid (`global_extent`): `border: preserve` means the GLOBAL border.
    `keep` = (lo, hi): only cells [lo, hi) along the last dimension of the
    result are needed (a slab's own rows); passes then skip the rows nothing
    can carry into that range any more (soda_hip_run_device_cone).  NOTE: the
    last pass still writes up to `fused iterations x reach` rows on either
    side of [lo, hi) -- computed with zeros where the launch ended, i.e. wrong
    -- and leaves the rows beyond those untouched: outside [lo, hi) the output
    arrays are unspecified, not "unchanged".
    With `keep`, a halo exchange can run underneath (soda_hip_run_device_slab):
    `ghosts` = (lo, hi) rows at either end of the INPUT arrays that an exchange
    on another stream is writing, complete when the hipEvent_t `ghosts_ready`
    fires; `sends` = (lo, hi) rows at either end of the kept range the
    neighbours fetch next, complete when `sendable` (recorded by this call)
    fires.
    `batch` = N: every input and output holds N independent grids of `extent`,
    one behind the other like a contiguous [N, ...] array (the param arrays
    are shared), and one launch per kernel runs them all
    (soda_hip_run_device_batch).  Needs a program built with
    LowerOptions.batch; not together with `keep` / `ghosts` / `sends` /
    `origin`.
    Streams, scratch, graphs (include/soda_hip.h has the full text): every
    kernel, fill and copy of a call is enqueued on `stream`, in order, and the
    side stream of a split pass joins it again inside the call.  Two kinds of
    call wait for the GPU: the first run of more than one iteration on an
    extent of a program that calibrates by itself (`calibrate=None`), and a
    call that grows the program's scratch -- a larger extent or batch, the
    first `keep` run of three passes or more (`scratch()` tells).  A Program
    is one queue of work: calls on one stream need nothing, a call on another
    stream has to be ordered behind the earlier ones by the caller (an event),
    and two streams may not run one Program at once.  Under
    `torch.cuda.graph` a call never calibrates and never allocates; if scratch
    would have to grow it is refused (BackendError, "nothing was launched")
    and the capture stays valid.  So: run the call once eagerly with the same
    extent, iterate, batch and keep range -- `calibrate()` first if the clock
    is to pick the schedule -- then capture.  The graph holds the addresses of
    the scratch: replay it only until a later call grows that scratch or the
    Program is closed.  Runs with `ghosts_ready` / `sendable` are not meant
    for capture.
    `residual` = the device address of 32 bytes (8-byte aligned): the run also
    leaves there how much its LAST iteration changed the grid
    (soda_hip_run_device_residual; `residual()` reads and decodes them).  The
    struct is zeroed on `stream` inside the call; the run stays asynchronous
    and can be captured like any other.  Needs a program built with
    LowerOptions.residual.  Together with `origin` / `global_extent` / `keep`
    / `ghosts` / `sends` the struct is the SLAB's share
    (soda_hip_run_device_slab_residual): the cells of `residual_box(...,
    origin=, global_extent=, keep=)` at `box_iterate` -- the iterations the
    state has seen since its inputs were the caller's (default: `iterate`; no
    less) -- ghost rows of the result not among them; the shares of all slabs
    add up (counts) and take the larger (maxima).  A last pass split around
    the exchange completes the struct with its interior part, behind
    `sendable`.  Not together with `batch`.
    `norms` = the device address of a soda_hip_norms_t (840 bytes, 8-byte
    aligned; ctypes.sizeof(NormsStruct)): the run also leaves there the exact
    sums of |d| and d^2 over the deltas of its LAST iteration
    (soda_hip_run_device_norms; `norms().fetch(ptr)` reads them,
    `norms_value` rounds them).  The run ends in the one-iteration pass, then
    the struct is zeroed and filled on `stream`: asynchronous and capturable
    like a `residual` run.  Needs a program built with LowerOptions.residual
    whose tensors all have one cell type.  Whole grids only: not together with
    `residual`, `batch`, `origin` / `keep` / `ghosts` / `sends`."""
    st = self.stencil
    iterate = st.iterate if iterate is None else iterate
    self._check_extent(extent)
    if len(outputs) != len(st.output_names) or len(inputs) != len(
        st.input_names) + len(st.param_stmts):
      raise util.InputError('wrong number of tensors')
    exchange = ghosts is not None or sends is not None or bool(
        ghosts_ready or sendable)
    slab = exchange or keep is not None or origin is not None or \
        global_extent is not None
    if norms is not None and (residual is not None or batch is not None or
                              slab or box_iterate is not None):
      raise util.InputError(
          'run_device: norms are taken on whole grids: not together with '
          'residual / batch / keep / ghosts / sends / origin')
    if residual is not None and batch is not None:
      raise util.InputError(
          'run_device: no residual of a batch (a residual per item is a '
          'reduction of its own)')
    if batch is not None and slab:
      raise util.InputError(
          'run_device: a batched run is a run on whole grids: no keep / '
          'ghosts / sends / origin')
    if residual is not None and not slab and box_iterate is not None and \
        int(box_iterate) != iterate:
      raise util.InputError(
          'run_device: box_iterate is for a slab run (origin / keep / '
          'ghosts / sends)')
    lib = self._lib
    outs = (ctypes.c_void_p * len(outputs))(*outputs)
    ins = (ctypes.c_void_p * len(inputs))(*inputs)
    ext = (ctypes.c_int32 * len(extent))(*extent)
    org = (ctypes.c_int32 * len(extent))(*(origin or [0] * len(extent)))
    gext = (ctypes.c_int32 * len(extent))(*(global_extent or extent))
    whole = (0, extent[-1])
    if slab:
      reach_lo, reach_hi = st.reach_along(st.dim - 1)
      keep_lo, keep_hi = keep if keep is not None else whole
      run = SlabRun(int(keep_lo), int(keep_hi), reach_lo, reach_hi,
                    *(int(v) for v in (ghosts or (0, 0))),
                    *(int(v) for v in (sends or (0, 0))),
                    ghosts_ready or None, sendable or None)
    window = (self._handle, outs, ins, ext, org, gext, iterate)
    on = ctypes.c_void_p(stream)
    what = 'running `%s`' % st.app_name
    # the entry of the C ABI the arguments ask for
    if norms is not None:
      entry, what = lib.soda_hip_run_device_norms, what + ' with norms'
      args = (self._handle, self.norms()._handle, outs, ins, ext, iterate,
              ctypes.c_void_p(norms), on)
    elif residual is not None and slab:
      entry = lib.soda_hip_run_device_slab_residual
      what += ' on a slab with a residual'
      args = window + (iterate if box_iterate is None else int(box_iterate),
                       ctypes.byref(run), ctypes.c_void_p(residual), on)
    elif residual is not None:
      entry, what = lib.soda_hip_run_device_residual, what + ' with a residual'
      args = (self._handle, outs, ins, ext, iterate,
              ctypes.c_void_p(residual), on)
    elif batch is not None:
      entry = lib.soda_hip_run_device_batch
      what += ' on a batch of %d' % batch
      args = (self._handle, outs, ins, ext, int(batch), iterate, on)
    elif exchange:
      entry = lib.soda_hip_run_device_slab
      args = window + (ctypes.byref(run), on)
    elif keep is not None and tuple(keep) != whole:
      entry = lib.soda_hip_run_device_cone
      args = window + (run.keep_lo, run.keep_hi, reach_lo, reach_hi, on)
    else:
      entry, args = lib.soda_hip_run_device_window, window + (on,)
    check(entry(*args), what)

  def residual(self, ptr: int, stream: int = 0) -> Residual:
    """The struct a `run_device(..., residual=ptr)` left at device address
    `ptr`, decoded.  Copies the 32 bytes on `stream` and waits for them."""
    raw = ResidualStruct()
    check(self._lib.soda_hip_memcpy_d2h(ctypes.byref(raw), ctypes.c_void_p(ptr),
                                        ctypes.sizeof(raw),
                                        ctypes.c_void_p(stream)),
          'residual: copy out')
    check(self._lib.soda_hip_stream_synchronize(ctypes.c_void_p(stream)),
          'residual: synchronize')
    return Residual.from_struct(raw)

  def norms(self) -> Norms:
    """The norms kernels that fit this program (one per Program, made on first
    use, closed with it): its cell type, its dimension count, its GPU.
    util.InputError for a program of mixed cell types: one accumulator holds
    one kind of units."""
    if getattr(self, '_norms', None) is None:
      st = self.stencil
      types = {t.c_type for t in list(st.input_types) + list(st.output_types)}
      if len(types) != 1:
        raise util.InputError(
            'norms: the tensors of `%s` have cells of types %s; one '
            'accumulator holds one kind of units' %
            (st.app_name, ', '.join(sorted(types))))
      self._norms = Norms(types.pop(), st.dim, self.device)
    return self._norms

  def last_residual(self):
    """How the last `run_device(..., residual=)` took its residual: ('twin' |
    'generic' | None, fusion depth of the pass launched last)."""
    mode, fused = ctypes.c_int32(), ctypes.c_int32()
    check(self._lib.soda_hip_last_residual(self._handle, ctypes.byref(mode),
                                           ctypes.byref(fused)),
          'last_residual')
    return {0: None, 1: 'twin', 2: 'generic'}[mode.value], fused.value

  def residual_box(self, extent: Sequence[int], iterate: int,
                   origin: Optional[Sequence[int]] = None,
                   global_extent: Optional[Sequence[int]] = None,
                   keep: Optional[Sequence[int]] = None):
    """[(lo, hi)] per output: the cells a residual over `iterate` iterations
    on `extent` counts, as the library derives them from the plan.  With
    `origin` / `global_extent` / `keep`: the cells a SLAB counts, in the
    coordinates of its arrays -- the global grid's box cut to the rows `keep`
    = (lo, hi) of the slab's last dimension
    (soda_hip_plan_residual_slab_box)."""
    return plan_residual_box(self.plan, extent, iterate, origin, global_extent,
                             keep)

  def run_until(self, inputs: Dict[str, 'numpy.ndarray'], tol: float,
                max_iterate: int, check_every: int = 8, int_tol: int = 0,
                norm: Optional[str] = None):
    """Iterates on numpy arrays until converged: `check_every` iterations at a
    time, stopping when the last iteration's residual has `unordered == 0`,
    `max_float <= tol` and `max_int <= int_tol`, or after `max_iterate`
    iterations (soda_hip_run_device_until; synchronous).  Returns (outputs,
    iterations done, Residual).  Like `run`, the outputs start as zeros and
    only each output's valid box after the iterations done is written; the
    input arrays are not touched.  Needs a program built with
    LowerOptions.residual.
    `norm` = 'l1' | 'l2': stop on the exact norm of the last iteration's
    deltas instead -- `unordered == 0`, `infinite == 0` and sum |d| <= tol
    ('l1') or sqrt(sum d^2) <= tol ('l2'), the sums rounded once
    (soda_hip_run_device_until_norm); the third value returned is then the
    NormsStruct of the last chunk and `int_tol` is not used.  None: the rule
    above, exactly as before."""
    import numpy as np
    if norm not in (None, 'l1', 'l2'):
      raise util.InputError("run_until: norm is None, 'l1' or 'l2'")
    norms = self.norms() if norm is not None else None
    st = self.stencil
    lib = self._lib
    first = np.asarray(inputs[st.input_names[0]])
    extent = tuple(first.shape[::-1])
    self._check_extent(extent)
    host_in = _host_inputs(st, inputs, first.shape)
    dense = [np.empty(first.shape, dtype=np.dtype(t.np_name))
             for t in st.output_types]
    raw = ResidualStruct() if norm is None else NormsStruct()
    done = ctypes.c_int32(0)
    with _staged(lib, self.device, host_in, dense, 'run_until') as (dev_in,
                                                                     dev_out):
      outs = (ctypes.c_void_p * len(dev_out))(*dev_out)
      ins = (ctypes.c_void_p * len(dev_in))(*dev_in)
      ext = (ctypes.c_int32 * len(extent))(*extent)
      if norm is None:
        check(
            lib.soda_hip_run_device_until(self._handle, outs, ins, ext,
                                          int(max_iterate), int(check_every),
                                          float(tol), int(int_tol),
                                          ctypes.byref(raw), ctypes.byref(done),
                                          None),
            'running `%s` until converged' % st.app_name)
      else:
        check(
            lib.soda_hip_run_device_until_norm(
                self._handle, norms._handle, outs, ins, ext, int(max_iterate),
                int(check_every), {'l1': NORMS_L1, 'l2': NORMS_L2}[norm],
                float(tol), ctypes.byref(raw), ctypes.byref(done), None),
            'running `%s` until its %s norm is small' % (st.app_name, norm))
      _copy_out(lib, dense, dev_out, 'run_until')
      check(lib.soda_hip_stream_synchronize(None), 'run_until: synchronize')
    return (_valid_boxes(st, extent, done.value, dense), done.value,
            Residual.from_struct(raw) if norm is None else raw)

  def last_split(self) -> int:
    """Passes of the last run launched in two parts around a halo exchange."""
    n = ctypes.c_int32()
    check(self._lib.soda_hip_last_split(self._handle, ctypes.byref(n)),
          'last_split')
    return n.value

  def scratch(self):
    """(device bytes of scratch the program holds, times a call replaced one of
    its buffers by a larger one -- each a call that waited for the device)."""
    n, grown = ctypes.c_int64(), ctypes.c_int32()
    check(self._lib.soda_hip_program_scratch(self._handle, ctypes.byref(n),
                                             ctypes.byref(grown)), 'scratch')
    return n.value, grown.value

  def last_rows(self) -> int:
    """Cells along the last dimension the passes of the last run covered,
    summed over the passes."""
    n = ctypes.c_int64()
    check(self._lib.soda_hip_last_rows(self._handle, ctypes.byref(n)),
          'last_rows')
    return n.value

  def set_debug_buffer(self, ptr: int) -> None:
    """Device buffer the time stamps of `stamps=True` kernels go to."""
    check(self._lib.soda_hip_program_set_debug_buffer(self._handle,
                                                      ctypes.c_void_p(ptr)),
          'set_debug_buffer')

  def last_launches(self):
    a, b = ctypes.c_int32(), ctypes.c_int32()
    check(self._lib.soda_hip_last_launches(self._handle, ctypes.byref(a),
                                           ctypes.byref(b)), 'last_launches')
    return a.value, b.value

  # -- host arrays (the soda::app::<app> analogue) -------------------------
  def run(self, inputs: Dict[str, 'numpy.ndarray'],
          iterate: Optional[int] = None,
          outputs: Optional[Dict[str, 'numpy.ndarray']] = None
          ) -> Dict[str, 'numpy.ndarray']:
    """numpy in, numpy out.  Array shape is extent reversed (dim 0 fastest =
    last axis).  Only the valid box of each output is written, the rest keeps
    what the caller's array held (zeros for arrays allocated here)."""
    import numpy as np
    st = self.stencil
    iterate = st.iterate if iterate is None else iterate
    first = inputs[st.input_names[0]]
    extent = tuple(first.shape[::-1])
    self._check_extent(extent)
    dim = st.dim
    keep = []
    in_list = [_host_tensor(np.asarray(inputs[n]), t.np_name, first.shape, dim,
                            keep)
               for n, t in zip(st.input_names, st.input_types)]
    for pstmt in st.param_stmts:        # param arrays follow, C order
      arr = _host_param(st, inputs, pstmt)
      keep.append(arr)
      in_list.append(HostTensor(arr.ctypes.data, None, None, None))
    ins = (HostTensor * len(in_list))(*in_list)
    result = {}
    for n, t in zip(st.output_names, st.output_types):
      if outputs is not None and n in outputs:
        result[n] = outputs[n]
      else:
        result[n] = np.zeros(first.shape, dtype=np.dtype(t.np_name))
    outs = (HostTensor * len(st.output_names))(*[
        _host_tensor(result[n], t.np_name, first.shape, dim, keep)
        for n, t in zip(st.output_names, st.output_types)
    ])
    lo, hi = [], []
    for n in st.output_names:
      l, h = clipped_box(st.valid_box(extent, n, iterate), extent)
      lo.extend(l)
      hi.extend(h)
    vlo = (ctypes.c_int32 * len(lo))(*lo)
    vhi = (ctypes.c_int32 * len(hi))(*hi)
    check(
        self._lib.soda_hip_run_host_box(self._handle, ins, outs, iterate, vlo,
                                        vhi), 'running `%s`' % st.app_name)
    return result

  # -- periodic domains ------------------------------------------------------
  def periodic(self, extent: Sequence[int],
               refill_every: Optional[int] = None,
               ghosts: Optional[Sequence[Sequence[int]]] = None,
               batch: Optional[int] = None) -> Periodic:
    """This program on a torus of `extent` (runtime.Periodic)
    -- `batch` = N: on N tori at once, every array [N, ...] (DESIGN.md 4.15;
    needs a program built with LowerOptions.batch).  The handle is closed
    with the program at the latest."""
    return Periodic(self, extent, refill_every, ghosts, batch)

  def run_periodic(self, inputs: Dict[str, 'numpy.ndarray'],
                   iterate: Optional[int] = None,
                   refill_every: Optional[int] = None
                   ) -> Dict[str, 'numpy.ndarray']:
    """`run` on a torus: numpy arrays of the domain in (shape = extent
    reversed; params as in `run`), the outputs out, EVERY cell of them
    defined.  A plain allocate / copy in / Periodic.run_device / copy out."""
    return self._run_domain(lambda extent: self.periodic(extent, refill_every),
                            'run_periodic', inputs, iterate)

  # -- bordered domains ------------------------------------------------------
  def bordered(self, extent: Sequence[int], modes, constants=None,
               depth: int = 1, batch: Optional[int] = None) -> Bordered:
    """This program on a domain of `extent` with a border mode per dimension
    (runtime.Bordered).  `depth` other than 1: fused away from
    the walls in chunks of `depth` iterations, 0 for the program's deepest
    (runtime.BorderedFused) -- the same bits, faster where the
    program fuses deep.  `batch` = N: on N domains at once, every array
    [N, ...] (needs a program built with LowerOptions.batch;
    the fused form has no batch: with `depth` other than 1 the library's
    refusal of a batched plan is raised).  A dimension's entry of `modes` may
    be a (low, high) pair or 'low/high', a constant a sequence of one entry
    per dimension, each a scalar or a (low, high) pair: a mode and a constant
    per face, here and in every run_bordered* method.  The
    handle is closed with the program at the latest."""
    if depth == 1:
      return Bordered(self, extent, modes, constants, batch)
    if batch is not None and not self.plan.batched:
      raise util.InputError('bordered: `batch` needs a program built with '
                            'LowerOptions.batch')
    return BorderedFused(self, extent, modes, constants, depth)

  def run_bordered(self, inputs: Dict[str, 'numpy.ndarray'], modes,
                   constants=None, iterate: Optional[int] = None,
                   depth: int = 1) -> Dict[str, 'numpy.ndarray']:
    """`run` with borders: numpy arrays of the domain in, the outputs out,
    EVERY cell of them defined -- each iteration sees its inputs extended by
    `modes` (one name, or one per dimension, dimension 0 first) and
    `constants` (a scalar or {input: scalar}; default zero).  A plain allocate
    / copy in / Bordered.run_device / copy out.  `depth`: as for `bordered`."""
    return self._run_domain(
        lambda extent: self.bordered(extent, modes, constants, depth),
        'run_bordered', inputs, iterate)

  def _run_domain(self, handle_of, what, inputs, iterate):
    """run's numpy plumbing around `handle_of(extent)`.run_device; the handle
    is made once the inputs are checked, and closed here."""
    import numpy as np
    st = self.stencil
    lib = self._lib
    iterate = st.iterate if iterate is None else iterate
    first = np.asarray(inputs[st.input_names[0]])
    extent = tuple(first.shape[::-1])
    self._check_extent(extent)
    host_in = _host_inputs(st, inputs, first.shape)
    result = {n: np.empty(first.shape, dtype=np.dtype(t.np_name))
              for n, t in zip(st.output_names, st.output_types)}
    dense = list(result.values())
    with handle_of(extent) as dom, \
        _staged(lib, self.device, host_in, dense, what,
                synchronize=True) as (dev_in, dev_out):
      dom.run_device(dev_out, dev_in, iterate)
      _copy_out(lib, dense, dev_out, what)
    return result

  def _run_domain_until(self, handle, what, inputs, tol, max_iterate,
                        check_every, int_tol, norm):
    """run_until's numpy plumbing around `handle`.run_until (which is closed
    here)."""
    import numpy as np
    st = self.stencil
    lib = self._lib
    first = np.asarray(inputs[st.input_names[0]])
    host_in = _host_inputs(st, inputs, first.shape)
    result = {n: np.empty(first.shape, dtype=np.dtype(t.np_name))
              for n, t in zip(st.output_names, st.output_types)}
    dense = list(result.values())
    with handle as dom, _staged(lib, self.device, host_in, dense, what,
                                synchronize=True) as (dev_in, dev_out):
      done, last = dom.run_until(dev_out, dev_in, tol, max_iterate,
                                 check_every, int_tol, norm)
      _copy_out(lib, dense, dev_out, what)
    return result, done, last

  def run_periodic_until(self, inputs: Dict[str, 'numpy.ndarray'], tol: float,
                         max_iterate: int, check_every: int = 8,
                         int_tol: int = 0, norm: Optional[str] = None,
                         refill_every: Optional[int] = None):
    """`run_until` on a torus: numpy arrays of the domain in; returns (outputs,
    iterations done, Residual -- or NormsStruct with `norm`), EVERY cell of
    the outputs defined and every cell of the domain counted
    (Periodic.run_until)."""
    import numpy as np
    extent = tuple(np.asarray(inputs[self.stencil.input_names[0]]).shape[::-1])
    if norm not in (None, 'l1', 'l2'):
      raise util.InputError("run_until: norm is None, 'l1' or 'l2'")
    return self._run_domain_until(
        self.periodic(extent, refill_every), 'run_periodic_until', inputs, tol,
        max_iterate, check_every, int_tol, norm)

  def run_bordered_until(self, inputs: Dict[str, 'numpy.ndarray'], modes,
                         tol: float, max_iterate: int, constants=None,
                         depth: int = 1, check_every: int = 8,
                         int_tol: int = 0, norm: Optional[str] = None):
    """`run_until` with borders (`modes`, `constants`, `depth` as for
    `run_bordered`): returns (outputs, iterations done, Residual -- or
    NormsStruct with `norm`), EVERY cell of the outputs defined and every cell
    of the domain counted (Bordered.run_until)."""
    import numpy as np
    extent = tuple(np.asarray(inputs[self.stencil.input_names[0]]).shape[::-1])
    if norm not in (None, 'l1', 'l2'):
      raise util.InputError("run_until: norm is None, 'l1' or 'l2'")
    return self._run_domain_until(
        self.bordered(extent, modes, constants, depth), 'run_bordered_until',
        inputs, tol, max_iterate, check_every, int_tol, norm)

  def run_batch(self, inputs: Dict[str, 'numpy.ndarray'],
                iterate: Optional[int] = None) -> Dict[str, 'numpy.ndarray']:
    """`run` on N independent grids in one launch per kernel: numpy arrays of
    shape (N,) + extent reversed in, the same out; params as in `run`, shared
    by all items.  A plain allocate / copy in / run_device(batch=N) / copy out
    through the library's own memory calls (not the banded host path).  Like
    `run`, the outputs start as zeros and only each item's valid box is
    written.  Needs a program built with LowerOptions.batch."""
    import numpy as np
    st = self.stencil
    lib = self._lib
    iterate = st.iterate if iterate is None else iterate
    first = np.asarray(inputs[st.input_names[0]])
    if first.ndim != st.dim + 1 or first.shape[0] < 1:
      raise util.InputError('run_batch: arrays of shape (N,) + extent[::-1]')
    batch = int(first.shape[0])
    extent = tuple(first.shape[:0:-1])
    self._check_extent(extent)
    host_in = _host_inputs(st, inputs, first.shape)
    dense = [np.empty(first.shape, dtype=np.dtype(t.np_name))
             for t in st.output_types]
    with _staged(lib, self.device, host_in, dense, 'run_batch') as (dev_in,
                                                                     dev_out):
      self.run_device(dev_out, dev_in, extent, iterate, batch=batch)
      _copy_out(lib, dense, dev_out, 'run_batch')
    return _valid_boxes(st, extent, iterate, dense, batched=True)

  # -- batched domains ---------------------------------------
  def run_periodic_batch(self, inputs: Dict[str, 'numpy.ndarray'],
                         iterate: Optional[int] = None,
                         refill_every: Optional[int] = None
                         ) -> Dict[str, 'numpy.ndarray']:
    """`run_periodic` on N independent tori in one launch per kernel: numpy
    arrays of shape (N,) + extent reversed in, the same out, EVERY cell of
    every item defined; params as in `run`, shared by all items.  Needs a
    program built with LowerOptions.batch."""
    return self._run_domain_batch(
        lambda extent, n: self.periodic(extent, refill_every, batch=n),
        'run_periodic_batch', inputs, iterate)

  def run_bordered_batch(self, inputs: Dict[str, 'numpy.ndarray'], modes,
                         constants=None, iterate: Optional[int] = None
                         ) -> Dict[str, 'numpy.ndarray']:
    """`run_bordered` on N independent domains in one launch per kernel: numpy
    arrays of shape (N,) + extent reversed in, the same out, EVERY cell of
    every item defined -- each item extended by `modes` and `constants` on its
    own.  Needs a program built with LowerOptions.batch."""
    return self._run_domain_batch(
        lambda extent, n: self.bordered(extent, modes, constants, batch=n),
        'run_bordered_batch', inputs, iterate)

  def _run_domain_batch(self, handle_of, what, inputs, iterate):
    """run_batch's numpy plumbing around `handle_of(extent, N)`.run_device; the
    handle is made once the inputs are checked, and closed here."""
    import numpy as np
    st = self.stencil
    lib = self._lib
    iterate = st.iterate if iterate is None else iterate
    first = np.asarray(inputs[st.input_names[0]])
    if first.ndim != st.dim + 1 or first.shape[0] < 1:
      raise util.InputError('%s: arrays of shape (N,) + extent[::-1]' % what)
    extent = tuple(first.shape[:0:-1])
    self._check_extent(extent)
    host_in = _host_inputs(st, inputs, first.shape)
    result = {n: np.empty(first.shape, dtype=np.dtype(t.np_name))
              for n, t in zip(st.output_names, st.output_types)}
    dense = list(result.values())
    with handle_of(extent, int(first.shape[0])) as dom, \
        _staged(lib, self.device, host_in, dense, what,
                synchronize=True) as (dev_in, dev_out):
      dom.run_device(dev_out, dev_in, iterate)
      _copy_out(lib, dense, dev_out, what)
    return result


def _host_param(st, inputs, pstmt):
  """The param array of `pstmt` among `inputs`, contiguous and flat (C
  order)."""
  import numpy as np
  arr = np.ascontiguousarray(inputs[pstmt.name]).reshape(-1)
  if arr.dtype != np.dtype(pstmt.haoda_type.np_name) or \
      arr.size != st.param_elems(pstmt):
    raise util.InputError('param %s must be %d x %s' % (
        pstmt.name, st.param_elems(pstmt), pstmt.haoda_type.np_name))
  return arr


def _host_inputs(st, inputs, shape):
  """What a staged run copies in, contiguous: the input tensors of `inputs`,
  each of `shape`, then the param arrays (C order)."""
  import numpy as np
  host_in = []
  for n, t in zip(st.input_names, st.input_types):
    arr = np.ascontiguousarray(inputs[n])
    if arr.dtype != np.dtype(t.np_name):
      raise util.InputError('expected dtype %s, got %s' % (t.np_name,
                                                           arr.dtype))
    if arr.shape != shape:
      raise util.InputError('all tensors must share one shape')
    host_in.append(arr)
  return host_in + [_host_param(st, inputs, p) for p in st.param_stmts]


@contextlib.contextmanager
def _staged(lib, device: int, host_in, host_out, what: str,
            synchronize: bool = False):
  """Device arrays for the numpy arrays `host_in` (copied in) and `host_out`
  (not touched): yields (input addresses, output addresses) and frees them all
  on the way out -- `synchronize`: behind a wait for the null stream.  `what`
  names the caller in the error texts."""
  dev_in, dev_out = [], []
  try:
    for arr in host_in:
      ptr = ctypes.c_void_p()
      check(lib.soda_hip_malloc(device, arr.nbytes, ctypes.byref(ptr)),
            what + ': allocating an input')
      dev_in.append(ptr)
      check(lib.soda_hip_memcpy_h2d(ptr, arr.ctypes.data, arr.nbytes, None),
            what + ': copy in')
    for arr in host_out:
      ptr = ctypes.c_void_p()
      check(lib.soda_hip_malloc(device, arr.nbytes, ctypes.byref(ptr)),
            what + ': allocating an output')
      dev_out.append(ptr)
    yield [p.value for p in dev_in], [p.value for p in dev_out]
  finally:
    if synchronize:
      lib.soda_hip_stream_synchronize(None)
    for ptr in dev_in + dev_out:
      lib.soda_hip_free(device, ptr)


def _copy_out(lib, host_out, dev_out, what: str) -> None:
  for arr, ptr in zip(host_out, dev_out):
    check(lib.soda_hip_memcpy_d2h(arr.ctypes.data, ctypes.c_void_p(ptr),
                                  arr.nbytes, None), what + ': copy out')


def _valid_boxes(st, extent, iterate: int, dense, batched: bool = False):
  """{output name: zeros, but for the output's valid box after `iterate`
  iterations, which is taken from its array in `dense`}.  `batched`: the
  arrays have a leading axis of items, each cut alike."""
  import numpy as np
  result = {}
  for n, arr in zip(st.output_names, dense):
    lo, hi = clipped_box(st.valid_box(extent, n, iterate), extent)
    box = tuple(slice(l, h) for l, h in zip(lo, hi))[::-1]
    if batched:
      box = (slice(None),) + box
    result[n] = np.zeros_like(arr)
    result[n][box] = arr[box]
  return result


def _host_tensor(arr, np_name: str, shape, dim: int, keep: list):
  """HostTensor for a numpy array (shape = extent reversed), keeping the ctypes
  arrays it points to alive in `keep`."""
  import numpy as np
  if arr.dtype != np.dtype(np_name):
    raise util.InputError('expected dtype %s, got %s' % (np_name, arr.dtype))
  if tuple(arr.shape) != tuple(shape):
    raise util.InputError('all tensors must share one shape')
  item = arr.dtype.itemsize
  strides = [b // item for b in arr.strides[::-1]]
  if any(v * item != b for v, b in zip(strides, arr.strides[::-1])):
    raise util.InputError('strides must be whole elements')
  ext = (ctypes.c_int32 * dim)(*shape[::-1])
  strd = (ctypes.c_int32 * dim)(*strides)
  mn = (ctypes.c_int32 * dim)(*([0] * dim))
  keep.extend((ext, strd, mn, arr))
  return HostTensor(arr.ctypes.data, ext, strd, mn)


class Group:
  """A SODA program on N GPUs driven by one host thread: the grid cut into
  slabs along the streamed dimension, halo exchange by peer copies hidden under
  the compute (soda_hip_group_*, include/soda_hip.h).  `devices` may name one
  GPU several times ("virtual devices"): the whole N-slab schedule then runs on
  that GPU -- how a one-GPU box tests it."""

  def __init__(self, stencil: core.Stencil, extent: Sequence[int],
               devices: Sequence[int],
               opts: Optional[lower.LowerOptions] = None,
               iterate: Optional[int] = None, exchange_every: int = 0,
               overlap: bool = True, calibrate: bool = False,
               threads: Optional[bool] = None):
    """`threads`: one enqueueing thread per slab inside the library (default:
    when the slabs sit on more than one GPU)."""
    self.stencil = stencil
    self.extent = tuple(int(e) for e in extent)
    self.devices = tuple(int(d) for d in devices)
    if len(self.extent) != stencil.dim:
      raise util.InputError('extent must have %d entries' % stencil.dim)
    if not 1 <= len(self.devices) <= MAX_SLABS:
      raise util.InputError('1 to %d slabs' % MAX_SLABS)
    iterate = stencil.iterate if iterate is None else iterate
    n = len(self.devices)
    reach_lo, reach_hi = stencil.reach_along(stencil.dim - 1)
    desc = GroupDesc()
    desc.num_slabs = n
    for i, d in enumerate(self.devices):
      desc.device[i] = d
    for i, e in enumerate(self.extent):
      desc.extent[i] = e
    desc.reach_lo, desc.reach_hi = reach_lo, reach_hi
    desc.iterate = iterate
    desc.exchange_every = exchange_every
    if threads is None:
      threads = len(set(self.devices)) > 1
    desc.flags = (0 if overlap else GROUP_NO_OVERLAP) | (
        GROUP_CALIBRATE if calibrate else 0) | (
            GROUP_THREADS if threads else 0)
    self._lib = library()
    # The kernels are shaped for the extent of a slab (row-covering blocks,
    # how much warm-up to peel); a slab's extent depends on the exchange
    # interval, which the library picks from the plan's pass times: lower once
    # for the own rows, ask, lower again for the rows really held.
    own = self.extent[-1] // n
    every = ctypes.c_int32(exchange_every)
    local = self.extent[:-1] + (max(1, own),)
    for _ in range(2):
      self.opts = resolve_options(stencil, opts, local)
      self.module = lower.lower(stencil, self.opts)
      self.code = compile_source(self.module.source,
                                 '%s.hip' % stencil.app_name)
      self.resources = kernel_resources(self.code)
      self.plan = make_plan(self.module, self.resources)
      check(self._lib.soda_hip_group_plan(ctypes.byref(self.plan),
                                          ctypes.byref(desc),
                                          ctypes.byref(every)),
            'slabs of `%s`' % stencil.app_name)
      ghosts = (reach_lo + reach_hi if n > 2 else max(reach_lo, reach_hi)
                if n > 1 else 0) * every.value
      grown = self.extent[:-1] + (own + ghosts,)
      if grown == local:
        break
      local = grown
    # The model's interval shaped the kernels.  With calibrate=True and no
    # interval of the caller's, create is handed 0 so that the LIBRARY times
    # the model's best candidates on a middle slab's GPU and lets the clock
    # pick (soda_hip_group_create: exchange_every == 0 && GROUP_CALIBRATE);
    # the kernels run on any extent, only their peel / chunk choices were made
    # for the model's one.
    desc.exchange_every = 0 if (calibrate and exchange_every == 0) else \
        every.value
    self.exchange_every = every.value
    self._handle = ctypes.c_void_p()
    check(
        self._lib.soda_hip_group_create(self.code, len(self.code),
                                        ctypes.byref(self.plan),
                                        ctypes.byref(desc),
                                        ctypes.byref(self._handle)),
        'loading `%s` on GPUs %s' % (stencil.app_name, list(self.devices)))
    # (with calibrate=True the clock may have picked another interval)
    self.exchange_every = int(self.stats()['exchange_every'])

  def close(self) -> None:
    if getattr(self, '_handle', None):
      self._lib.soda_hip_group_destroy(self._handle)
      self._handle = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()

  def slab(self, i: int) -> SlabInfo:
    info = SlabInfo()
    check(self._lib.soda_hip_group_slab(self._handle, i, ctypes.byref(info)),
          'slab %d' % i)
    return info

  def load(self, inputs: Dict[str, 'numpy.ndarray']) -> None:
    """Scatters the global input arrays (and params) over the slabs."""
    import numpy as np
    st = self.stencil
    shape = self.extent[::-1]
    keep: list = []
    tensors = [_host_tensor(np.asarray(inputs[n]), t.np_name, shape, st.dim,
                            keep)
               for n, t in zip(st.input_names, st.input_types)]
    for pstmt in st.param_stmts:
      arr = _host_param(st, inputs, pstmt)
      keep.append(arr)
      tensors.append(HostTensor(arr.ctypes.data, None, None, None))
    arr_t = (HostTensor * len(tensors))(*tensors)
    check(self._lib.soda_hip_group_load(self._handle, arr_t), 'group load')

  def loaded(self) -> None:
    """The caller filled the slabs' input arrays on the devices itself."""
    check(self._lib.soda_hip_group_loaded(self._handle), 'group loaded')

  def run(self, iterate: Optional[int] = None, residual: bool = False) -> None:
    """Enqueues `iterate` iterations on every slab; asynchronous.  `residual`:
    every slab's last interval also takes its share of the residual of the
    last iteration, over the box of all iterations since `load` / `loaded`
    (soda_hip_group_run_residual; `residual()` fetches and folds the shares).
    Needs a group built with LowerOptions(residual=True)."""
    iterate = self.stencil.iterate if iterate is None else iterate
    run = self._lib.soda_hip_group_run_residual if residual else \
        self._lib.soda_hip_group_run
    check(run(self._handle, iterate),
          'running `%s` on %d slabs%s' % (self.stencil.app_name,
                                          len(self.devices),
                                          ' with a residual' if residual else
                                          ''))

  def residual(self, per_slab: bool = False):
    """The residual of the last `run(..., residual=True)`: the slabs' structs
    folded on the host, counts added, maxima the larger -- exactly the
    residual of the whole grid.  Synchronises.  `per_slab`: (Residual, [one
    Residual per slab])."""
    raw = ResidualStruct()
    each = (ResidualStruct * len(self.devices))()
    check(self._lib.soda_hip_group_residual(self._handle, ctypes.byref(raw),
                                            each),
          'group residual')
    total = Residual.from_struct(raw)
    if per_slab:
      return total, [Residual.from_struct(r) for r in each]
    return total

  def last_residual(self, slab: int):
    """How slab `slab` took its share in the last residual run: ('twin' |
    'generic' | None, fusion depth of its last pass)."""
    mode, fused = ctypes.c_int32(), ctypes.c_int32()
    check(self._lib.soda_hip_group_last_residual(self._handle, int(slab),
                                                 ctypes.byref(mode),
                                                 ctypes.byref(fused)),
          'group last_residual')
    return {0: None, 1: 'twin', 2: 'generic'}[mode.value], fused.value

  def run_until(self, tol: float, max_iterate: int, check_every: int = 8,
                int_tol: int = 0):
    """Iterates the loaded state until converged: `check_every` iterations at
    a time, stopping when the last iteration's residual has `unordered == 0`,
    `max_float <= tol` and `max_int <= int_tol`, or after `max_iterate`
    iterations (soda_hip_group_run_until; synchronous).  Returns (iterations
    done, Residual); `store(iterations since the load)` delivers the grid."""
    raw = ResidualStruct()
    done = ctypes.c_int32(0)
    check(self._lib.soda_hip_group_run_until(self._handle, int(max_iterate),
                                             int(check_every), float(tol),
                                             int(int_tol), ctypes.byref(raw),
                                             ctypes.byref(done)),
          'running `%s` on %d slabs until converged' % (
              self.stencil.app_name, len(self.devices)))
    return done.value, Residual.from_struct(raw)

  def synchronize(self) -> None:
    check(self._lib.soda_hip_group_synchronize(self._handle),
          'group synchronize')

  def store(self, iterate: Optional[int] = None,
            outputs: Optional[Dict[str, 'numpy.ndarray']] = None
            ) -> Dict[str, 'numpy.ndarray']:
    """Gathers the results; only the valid box of `iterate` iterations of each
    output is written (the rest keeps what the caller's array held, zeros for
    arrays allocated here)."""
    import numpy as np
    st = self.stencil
    iterate = st.iterate if iterate is None else iterate
    shape = self.extent[::-1]
    keep: list = []
    result = {}
    for n, t in zip(st.output_names, st.output_types):
      result[n] = outputs[n] if outputs is not None and n in outputs else \
          np.zeros(shape, dtype=np.dtype(t.np_name))
    outs = (HostTensor * len(st.output_names))(*[
        _host_tensor(result[n], t.np_name, shape, st.dim, keep)
        for n, t in zip(st.output_names, st.output_types)])
    lo, hi = [], []
    for n in st.output_names:
      l, h = clipped_box(st.valid_box(self.extent, n, iterate), self.extent)
      lo.extend(l)
      hi.extend(h)
    vlo = (ctypes.c_int32 * len(lo))(*lo)
    vhi = (ctypes.c_int32 * len(hi))(*hi)
    check(self._lib.soda_hip_group_store(self._handle, outs, vlo, vhi),
          'group store')
    return result

  def run_host(self, inputs: Dict[str, 'numpy.ndarray'],
               iterate: Optional[int] = None) -> Dict[str, 'numpy.ndarray']:
    """numpy in, numpy out: load, run, store (soda::app::<app>() on N GPUs)."""
    self.load(inputs)
    self.run(iterate)
    return self.store(iterate)

  def stats(self) -> Dict[str, float]:
    st = GroupStats()
    check(self._lib.soda_hip_group_last_stats(self._handle, ctypes.byref(st)),
          'group stats')
    return {name: getattr(st, name) for name, _ in GroupStats._fields_}


class Event:
  """hipEvent wrapper; records on the stream the kernels are launched on."""

  def __init__(self):
    self._lib = library()
    self._h = ctypes.c_void_p()
    check(self._lib.soda_hip_event_create(ctypes.byref(self._h)),
          'event_create')

  def record(self, stream: int = 0) -> None:
    check(self._lib.soda_hip_event_record(self._h, ctypes.c_void_p(stream)),
          'event_record')

  def handle(self) -> int:
    """The hipEvent_t inside (what run_device's ghosts_ready / sendable take)."""
    h = ctypes.c_void_p()
    check(self._lib.soda_hip_event_handle(self._h, ctypes.byref(h)),
          'event_handle')
    return h.value

  def elapsed_ms(self, stop: 'Event') -> float:
    ms = ctypes.c_float()
    check(self._lib.soda_hip_event_elapsed_ms(self._h, stop._h,
                                              ctypes.byref(ms)),
          'event_elapsed')
    return ms.value

  def __del__(self):
    try:
      if self._h:
        self._lib.soda_hip_event_destroy(self._h)
    except Exception:
      pass


class Stream:
  """A HIP stream of the caller's own (for a halo exchange that runs beside
  Program.run_device)."""

  def __init__(self, device: int = 0):
    self._lib = library()
    self._h = ctypes.c_void_p()
    check(self._lib.soda_hip_hipstream_create(device, ctypes.byref(self._h)),
          'hipstream_create')
    self.device = device

  @property
  def handle(self) -> int:
    return self._h.value

  def wait_event(self, event: Event) -> None:
    check(self._lib.soda_hip_hipstream_wait_event(self._h, event._h),
          'hipstream_wait_event')

  def copy(self, dst: int, src: int, nbytes: int,
           src_device: Optional[int] = None) -> None:
    check(self._lib.soda_hip_memcpy_d2d(
        ctypes.c_void_p(dst), self.device, ctypes.c_void_p(src),
        self.device if src_device is None else src_device, nbytes, self._h),
          'memcpy_d2d')

  def synchronize(self) -> None:
    check(self._lib.soda_hip_stream_synchronize(self._h), 'stream_synchronize')

  def __del__(self):
    try:
      if self._h:
        self._lib.soda_hip_hipstream_destroy(self._h)
    except Exception:
      pass


def synchronize(stream: int = 0) -> None:
  check(library().soda_hip_stream_synchronize(ctypes.c_void_p(stream)),
        'stream_synchronize')


class PinnedBuffer:
  """Page-aligned host memory of its own (an anonymous mmap), registered with
  the GPU for its lifetime (soda_hip_host_register): dense arrays carved from
  it travel by DMA from / to where they are when handed to Program.run, no
  staging slots, no worker threads.  Meant to live long -- allocate once, run
  many times, close() at the end -- like the buffers the reference host
  allocates once with aligned_alloc(4096, ...) (ref frt/host.py:165-178).

  Why not register any numpy array: heap memory shares pages with other
  objects and is recycled by malloc; registrations that come and go over such
  pages next to the HIP runtime's own pinning of pageable copies ended in GPU
  memory faults in a soak (tools/experiments/r05_host_soak.py), so the library
  only registers ranges that start on a page boundary."""

  def __init__(self, nbytes: int):
    import mmap
    self.nbytes = max(int(nbytes), 1)
    self._map = mmap.mmap(-1, self.nbytes)
    self._addr = ctypes.addressof(ctypes.c_char.from_buffer(self._map))
    check(library().soda_hip_host_register(ctypes.c_void_p(self._addr),
                                           self.nbytes), 'host_register')
    self._open = True

  def array(self, shape, dtype, offset: int = 0):
    """A dense numpy array of `shape` at byte `offset` of the buffer (the
    caller keeps arrays apart; offsets should be multiples of 4096)."""
    import numpy as np
    dtype = np.dtype(dtype)
    count = 1
    for n in shape:
      count *= int(n)
    if offset < 0 or offset + count * dtype.itemsize > self.nbytes:
      raise util.InputError('PinnedBuffer: %d bytes at offset %d do not fit %d'
                            % (count * dtype.itemsize, offset, self.nbytes))
    return np.frombuffer(self._map, dtype, count, offset).reshape(shape)

  def close(self) -> None:
    if not self._open:
      return
    self._open = False
    rc = library().soda_hip_host_unregister(ctypes.c_void_p(self._addr))
    try:
      self._map.close()
    except BufferError:       # arrays still alive: the pages go with them
      pass
    if rc:
      raise util.BackendError('host_unregister: %s' % last_error())

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()
    return False

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
