// soda_stream.h -- the wire-format stream object (soda_stream.cpp) and the route
// of one of its calls, for that unit and for its host test
// (tests/host/stream_route_main.cpp).  Nothing here crosses the C ABI.
#ifndef SODA_STREAM_H_
#define SODA_STREAM_H_

#include "soda_internal.h"

#include <utility>

namespace soda_detail {

// One tensor's place in the caller's bank lists, made once at
// soda_hip_stream_create (inputs first, then outputs)
struct StreamTensor {
  int32_t first;    // its first bank in in_banks (an input) / out_banks
  int32_t banks;
  int32_t elem;     // bytes per cell
  int32_t shift;
  bool input;
};

}  // namespace soda_detail

struct soda_hip_stream {
  soda_hip_stream_desc_t desc;
  std::vector<soda_detail::StreamTensor> tensors;
  soda_hip_program* dense = nullptr;
  // per input / output: unwire_<in>, wire_<out> (null: none needed)
  std::vector<soda_hip_program*> linear, unwire, wire;
  // de-interleaved streams
  std::vector<soda_detail::DeviceBuffer> dense_in, dense_out;
  std::vector<soda_detail::DeviceBuffer> host_banks;   // run_host staging
  bool dense_failed = false;
  int last_mode = 0;
  // Device-resident banks narrower than this run the linear form even where
  // the dense view exists: narrow tiles leave most of a 64-lane x V-wide
  // marching strip idle (heat3d 32 x 32 tiles: 0.50 vs 0.79 ms).  Host banks
  // take the dense view whenever there is one -- there the copies dominate and
  // the dense view is what lets them overlap in bands.
  int device_dense_min_tile0 = 256;
  // The banked form of the dense program (soda_hip_stream_set_banked): one
  // kernel that runs all `iterate` iterations and addresses the banks of the
  // tensors marked in `in_kernel` itself -- to run_core a one-pass program of
  // one iteration with every such bank a tensor of its own.  So it meets
  // neither of run_core's one-shape-per-tensor assumptions: a stream run has
  // no slab, hence no row-range offset, and iterate is 1 there.
  soda_hip_program* banked = nullptr;
  std::vector<int32_t> in_kernel;     // per tensor, inputs first
  // Two-iteration programs (soda_hip_stream_set_banked_pair): the
  // one-iteration kernel with the in_kernel INPUTS bank by bank, and with the
  // in_kernel OUTPUTS bank by bank.  Where the dense program's schedule for
  // the stream's extent is two one-iteration launches, these two run instead
  // of `banked`, a dense temporary per output between them: the banked path
  // then computes every cell of the dense view -- the array's border cells
  // included, which a fused kernel and two launches do not agree on -- as the
  // dense program does.
  soda_hip_program* banked_first = nullptr;
  soda_hip_program* banked_last = nullptr;
  std::vector<soda_detail::DeviceBuffer> banked_tmp;
  // (stream length, banked launches) of the device runs that went through:
  // the staging arrays and the scratch of every program such a call runs are
  // in place, a repeat allocates nothing and skips the look-ahead
  // (route_grows).  Emptied by whatever changes the route a length takes.
  std::vector<std::pair<int32_t, int>> warm;
};

namespace soda_detail {

enum StreamForm { kBankedOne, kBankedTwo, kDenseView, kLinear };
// how the program meets a tensor: handed over bank by bank, the caller's one
// bank read / written in place, or staged through dense_in / dense_out
enum StreamRole { kByBank, kInPlace, kStaged };

struct RouteBuffer {
  DeviceBuffer* buf;
  size_t bytes;
  bool zero_new;    // new memory is zero-filled on the caller's stream
};

struct RouteLaunch {
  soda_hip_program* program;
  int32_t extent[SODA_HIP_MAX_DIM];
  int32_t iterate;
  int32_t stream_elems;
  int tensor;       // a copy kernel's tensor; -1: the program itself
};

// Everything soda_hip_stream_run_device decides about one call.  The
// look-ahead, the refusals and the run only walk it.
struct StreamRoute {
  int32_t n;                             // stream length, in elements
  StreamForm form;
  int linear_pick;                       // the linear program of this length
  int32_t extent[SODA_HIP_MAX_DIM];      // the dense view (not kLinear)
  StreamRole role[SODA_HIP_MAX_TENSORS];
  int staging[SODA_HIP_MAX_TENSORS];     // kStaged: index into buffers
  // staging arrays by tensor, then the temporaries of kBankedTwo by output
  RouteBuffer buffers[2 * SODA_HIP_MAX_TENSORS];
  int num_buffers;
  // unwire_<in>..., the program (one launch or two), wire_<out>...
  RouteLaunch launches[SODA_HIP_MAX_TENSORS + 2];
  int num_launches;
  // launches of the banked form (0: the call runs as without one)
  int banked() const {
    return form == kBankedOne ? 1 : form == kBankedTwo ? 2 : 0;
  }
};

// The route of a call on `n` elements.  Makes no HIP call, allocates nothing
// on the device and leaves the stream object as it is; a NULL bank routes like
// a misaligned one (route_refusal names it).
int stream_route(soda_hip_stream* s, void* const* out_banks,
                 const void* const* in_banks, int32_t n, StreamRoute* route);
// The look-ahead: would the call allocate -- a buffer of the route too_small,
// a launch of the route growing its program's scratch?  `asked` (tests): every
// buffer and program it looked at, in order.
int route_grows(const StreamRoute& route, bool* grows,
                std::vector<const void*>* asked = nullptr);
// What a call is refused for: a NULL bank, an in-place bank not 16-byte aligned
int route_refusal(const soda_hip_stream* s, const StreamRoute& route,
                  void* const* out_banks, const void* const* in_banks);

}  // namespace soda_detail

#endif  // SODA_STREAM_H_
