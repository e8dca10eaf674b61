// cpx_internal.h -- what the host files of libcpx_hip.so (cpx_api*.cpp) share: the handle, error reporting, the entry
// macros.  Not installed, not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "cpx.h"
#include "cpx_kernels.h"

struct cpx_cnn;
struct cpx_mog2;
struct cpx_graph;
// what cpx_destroy releases of the objects created on a handle (cpx_api_cnn.cpp, cpx_api_graph.cpp, cpx_api_ir.cpp)
void cnn_free(cpx_cnn* c);
void graph_free(cpx_graph* g);
void mog2_free(cpx_mog2* m);

// One device allocation that only ever grows: owned by the object it is a member of, which releases it by name
// (cpx_api.cpp: release_buffers).  Sizes are bytes.
struct DeviceBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  int grow(cpx_handle* h, size_t need, const char* what);  // (below, behind fail())
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

struct cpx_handle {
  int device = 0;
  cpx_config cfg{};
  hipStream_t stream = nullptr;
  std::string err;
  // device workspace (grown lazily, reused)
  DeviceBuffer ws;
  DeviceBuffer wtab_dev, wthr_dev;  // double / uint32_t [wtab_len], allocated once by cpx_create
  int wtab_len = 0;
  std::vector<double> wtab_host;  // w_k, k = 0 .. wtab_len - 1 (the table the device holds)
  DeviceBuffer nlm_lut_dev;  // int [64], allocated once by cpx_create (denoise only)
  DeviceBuffer sched;  // the schedule's int arrays (cpx_schedule_core.h: SchedLayout)
  struct ConvEv { int key; double flops; hipEvent_t e0, e1; };
  std::vector<ConvEv> conv_events;
  bool conv_timing = false;
  // Two users, both from offset 0: assoc_run's arrays, among them the state a stream resumes from (active, resume), and
  // the scalars of the end-of-clip kernels (final_args).  The end-of-clip calls of a clip come after its last
  // association, so they may overwrite that state.
  DeviceBuffer ws_assoc;
  // timing of the last batch
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  int last_launches = 0;
  bool timing_valid = false;
  // incremental (one clip, frame by frame) tracking: frames consumed so far, -1 = no stream open
  // second stream: the deferred medians (CPX_TRACK_DEFER_MEDIANS)
  hipStream_t stream2 = nullptr;
  // the last track call kept the per-pixel kept-frame counts in the window sums' top ten bits (cpx_frame_kernel<true>): whatever
  // continues from that state, or exports it, unpacks it first (unpack_state)
  bool state_packed = false;
  bool packed_state_ok = true;   // CPX_TRACK_PACKED_STATE=0: never pack
  bool fuse_conv1 = true;   // conv1_1 inside the fused first block of stage 2 (CPX_CNN_FUSE_CONV1=0: a launch of its own)
  // CPX_TRACK_DEFER_MEDIANS: the median kernel of the last track call runs on stream2; ev_median marks its end
  bool medians_pending = false;
  hipEvent_t ev_median = nullptr;
  bool track_per_step = false;  // CPX_TRACK_PER_STEP=1: one launch per frame step (the form before the per-clip walk)
  std::vector<struct cpx_cnn*> cnns;  // networks created on this handle (destroyed with it)
  std::vector<struct cpx_mog2*> mog2s;  // background models created on this handle
  std::vector<struct cpx_graph*> graphs;  // TFLite graphs created on this handle
  // activation arena of cpx_graph_forward: grown to the largest call seen, shared by the handle's graphs (forwards are
  // serialised on the stream), apart from cnn_arena so that a WR-ResNet and a graph can alternate on one handle
  DeviceBuffer graph_arena;
  int stream_frames = -1;
  int stream_assoc_frames = -1;
  bool stream_filt_state = false;
  int last_B = 0;  // clips of the last track call: whose state cpx_get_background / CPX_TRACK_KEEP_BACKGROUND refer to
  struct StagedBackground { std::vector<uint16_t> bg, kcnt; double average; };
  std::map<int, StagedBackground> staged_bg;  // cpx_set_background: applied by the next track call
  int cnn_math = CPX_CNN_MATH_FP16X2;    // cpx_set_cnn_math / CPX_CNN_MATH (the default: include/cpx.h)
  bool fuse_shortcut = true;             // CPX_CNN_FUSE_SHORTCUT=0 keeps the 1x1 shortcuts as launches of their own
  bool shortcut_fp16 = true;             // CPX_CNN_SHORTCUT_FP16=0 keeps the fused shortcuts' products on the float32 matrix instruction
  bool flat16 = true;                    // CPX_CNN_FLAT16=0 keeps stage 4's stride-1 fp16x2 launches on conv_bf3flat_kernel (32x32x16 products)
  DeviceBuffer bf3_scratch;             // split weights of a cpx_conv2d call that brought none
  // activation buffers of cpx_cnn_forward (act0 | act1 | mid | sc), grown to the largest call seen and shared by every
  // network of the handle: forwards on one handle are serialised on its stream, and a second network (another model, another
  // leg of a run) must not bring 54 GB of its own (2,048 samples at frame size 32)
  DeviceBuffer cnn_arena;
  DeviceBuffer cnn_ovf;                  // CPX_CNN_MATH_FP16X2: the overflow word of the forward (or bare convolution) in flight
  int block_fusion = 2;                  // CPX_CNN_BLOCK_FUSION: fp16x2 runs as ONE launch (conv_block32_kernel) 2 = every stage-2 block, 1 = all but the stage's first, 0 = none
  DeviceBuffer ir_scratch;  // cpx_ir_detect: slots for frames whose run / component tables outgrow LDS
  DeviceBuffer ir_bitmap;   // 32 bytes, allocated by the first cpx_ir_detect
};

inline int fail(cpx_handle* h, int code, const char* what, hipError_t e = hipSuccess) {
  if (h) {
    h->err = what;
    if (e != hipSuccess) {
      h->err += ": ";
      h->err += hipGetErrorString(e);
    }
  }
  return code;
}

#define CPX_HIP(h, call)                                            \
  do {                                                              \
    hipError_t _e = (call);                                         \
    if (_e != hipSuccess) return fail((h), CPX_ERR_HIP, #call, _e); \
  } while (0)

// every entry point: select the handle's device and drop stale errors other HIP users of the process left behind,
// so that the hipGetLastError() after our launches reports our launches only
#define CPX_ENTER(h)                           \
  do {                                         \
    CPX_HIP((h), hipSetDevice((h)->device));   \
    (void)hipGetLastError();                   \
  } while (0)

// Makes the buffer at least `need` bytes.  A buffer that is large enough costs no HIP call, so steady-state callers
// issue what they issued before.  One that must grow is freed first (its contents are NOT kept), behind a
// synchronisation of the handle's stream: hipFree waits for the device by itself, the explicit wait only says so.
// Failure leaves the buffer empty.
inline int DeviceBuffer::grow(cpx_handle* h, size_t need, const char* what) {
  if (need <= bytes) return CPX_OK;
  if (p) CPX_HIP(h, hipStreamSynchronize(h->stream));
  release();
  const hipError_t e = hipMalloc(&p, need);
  if (e != hipSuccess) {
    p = nullptr;
    (void)hipGetLastError();
    return fail(h, CPX_ERR_NOMEM, what, e);
  }
  bytes = need;
  return CPX_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
