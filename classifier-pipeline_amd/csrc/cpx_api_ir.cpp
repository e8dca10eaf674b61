// cpx_api_ir.cpp -- the IR pipeline's entry points (include/cpx.h: cpx_ir_*) and its background model (cpx_mog2_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "cpx_internal.h"

// ---- IR background model ---------------------------------------------------------------------------------------------
struct cpx_mog2 {
  cpx_handle* h = nullptr;
  int n_streams = 0, width = 0, height = 0, history = 0, nframes = 0;
  float var_threshold = 16.0f;
  size_t n = 0;
  DeviceBuffer state;            // float: weight | var | mean, each [5][n]
  DeviceBuffer modes;            // unsigned char [n]
};

void mog2_free(cpx_mog2* m) {
  m->state.release();
  m->modes.release();
  delete m;
}

extern "C" {

int cpx_ir_delta_variance(cpx_handle* h, const uint8_t* cur_dev, const uint8_t* prev_dev, int width, int height,
                          const int32_t* rects_dev, int n, double* var_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!cur_dev || !prev_dev || width < 1 || height < 1 || n < 0 || (n > 0 && (!rects_dev || !var_dev)))
    return fail(h, CPX_ERR_INVALID, "cpx_ir_delta_variance: bad argument");
  if (n == 0) return CPX_OK;
  CPX_ENTER(h);
  cpx::IrVarArgs a{};
  a.W = width; a.H = height; a.n = n;
  a.cur = cur_dev; a.prev = prev_dev; a.rects = rects_dev; a.out = var_dev;
  cpx::launch_ir_delta_variance(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_ir_resize_area(cpx_handle* h, const uint8_t* src_dev, int n, int width, int height, int factor, uint8_t* dst_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!src_dev || !dst_dev || n < 0 || width < 1 || height < 1 || factor < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_ir_resize_area: bad argument");
  if (factor > 16 || width % factor || height % factor)
    return fail(h, CPX_ERR_UNSUPPORTED, "cpx_ir_resize_area: the factor must divide both sides (integer-ratio INTER_AREA only)");
  if (n == 0) return CPX_OK;
  CPX_ENTER(h);
  cpx::launch_ir_resize_area(src_dev, dst_dev, n, width, height, factor, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_ir_merge(cpx_handle* h, const cpx_component* comps_dev, const int32_t* counts_dev, int n, int cap_in, int cap_out,
                 const uint8_t* cur_dev, const uint8_t* prev_dev, int width, int height, int frame_number, int out_stride,
                 cpx_component* out_comps_dev, cpx_frame_info* out_info_dev, int32_t* status_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!comps_dev || !counts_dev || !cur_dev || !out_comps_dev || !status_dev || n < 0 || cap_in < 1 || cap_out < 1 ||
      cap_out > 1024 || width < 1 || height < 1 || frame_number < 0 || out_stride < 1 || frame_number >= out_stride)
    return fail(h, CPX_ERR_INVALID, "cpx_ir_merge: bad argument");
  if (n == 0) return CPX_OK;
  CPX_ENTER(h);
  cpx::IrMergeArgs a{};
  a.W = width; a.H = height; a.n = n; a.cap_in = cap_in; a.cap_out = cap_out;
  a.frame_number = frame_number; a.out_stride = out_stride;
  a.comps = comps_dev; a.counts = counts_dev; a.cur = cur_dev; a.prev = prev_dev;
  a.out_comps = out_comps_dev; a.out_info = out_info_dev; a.status = status_dev;
  cpx::launch_ir_merge(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_ir_frame_statistics(cpx_handle* h, const uint8_t* frames_dev, const uint8_t* masks_dev, int n, int pixels,
                            uint32_t* hist_dev, cpx_ir_frame_stats* out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !hist_dev || !out_dev || n < 0 || pixels < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_ir_frame_statistics: bad argument");
  if (n == 0) return CPX_OK;
  CPX_ENTER(h);
  CPX_HIP(h, hipMemsetAsync(hist_dev, 0, (size_t)n * 256 * sizeof(uint32_t), h->stream));
  CPX_HIP(h, hipMemsetAsync(out_dev, 0, (size_t)n * sizeof(cpx_ir_frame_stats), h->stream));
  cpx::IrStatsArgs a{};
  a.n = n; a.pixels = pixels;
  a.vec16 = pixels % 16 == 0 && reinterpret_cast<uintptr_t>(frames_dev) % 16 == 0 &&
            (!masks_dev || reinterpret_cast<uintptr_t>(masks_dev) % 16 == 0);
  a.frames = frames_dev; a.masks = masks_dev; a.hist = hist_dev; a.out = out_dev;
  cpx::launch_ir_frame_stats(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_mog2_create(cpx_handle* h, int n_streams, int width, int height, int history, float var_threshold,
                    cpx_mog2** out) {
  if (!h) return CPX_ERR_INVALID;
  if (!out || n_streams < 1 || width < 1 || height < 1 || !(var_threshold > 0.0f))
    return fail(h, CPX_ERR_INVALID, "cpx_mog2_create: bad argument");
  *out = nullptr;
  CPX_ENTER(h);
  cpx_mog2* m = new (std::nothrow) cpx_mog2();
  if (!m) return fail(h, CPX_ERR_NOMEM, "cpx_mog2_create: out of memory");
  m->h = h;
  m->n_streams = n_streams;
  m->width = width;
  m->height = height;
  m->history = history > 0 ? history : 500;
  m->var_threshold = var_threshold;
  m->n = (size_t)n_streams * width * height;
  if (m->state.grow(h, 15 * m->n * sizeof(float), "cpx_mog2_create: state allocation failed") ||
      m->modes.grow(h, m->n, "cpx_mog2_create: state allocation failed")) {
    mog2_free(m);
    return CPX_ERR_NOMEM;
  }
  CPX_HIP(h, hipMemsetAsync(m->state.p, 0, m->state.bytes, h->stream));
  CPX_HIP(h, hipMemsetAsync(m->modes.p, 0, m->modes.bytes, h->stream));
  h->mog2s.push_back(m);
  *out = m;
  return CPX_OK;
}

void cpx_mog2_destroy(cpx_mog2* m) {
  if (!m) return;
  cpx_handle* h = m->h;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  h->mog2s.erase(std::remove(h->mog2s.begin(), h->mog2s.end(), m), h->mog2s.end());
  mog2_free(m);
}

static cpx::Mog2Args mog2_args(const cpx_mog2* m) {
  cpx::Mog2Args a{};
  a.n = m->n;
  a.var_threshold = m->var_threshold;
  a.background_ratio = 0.9f;
  a.var_threshold_gen = 9.0f;
  a.var_init = 15.0f;
  a.var_min = 4.0f;
  a.var_max = 75.0f;
  a.weight = m->state.as<float>();
  a.var = a.weight + 5 * m->n;
  a.mean = a.weight + 10 * m->n;
  a.modes = m->modes.as<unsigned char>();
  return a;
}

int cpx_mog2_apply(cpx_mog2* m, const uint8_t* frames_dev, double learning_rate, uint8_t* fgmask_dev) {
  if (!m) return CPX_ERR_INVALID;
  cpx_handle* h = m->h;
  if (!frames_dev || !fgmask_dev) return fail(h, CPX_ERR_INVALID, "cpx_mog2_apply: null argument");
  CPX_ENTER(h);
  m->nframes += 1;
  const double rate = (learning_rate >= 0 && m->nframes > 1) ? learning_rate
                                                            : 1.0 / std::min(2 * m->nframes, m->history);
  cpx::Mog2Args a = mog2_args(m);
  a.alphaT = (float)rate;
  a.alpha1 = 1.0f - a.alphaT;
  a.prune = (float)(-rate * 0.05f);  // -learningRate * fCT, fCT a float member as in the reference implementation
  a.frames = frames_dev;
  a.mask = fgmask_dev;
  cpx::launch_mog2_apply(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_mog2_background(cpx_mog2* m, uint8_t* out_dev) {
  if (!m) return CPX_ERR_INVALID;
  cpx_handle* h = m->h;
  if (!out_dev) return fail(h, CPX_ERR_INVALID, "cpx_mog2_background: null argument");
  CPX_ENTER(h);
  cpx::launch_mog2_background(mog2_args(m), out_dev, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_ir_detect(cpx_handle* h, const uint8_t* images_dev, int n_frames, int width, int height, int threshold,
                  int max_components, cpx_component* comps_dev, int32_t* counts_dev, int32_t* status_dev,
                  int32_t* labels_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!images_dev || !comps_dev || !counts_dev || !status_dev || n_frames < 1 || max_components < 1 || threshold < 0 ||
      threshold > 255)
    return fail(h, CPX_ERR_INVALID, "cpx_ir_detect: bad argument");
  if (!cpx::ir_supported(width, height))
    return fail(h, CPX_ERR_UNSUPPORTED, "cpx_ir_detect: width must be a multiple of 64 and width x height at most 640 x 480");
  CPX_ENTER(h);
  cpx::IrArgs a{};
  a.W = width;
  a.H = height;
  a.threshold = threshold;
  a.max_components = max_components;
  a.images = images_dev;
  a.comps = comps_dev;
  a.counts = counts_dev;
  a.status = status_dev;
  a.labels = labels_dev;
  // one slot per frame that can be resident at once (at most one workgroup of this LDS size per CU pair)
  a.n_slots = n_frames < 256 ? n_frames : 256;
  a.slot_bytes = cpx::ir_slot_bytes(width, height);
  if (int rc = h->ir_scratch.grow(h, a.slot_bytes * (size_t)a.n_slots, "cpx_ir_detect: scratch allocation failed")) return rc;
  if (int rc = h->ir_bitmap.grow(h, 32, "cpx_ir_detect: scratch allocation failed")) return rc;
  CPX_HIP(h, hipMemsetAsync(h->ir_bitmap.p, 0, 32, h->stream));
  a.slots = h->ir_scratch.as<unsigned char>();
  a.slot_bitmap = h->ir_bitmap.as<uint32_t>();
  if (cpx::launch_ir_detect(a, n_frames, h->stream) != 0)
    return fail(h, CPX_ERR_HIP, "cpx_ir_detect: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

}  // extern "C"
