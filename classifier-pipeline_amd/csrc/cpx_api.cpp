// cpx_api.cpp -- the C-ABI of libcpx_hip.so (include/cpx.h): handle lifetime,
// device workspace, host-side schedule of the per-frame launches.  No torch
// types, no exceptions across the boundary.  (The WR-ResNet: cpx_api_cnn.cpp; the
// TFLite graph executor: cpx_api_graph.cpp; the IR pipeline: cpx_api_ir.cpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "cpx_internal.h"
#include "cpx_schedule_core.h"

static_assert(sizeof(cpx_component) == 32, "cpx_component layout is part of the ABI");
static_assert(sizeof(cpx_frame_info) == 80, "cpx_frame_info layout is part of the ABI");
static_assert(sizeof(cpx_frame_meta) == 24, "cpx_frame_meta layout is part of the ABI");
static_assert(sizeof(cpx_config) == 48, "cpx_config layout is part of the ABI");
static_assert(sizeof(cpx_region_ref) == 24 && sizeof(cpx_track_limits) == 32 && sizeof(cpx_crop_req) == 32,
              "classification request layouts are part of the ABI");
static_assert(sizeof(cpx_filter_params) == 72 && sizeof(cpx_track_summary) == 120,
              "end-of-clip layouts are part of the ABI");
static_assert(sizeof(cpx_region) == 56, "cpx_region layout is part of the ABI");
static_assert(sizeof(cpx_track_record) == 32, "cpx_track_record layout is part of the ABI");
static_assert(sizeof(cpx_track_params) == 120, "cpx_track_params layout is part of the ABI");

namespace {

struct WsLayout {
  size_t bg, wsum, kcnt, filt, cstate, u8, carry, bgavg, big, total;
};

WsLayout ws_layout(const cpx_config& c, int B, bool need_filt_state) {
  const size_t P = (size_t)c.width * c.height;
  WsLayout l{};
  size_t off = 0;
  l.bg = off;
  off = align_up(off + (size_t)B * 2 * P * sizeof(uint16_t), 256);
  l.wsum = off;
  off = align_up(off + (size_t)B * P * sizeof(uint32_t), 256);
  l.kcnt = off;
  off = align_up(off + (size_t)B * P * sizeof(uint16_t), 256);
  l.filt = off;
  if (need_filt_state) off = align_up(off + (size_t)B * 2 * P * sizeof(float), 256);
  l.cstate = off;
  off = align_up(off + (size_t)B * sizeof(cpx::ClipState), 256);
  // hand-over buffers of split frame steps (front -> NLM -> back, or front || back pipelined): two slots per clip
  l.u8 = off;
  off = align_up(off + (size_t)B * 2 * P, 256);
  l.carry = off;
  off = align_up(off + (size_t)B * 2 * sizeof(cpx::FrameCarry), 256);
  l.bgavg = off;
  off = align_up(off + (size_t)B * sizeof(double), 256);
  // a handle whose frames may hold more components than the frame kernel's LDS tables: the same tables per clip in HBM
  // (eight statistics rows + the rank row of max_components entries; cpx_track.hip phase 7)
  l.big = off;
  if (c.max_components > cpx::track_lds_components())
    off = align_up(off + (size_t)B * 9 * c.max_components * sizeof(uint32_t), 256);
  l.total = off;
  return l;
}

int build_schedule(cpx_handle* h, const int32_t* clip_offsets, const cpx_frame_meta* meta, int B, cpx::Schedule* sc) {
  switch (cpx::schedule_build(clip_offsets, meta, B, h->cfg.max_frames, sc)) {
    case cpx::SchedError::EmptyClip: return fail(h, CPX_ERR_INVALID, "empty clip in batch");
    case cpx::SchedError::TooLong: return fail(h, CPX_ERR_INVALID, "clip longer than max_frames");
    case cpx::SchedError::Ok: break;
  }
  return CPX_OK;
}

// the schedule in h->sched; *sl says where its arrays lie there
int upload_schedule(cpx_handle* h, const cpx::Schedule& sc, int B, cpx::SchedLayout* sl) {
  const std::vector<int> flat = cpx::schedule_flatten(sc, B);
  *sl = cpx::SchedLayout::of(B, (int)sc.proc_idx.size());
  if (int rc = h->sched.grow(h, flat.size() * sizeof(int), "schedule hipMalloc")) return rc;
  CPX_HIP(h, hipMemcpyAsync(h->sched.p, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  CPX_HIP(h, hipStreamSynchronize(h->stream));  // `flat` dies with this scope
  return CPX_OK;
}

}  // namespace

extern "C" {

int cpx_abi_version(void) { return CPX_ABI_VERSION; }

int cpx_create(int device_id, const cpx_config* cfg, cpx_handle** out) {
  if (!cfg || !out) return CPX_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CPX_ERR_NO_DEVICE;
  if (device_id < 0 || device_id >= ndev) return CPX_ERR_INVALID;
  const int W = cfg->width, H = cfg->height;
  if (W <= 0 || H <= 0 || (W % 8) != 0 || W >= 192 || W * H > cpx::track_max_pixels() || H < 5 || W < 8)
    return CPX_ERR_UNSUPPORTED;
  if (cfg->edge_pixels < 0 || 2 * cfg->edge_pixels >= std::min(W, H) || cfg->window < 1 ||
      cfg->max_components < 1 || cfg->max_frames < 1 || cfg->max_frames > 65534)
    return CPX_ERR_INVALID;
  cpx_handle* h = new (std::nothrow) cpx_handle();
  if (!h) return CPX_ERR_NOMEM;
  h->device = device_id;
  h->cfg = *cfg;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_median, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess) {
    cpx_destroy(h);
    return CPX_ERR_HIP;
  }
  // weight table: w_k = k-fold float64 accumulation of weight_add, exactly as
  // NumPy evaluates background_weight + weight_add (motiondetector.py:218-222)
  // one entry per value the uint16 per-pixel counter can take: CPX_TRACK_KEEP_BACKGROUND chains and long streams
  // carry a pixel's count past this handle's max_frames (the tables cost 786 KB per handle)
  h->wtab_len = 65536;
  h->wtab_host.resize(h->wtab_len);
  std::vector<double>& wt = h->wtab_host;
  double w = 0.0;
  for (int k = 0; k < h->wtab_len; ++k) {
    wt[k] = w;
    w = w + cfg->weight_add;
  }
  if (cfg->denoise) {
    if (!cpx::nlm_supported(W, H)) {
      cpx_destroy(h);
      return CPX_ERR_UNSUPPORTED;
    }
    // fastNlMeansDenoising weight table (h = 3, template 7x7, search 21x21), SURVEY.md Appendix A.6:
    // w[a] = round(fixed_point_mult * exp(-a * (64/49) / h^2)), zero below 0.001 * fixed_point_mult
    const int fixed_point_mult = (int)(2147483647LL / (21 * 21 * 255));
    std::vector<int> lut(64, 0);
    for (int a2 = 0; a2 < 64; ++a2) {
      const double wv = std::exp(-((double)a2 * (64.0 / 49.0)) / 9.0);
      const double wr = std::nearbyint((double)fixed_point_mult * wv);
      lut[a2] = (wr < 0.001 * fixed_point_mult) ? 0 : (int)wr;
    }
    if (lut[63] != 0 || h->nlm_lut_dev.grow(h, 64 * sizeof(int), "NLM weight table allocation") ||
        hipMemcpy(h->nlm_lut_dev.p, lut.data(), 64 * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      cpx_destroy(h);
      return CPX_ERR_HIP;
    }
  }
  // integer form of `bg < f - w_k` for integer bg, f (cpx_track.hip, streaming pass): keep <=> f - bg >= hi_k,
  // hi_k = floor(w_k) + 1.  Exact whenever w_k is an integer or at least 1e-6 away from one (f - w_k is then no
  // integer and its float64 rounding, < 2e-11 for f < 65536, cannot reach one).  Otherwise ("near") the kernel decides
  // f - bg == rint(w_k) with the float64 expression; hi_k = rint(w_k) + 1 then.  The entry is 2 hi_k - near_k: the kernel
  // keeps on 2 (f - bg) + 1 > entry and evaluates the float64 expression on equality (odd entries only).
  std::vector<uint32_t> thr(h->wtab_len);
  for (int k = 0; k < h->wtab_len; ++k) {
    const double wk = wt[k], m = std::nearbyint(wk);
    const bool exact = (wk == m), near = !exact && std::fabs(wk - m) < 1e-6;
    double hi = near ? m + 1.0 : std::floor(wk) + 1.0;
    if (!(hi >= 0.0)) hi = 0.0;                    // (negative weight_add: never reached by a sane config)
    if (hi > 536870912.0) hi = 536870912.0;        // beyond any f - bg: never kept (and 2 hi a positive int32)
    thr[k] = 2u * (uint32_t)hi - (near ? 1u : 0u);
  }
  if (h->wthr_dev.grow(h, thr.size() * sizeof(uint32_t), "threshold table allocation") ||
      hipMemcpy(h->wthr_dev.p, thr.data(), thr.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    cpx_destroy(h);
    return CPX_ERR_HIP;
  }
  if (h->wtab_dev.grow(h, wt.size() * sizeof(double), "weight table allocation") ||
      hipMemcpy(h->wtab_dev.p, wt.data(), wt.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      cpx::frame_kernel_attr_setup() != 0) {
    cpx_destroy(h);
    return CPX_ERR_HIP;
  }
  if (const char* env = std::getenv("CPX_TRACK_PACKED_STATE")) h->packed_state_ok = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_CNN_FUSE_CONV1")) h->fuse_conv1 = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_TRACK_PER_STEP")) h->track_per_step = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_CNN_FUSE_SHORTCUT")) h->fuse_shortcut = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_CNN_SHORTCUT_FP16")) h->shortcut_fp16 = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_CNN_FLAT16")) h->flat16 = std::atoi(env) != 0;
  if (const char* env = std::getenv("CPX_CNN_BLOCK_FUSION")) h->block_fusion = std::min(std::max(std::atoi(env), 0), 2);
  if (const char* env = std::getenv("CPX_CNN_MATH")) {
    if (!std::strcmp(env, "f32")) h->cnn_math = CPX_CNN_MATH_F32;
    else if (!std::strcmp(env, "bf16x3")) h->cnn_math = CPX_CNN_MATH_BF16X3;
    else if (!std::strcmp(env, "bf16x2")) h->cnn_math = CPX_CNN_MATH_BF16X2;
    else if (!std::strcmp(env, "fp16x2")) h->cnn_math = CPX_CNN_MATH_FP16X2;
  }
  *out = h;
  return CPX_OK;
}

// The one place that names the handle's device buffers.  cpx_release_memory gives back the first list, the ones that
// grow with the calls; cpx_destroy the small tables of the second as well.
static void release_buffers(cpx_handle* h, bool all) {
  for (DeviceBuffer* b : {&h->ws, &h->ws_assoc, &h->bf3_scratch, &h->cnn_arena, &h->graph_arena, &h->ir_scratch}) b->release();
  if (!all) return;
  for (DeviceBuffer* b : {&h->sched, &h->wtab_dev, &h->wthr_dev, &h->nlm_lut_dev, &h->cnn_ovf, &h->ir_bitmap}) b->release();
}

void cpx_destroy(cpx_handle* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (cpx_cnn* c : h->cnns) cnn_free(c);
  h->cnns.clear();
  for (cpx_mog2* m : h->mog2s) mog2_free(m);
  h->mog2s.clear();
  for (cpx_graph* g : h->graphs) graph_free(g);
  h->graphs.clear();
  release_buffers(h, true);
  for (auto& e : h->conv_events) {
    hipEventDestroy(e.e0);
    hipEventDestroy(e.e1);
  }
  if (h->stream2) {
    hipStreamSynchronize(h->stream2);
    hipStreamDestroy(h->stream2);
  }
  if (h->ev_median) hipEventDestroy(h->ev_median);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

const char* cpx_last_error(const cpx_handle* h) { return h ? h->err.c_str() : "null handle"; }

void* cpx_stream(cpx_handle* h) { return h ? (void*)h->stream : nullptr; }

// Medians of a CPX_TRACK_DEFER_MEDIANS call still in flight on stream2: what is enqueued on the handle's stream from here
// on runs behind them.  Called by every entry point that reads cpx_frame_info.thermal_median or reuses the buffers the
// median kernel reads and writes.
static int join_medians(cpx_handle* h) {
  if (h->medians_pending) {
    h->medians_pending = false;
    CPX_HIP(h, hipStreamWaitEvent(h->stream, h->ev_median, 0));
  }
  return CPX_OK;
}

int cpx_join_medians(cpx_handle* h) {
  if (!h) return CPX_ERR_INVALID;
  return join_medians(h);
}

int cpx_release_memory(cpx_handle* h) {
  if (!h) return CPX_ERR_INVALID;
  CPX_ENTER(h);
  if (int rc = join_medians(h)) return rc;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  CPX_HIP(h, hipStreamSynchronize(h->stream2));
  release_buffers(h, false);
  h->last_B = 0;  // (the track state went with the workspace)
  h->state_packed = false;
  return CPX_OK;
}

int cpx_synchronize(cpx_handle* h) {
  if (!h) return CPX_ERR_INVALID;
  if (int rc = join_medians(h)) return rc;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  return CPX_OK;
}

size_t cpx_track_workspace_bytes(const cpx_handle* h, int B, int total_frames) {
  if (!h || B <= 0) return 0;
  (void)total_frames;
  return ws_layout(h->cfg, B, true).total;
}

// Track stage for B clips.  n_prev < 0: whole clips (cpx_track_batch).  n_prev >= 0 (B == 1): the clip's first n_prev
// frames were consumed by earlier calls on this handle and its state is still in the workspace; only the frames
// [n_prev, clip_offsets[1]) are processed (cpx_track_frame).
// the state of the last track call in the layout every path but cpx_frame_kernel<true> reads (see cpx_handle::state_packed)
static int unpack_state(cpx_handle* h) {
  if (h->state_packed && h->ws.p && h->last_B > 0) {
    const WsLayout lp = ws_layout(h->cfg, h->last_B, h->stream_filt_state);
    char* base = h->ws.as<char>();
    cpx::launch_unpack_state((uint32_t*)(base + lp.wsum), (uint16_t*)(base + lp.kcnt),
                             (size_t)h->last_B * h->cfg.width * h->cfg.height, h->stream);
    CPX_HIP(h, hipGetLastError());
  }
  h->state_packed = false;
  return CPX_OK;
}

static int track_run(cpx_handle* h, const uint16_t* frames_dev, const int32_t* clip_offsets,
                     const cpx_frame_meta* meta, int B, int n_prev, cpx_component* comps_dev,
                     cpx_frame_info* info_dev, int32_t* labels_dev, float* filtered_dev,
                     float* background_dev, int flags) {
  CPX_ENTER(h);
  if (flags & ~(CPX_TRACK_KEEP_BACKGROUND | CPX_TRACK_FREEZE_ON_FFC | CPX_TRACK_FREEZE_BACKGROUND | CPX_TRACK_DEFER_MEDIANS))
    return fail(h, CPX_ERR_INVALID, "track: unknown flag");
  if (int jrc = join_medians(h)) return jrc;  // (a previous call's medians read the frames / write the records this one may reuse)
  const bool defer_medians = (flags & CPX_TRACK_DEFER_MEDIANS) != 0;
  const cpx_config& c = h->cfg;
  cpx::Schedule sc;
  int rc = build_schedule(h, clip_offsets, meta, B, &sc);
  if (rc != CPX_OK) return rc;
  const int total = sc.total, max_proc = sc.max_proc;
  const bool resume = n_prev > 0;
  const int t_begin = cpx::processed_before(meta, n_prev);
  // ---- device workspace ----
  const bool need_filt = (filtered_dev == nullptr);
  const WsLayout l = ws_layout(c, B, need_filt);
  if (resume && (l.total > h->ws.bytes || need_filt != h->stream_filt_state))
    return fail(h, CPX_ERR_INVALID, "cpx_track_frame: the stream's workspace is gone (optional outputs changed?)");
  const bool keep = !resume && (flags & CPX_TRACK_KEEP_BACKGROUND);
  if (keep) {
    // every clip needs a state to continue from: the previous call's (same layout) or a staged one
    const bool have_prev = h->ws.p && h->last_B == B && need_filt == h->stream_filt_state && l.total <= h->ws.bytes;
    for (int b = 0; b < B && !have_prev; ++b)
      if (!h->staged_bg.count(b)) {
        h->staged_bg.clear();  // staged for THIS call: a refused call does not leave them behind for the one after
        return fail(h, CPX_ERR_INVALID, "CPX_TRACK_KEEP_BACKGROUND: no background state for a clip (previous call had another batch size, and nothing staged; staged states dropped)");
      }
  }
  for (const auto& kv : h->staged_bg)
    if (kv.first >= B) {
      h->staged_bg.clear();  // staged for THIS call: a refused call does not leave them behind for the one after
      return fail(h, CPX_ERR_INVALID, "cpx_set_background: staged clip index outside the batch (staged states dropped)");
    }
  // a call that continues from the previous call's state reads it in the two-array layout; a fresh one starts its own
  if (resume || keep) {
    if (int urc = unpack_state(h)) return urc;
  }
  h->state_packed = false;
  h->stream_filt_state = need_filt;
  h->last_B = B;
  // from here on the workspace no longer holds the previous call's state: a return before the end leaves no state at all
  // (KEEP_BACKGROUND, the *_frame calls and cpx_get_background refuse), never one read in the wrong layout or batch size
  struct StateGuard {
    cpx_handle* h;
    bool armed = true;
    ~StateGuard() {
      if (armed) {
        h->last_B = 0;
        h->state_packed = false;
      }
    }
  } guard{h};
  if ((rc = h->ws.grow(h, l.total, "workspace hipMalloc"))) return rc;
  cpx::SchedLayout sl;
  rc = upload_schedule(h, sc, B, &sl);
  if (rc != CPX_OK) return rc;

  cpx::TrackArgs a{};
  a.W = c.width;
  a.H = c.height;
  a.edge = c.edge_pixels;
  a.window = c.window;
  a.cap_out = c.max_components;
  a.flags = flags;
  a.background_thresh = c.background_thresh;
  a.weight_add = c.weight_add;
  a.frames = frames_dev;
  cpx::schedule_point(a, h->sched.as<int>(), sl);
  a.order = h->sched.as<int>() + sl.order;
  a.wtab = h->wtab_dev.as<double>();
  a.wtab_len = h->wtab_len;
  a.wthr = h->wthr_dev.as<uint32_t>();
  char* base = h->ws.as<char>();
  a.bg = (uint16_t*)(base + l.bg);
  a.wsum = (uint32_t*)(base + l.wsum);
  a.kcnt = (uint16_t*)(base + l.kcnt);
  // a fresh batch of at most 1023 processed frames per clip: the kept-frame counts ride in the window sums (cpx_track.hip, PK)
  a.packed_state = (h->packed_state_ok && !resume && !keep && h->staged_bg.empty() && max_proc <= 1023 && c.window <= 64) ? 1 : 0;
  a.filt_state = need_filt ? (float*)(base + l.filt) : nullptr;
  a.cstate = (cpx::ClipState*)(base + l.cstate);
  a.u8_state = (unsigned char*)(base + l.u8);
  a.carry = (cpx::FrameCarry*)(base + l.carry);
  a.bgavg = (double*)(base + l.bgavg);
  a.big_stat = c.max_components > cpx::track_lds_components() ? (uint32_t*)(base + l.big) : nullptr;
  a.nlm_flip = c.denoise ? 1 : 0;
  a.nlm_lut = h->nlm_lut_dev.as<int>();
  a.comps_out = comps_dev;
  a.info_out = info_dev;
  a.labels_out = labels_dev;
  a.filtered_out = filtered_dev;

  // frames that are never processed (background frames) get frame_number = -1
  const int f_new = resume ? n_prev : 0;
  CPX_HIP(h, hipMemsetAsync(info_dev + f_new, 0xFF, (size_t)(total - f_new) * sizeof(cpx_frame_info), h->stream));
  if (!resume) cpx::launch_init(a, B, keep ? 1 : 0, h->stream);
  if (!h->staged_bg.empty()) {
    // staged states replace the seeding (or, in the middle of a stream, the model an external owner changed): both
    // ping-pong slots, the weight counters, the average
    const size_t P = (size_t)c.width * c.height;
    for (const auto& kv : h->staged_bg) {
      const int b = kv.first;
      const auto& sb = kv.second;
      for (int slot = 0; slot < 2; ++slot)
        CPX_HIP(h, hipMemcpyAsync(a.bg + ((size_t)b * 2 + slot) * P, sb.bg.data(), P * sizeof(uint16_t),
                                  hipMemcpyHostToDevice, h->stream));
      CPX_HIP(h, hipMemcpyAsync(a.kcnt + (size_t)b * P, sb.kcnt.data(), P * sizeof(uint16_t), hipMemcpyHostToDevice,
                                h->stream));
      CPX_HIP(h, hipMemcpyAsync(&a.cstate[b].bg_average, &sb.average, sizeof(double), hipMemcpyHostToDevice, h->stream));
      CPX_HIP(h, hipMemcpyAsync(a.bgavg + b, &sb.average, sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    CPX_HIP(h, hipStreamSynchronize(h->stream));  // the staged vectors die here
    h->staged_bg.clear();
  }
  // medians of all new frames first (independent of the clips' frame order; their word of the records is theirs alone,
  // the frame kernel stores around it): one workgroup per (clip, step).  Nothing orders the two kernels, but running
  // them side by side on two streams gains nothing (the call takes 123.1 ms against 122.6 ms,
  // profiles/r06_track_experiments.md): in front, on the one stream.
  if ((long long)B * (max_proc - t_begin) > 2147483647LL) return fail(h, CPX_ERR_INVALID, "batch too large for one launch");
  // CPX_TRACK_DEFER_MEDIANS: behind the frame kernel on the second stream instead (below), beside the caller's next stages
  if (!defer_medians) cpx::launch_median(a, B, t_begin, max_proc, h->stream);
  CPX_HIP(h, hipEventRecord(h->ev0, h->stream));  // (ev0 .. ev1 bracket the frame / NLM kernels)
  int launches = 0;
  if (!c.denoise && !h->track_per_step) {
    // one workgroup per clip walks its frames: a single launch, no phase lockstep between the clips (cpx_track.hip)
    cpx::launch_frame(a, B, t_begin, max_proc, 0, h->stream);
    launches = 1;
  } else {
    for (int t = t_begin; t < max_proc; ++t) {
      if (!c.denoise) {
        cpx::launch_frame(a, B, t, t + 1, 0, h->stream);
      } else {  // front (normalise) -> non-local means -> back (blur / threshold / label / statistics)
        cpx::launch_frame(a, B, t, t + 1, 1, h->stream);
        cpx::launch_nlm(a, B, t, h->stream);
        cpx::launch_frame(a, B, t, t + 1, 2, h->stream);
      }
      ++launches;
    }
  }
  CPX_HIP(h, hipEventRecord(h->ev1, h->stream));
  if (defer_medians) {
    CPX_HIP(h, hipStreamWaitEvent(h->stream2, h->ev1, 0));  // (the records' memset and the frame kernels are in front of ev1)
    cpx::launch_median(a, B, t_begin, max_proc, h->stream2);
    CPX_HIP(h, hipEventRecord(h->ev_median, h->stream2));
    h->medians_pending = true;
  }
  h->state_packed = a.packed_state != 0;
  h->last_launches = launches;
  h->timing_valid = true;
  if (background_dev) cpx::launch_export_background(a, B, background_dev, h->stream);
  CPX_HIP(h, hipGetLastError());
  guard.armed = false;
  return CPX_OK;
}

int cpx_track_batch_ex(cpx_handle* h, const uint16_t* frames_dev, const int32_t* clip_offsets,
                       const cpx_frame_meta* meta, int B, cpx_component* comps_dev, cpx_frame_info* info_dev,
                       int32_t* labels_dev, float* filtered_dev, float* background_dev, int flags) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !clip_offsets || !meta || B <= 0 || !comps_dev || !info_dev)
    return fail(h, CPX_ERR_INVALID, "cpx_track_batch: null argument");
  h->stream_frames = -1;  // the workspace is re-initialised: an open stream ends here
  return track_run(h, frames_dev, clip_offsets, meta, B, -1, comps_dev, info_dev, labels_dev, filtered_dev,
                   background_dev, flags);
}

int cpx_track_batch(cpx_handle* h, const uint16_t* frames_dev, const int32_t* clip_offsets,
                    const cpx_frame_meta* meta, int B, cpx_component* comps_dev,
                    cpx_frame_info* info_dev, int32_t* labels_dev, float* filtered_dev,
                    float* background_dev) {
  return cpx_track_batch_ex(h, frames_dev, clip_offsets, meta, B, comps_dev, info_dev, labels_dev, filtered_dev,
                            background_dev, 0);
}

int cpx_track_frame_ex(cpx_handle* h, const uint16_t* frames_dev, const cpx_frame_meta* meta, int n_prev, int n_frames,
                       cpx_component* comps_dev, cpx_frame_info* info_dev, int32_t* labels_dev, float* filtered_dev,
                       float* background_dev, int flags) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !meta || !comps_dev || !info_dev || n_prev < 0 || n_frames <= n_prev)
    return fail(h, CPX_ERR_INVALID, "cpx_track_frame: bad argument");
  if (n_prev > 0 && h->stream_frames != n_prev)
    return fail(h, CPX_ERR_INVALID, "cpx_track_frame: n_prev does not match the frames this handle has consumed");
  const int32_t offs[2] = {0, n_frames};
  h->stream_frames = -1;
  if (n_prev == 0) h->stream_assoc_frames = -1;  // a new clip: its association starts fresh
  const int rc = track_run(h, frames_dev, offs, meta, 1, n_prev, comps_dev, info_dev, labels_dev, filtered_dev,
                           background_dev, flags);
  if (rc == CPX_OK) h->stream_frames = n_frames;
  return rc;
}

int cpx_track_frame(cpx_handle* h, const uint16_t* frames_dev, const cpx_frame_meta* meta, int n_prev, int n_frames,
                    cpx_component* comps_dev, cpx_frame_info* info_dev, int32_t* labels_dev, float* filtered_dev,
                    float* background_dev) {
  return cpx_track_frame_ex(h, frames_dev, meta, n_prev, n_frames, comps_dev, info_dev, labels_dev, filtered_dev,
                            background_dev, 0);
}

int cpx_set_background(cpx_handle* h, int clip, const float* background, const double* weights, double average) {
  if (!h) return CPX_ERR_INVALID;
  if (clip < 0 || !background) return fail(h, CPX_ERR_INVALID, "cpx_set_background: bad argument");
  const cpx_config& c = h->cfg;
  const int W = c.width, H = c.height, e = c.edge_pixels;
  const size_t P = (size_t)W * H;
  cpx_handle::StagedBackground sb;
  sb.bg.resize(P);
  sb.kcnt.assign(P, 0);
  sb.average = average;
  for (size_t p = 0; p < P; ++p) {
    const float v = background[p];
    if (!(v >= 0.0f && v <= 65535.0f) || v != std::floor(v))
      return fail(h, CPX_ERR_UNSUPPORTED, "cpx_set_background: the background must be integer-valued in [0, 65535]");
    sb.bg[p] = (uint16_t)v;
  }
  if (weights) {
    // a weight is the k-fold float64 accumulation of weight_add (motiondetector.py:218-222): find k, exactly
    const std::vector<double>& wt = h->wtab_host;
    const int iw = W - 2 * e, ih = H - 2 * e;
    for (int y = 0; y < ih; ++y)
      for (int x = 0; x < iw; ++x) {
        const double wv = weights[(size_t)y * iw + x];
        long k = c.weight_add > 0 ? std::lround(wv / c.weight_add) : 0;
        bool ok = false;
        for (long kk = std::max(0L, k - 1); kk <= k + 1 && kk < h->wtab_len; ++kk)
          if (wt[kk] == wv) {
            k = kk;
            ok = true;
            break;
          }
        if (!ok) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_set_background: a weight is not an accumulation of weight_add");
        sb.kcnt[(size_t)(y + e) * W + (x + e)] = (uint16_t)k;
      }
  }
  h->staged_bg[clip] = std::move(sb);
  return CPX_OK;
}

int cpx_get_background(cpx_handle* h, int clip, float* background, double* weights, double* average) {
  if (!h) return CPX_ERR_INVALID;
  if (clip < 0 || clip >= h->last_B || !h->ws.p) return fail(h, CPX_ERR_INVALID, "cpx_get_background: no such clip in the last track call");
  CPX_ENTER(h);
  const cpx_config& c = h->cfg;
  const int W = c.width, H = c.height, e = c.edge_pixels;
  const size_t P = (size_t)W * H;
  const WsLayout l = ws_layout(c, h->last_B, h->stream_filt_state);
  char* base = h->ws.as<char>();
  if (int urc = unpack_state(h)) return urc;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  cpx::ClipState st;
  CPX_HIP(h, hipMemcpy(&st, base + l.cstate + (size_t)clip * sizeof(cpx::ClipState), sizeof(st), hipMemcpyDeviceToHost));
  if (average) *average = st.bg_average;
  if (background) {
    std::vector<uint16_t> bg(P);
    CPX_HIP(h, hipMemcpy(bg.data(), base + l.bg + ((size_t)clip * 2 + (st.n_done & 1)) * P * sizeof(uint16_t),
                         P * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {  // the interior is authoritative, edges replicate it (motiondetector.py:239-244)
        const int cy = std::min(std::max(y, e), H - 1 - e), cx = std::min(std::max(x, e), W - 1 - e);
        background[(size_t)y * W + x] = (float)bg[(size_t)cy * W + cx];
      }
  }
  if (weights) {
    std::vector<uint16_t> kc(P);
    CPX_HIP(h, hipMemcpy(kc.data(), base + l.kcnt + (size_t)clip * P * sizeof(uint16_t), P * sizeof(uint16_t),
                         hipMemcpyDeviceToHost));
    const std::vector<double>& wt = h->wtab_host;
    const int iw = W - 2 * e, ih = H - 2 * e;
    for (int y = 0; y < ih; ++y)
      for (int x = 0; x < iw; ++x) {
        const int k = kc[(size_t)(y + e) * W + (x + e)];
        weights[(size_t)y * iw + x] = k < h->wtab_len ? wt[k] : (double)k * c.weight_add;
      }
  }
  return CPX_OK;
}

static int assoc_run(cpx_handle* h, const cpx_track_params* params, const int32_t* clip_offsets,
                     const cpx_frame_meta* meta, int B, int n_prev, bool fresh, const cpx_component* comps_dev,
                     const cpx_frame_info* info_dev, cpx_region* pool_dev,
                     cpx_track_record* tracks_dev, int32_t* n_tracks_dev, int32_t* status_dev,
                     cpx_region* regions_dev, int32_t* region_counts_dev) {
  if (params->max_active_tracks < 1 || params->max_tracks < 1)
    return fail(h, CPX_ERR_INVALID, "association: capacities must be positive");
  CPX_ENTER(h);
  const bool resume = n_prev > 0 && !fresh;
  const int t_begin = cpx::processed_before(meta, n_prev);
  cpx::Schedule sc;
  cpx::SchedLayout sl;
  int rc = build_schedule(h, clip_offsets, meta, B, &sc);
  if (rc != CPX_OK) return rc;
  rc = upload_schedule(h, sc, B, &sl);
  if (rc != CPX_OK) return rc;
  const int cap = h->cfg.max_components, ma = params->max_active_tracks;
  size_t off = 0;
  const size_t o_active = off;
  off = align_up(off + (size_t)B * ma * cpx::assoc_active_bytes(), 256);
  const size_t o_regs = off;
  off = align_up(off + (size_t)B * cap * sizeof(cpx_region), 256);
  const size_t o_scores = off;
  off = align_up(off + (size_t)B * cap * ma * cpx::assoc_score_bytes(), 256);
  const size_t o_used = off;
  off = align_up(off + (size_t)B * cap, 256);
  const size_t o_resume = off;
  off = align_up(off + (size_t)B * sizeof(cpx::AssocResume), 256);
  if (resume && off > h->ws_assoc.bytes)
    return fail(h, CPX_ERR_INVALID, "cpx_associate_frame: the stream's association state is gone");
  if ((rc = h->ws_assoc.grow(h, off, "association workspace hipMalloc"))) return rc;
  char* base = h->ws_assoc.as<char>();
  cpx::AssocArgs a{};
  a.B = B;
  a.cap = cap;
  a.params = *params;
  cpx::schedule_point(a, h->sched.as<int>(), sl);
  a.comps = comps_dev;
  a.info = info_dev;
  a.pool = pool_dev;
  a.tracks = tracks_dev;
  a.n_tracks = n_tracks_dev;
  a.status = status_dev;
  a.regions_out = regions_dev;
  a.region_counts = region_counts_dev;
  a.active = (cpx::ActiveTrack*)(base + o_active);
  a.regs = (cpx_region*)(base + o_regs);
  a.scores = (cpx::ScoreRec*)(base + o_scores);
  a.used = (unsigned char*)(base + o_used);
  a.resume = (cpx::AssocResume*)(base + o_resume);
  a.t_begin = t_begin;
  a.fresh = resume ? 0 : 1;
  cpx::launch_assoc(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_associate_batch(cpx_handle* h, const cpx_track_params* params, const int32_t* clip_offsets,
                        const cpx_frame_meta* meta, int B, const cpx_component* comps_dev,
                        const cpx_frame_info* info_dev, cpx_region* pool_dev,
                        cpx_track_record* tracks_dev, int32_t* n_tracks_dev, int32_t* status_dev,
                        cpx_region* regions_dev, int32_t* region_counts_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!params || !clip_offsets || !meta || B <= 0 || !comps_dev || !info_dev || !pool_dev || !tracks_dev ||
      !n_tracks_dev || !status_dev)
    return fail(h, CPX_ERR_INVALID, "cpx_associate_batch: null argument");
  h->stream_assoc_frames = -1;
  return assoc_run(h, params, clip_offsets, meta, B, -1, true, comps_dev, info_dev, pool_dev, tracks_dev, n_tracks_dev,
                   status_dev, regions_dev, region_counts_dev);
}

int cpx_associate_frame(cpx_handle* h, const cpx_track_params* params, const cpx_frame_meta* meta, int n_prev,
                        int n_frames, const cpx_component* comps_dev, const cpx_frame_info* info_dev,
                        cpx_region* pool_dev, cpx_track_record* tracks_dev, int32_t* n_tracks_dev,
                        int32_t* status_dev, cpx_region* regions_dev, int32_t* region_counts_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!params || !meta || !comps_dev || !info_dev || !pool_dev || !tracks_dev || !n_tracks_dev || !status_dev ||
      n_prev < 0 || n_frames <= n_prev)
    return fail(h, CPX_ERR_INVALID, "cpx_associate_frame: bad argument");
  // frames in [stream_assoc_frames, n_prev) were never handed to the association: they stay un-tracked
  const bool fresh = h->stream_assoc_frames < 0;
  if (!fresh && h->stream_assoc_frames > n_prev)
    return fail(h, CPX_ERR_INVALID, "cpx_associate_frame: n_prev is behind the frames this handle has consumed");
  const int32_t offs[2] = {0, n_frames};
  h->stream_assoc_frames = -1;
  const int rc = assoc_run(h, params, offs, meta, 1, n_prev, fresh, comps_dev, info_dev, pool_dev, tracks_dev, n_tracks_dev,
                           status_dev, regions_dev, region_counts_dev);
  if (rc == CPX_OK) h->stream_assoc_frames = n_frames;
  return rc;
}

static cpx::ClassifyArgs classify_args(const cpx_handle* h) {
  cpx::ClassifyArgs a{};
  const cpx_config& c = h->cfg;
  a.W = c.width;
  a.H = c.height;
  a.crop_x = c.edge_pixels;
  a.crop_y = c.edge_pixels;
  a.crop_w = c.width - 2 * c.edge_pixels;
  a.crop_h = c.height - 2 * c.edge_pixels;
  return a;
}

int cpx_track_limits_batch(cpx_handle* h, const uint16_t* frames_dev, const float* filtered_dev,
                           const cpx_frame_info* info_dev, const cpx_region_ref* refs_dev,
                           const int32_t* track_offsets_dev, int n_tracks, cpx_track_limits* limits_dev) {
  return cpx_track_limits_batch_ex(h, frames_dev, filtered_dev, info_dev, refs_dev, track_offsets_dev, n_tracks,
                                   limits_dev, 0);
}

int cpx_track_limits_batch_ex(cpx_handle* h, const uint16_t* frames_dev, const float* filtered_dev,
                              const cpx_frame_info* info_dev, const cpx_region_ref* refs_dev,
                              const int32_t* track_offsets_dev, int n_tracks, cpx_track_limits* limits_dev, int flags) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !filtered_dev || !info_dev || !refs_dev || !track_offsets_dev || !limits_dev || n_tracks < 0 ||
      (flags & ~(CPX_LIMITS_POST_PROCESS | CPX_LIMITS_THERMAL_DIFF_NORM | CPX_LIMITS_NO_DIFF_NORM | CPX_LIMITS_ALWAYS_CLIP |
                 CPX_LIMITS_SWAP_CHANNELS | CPX_LIMITS_TF_SCALING)))
    return fail(h, CPX_ERR_INVALID, "cpx_track_limits_batch: bad argument");
  if (n_tracks == 0) return CPX_OK;
  CPX_ENTER(h);
  if (int jrc = join_medians(h)) return jrc;  // (reads cpx_frame_info.thermal_median)
  cpx::ClassifyArgs a = classify_args(h);
  a.limits_flags = flags;
  a.frames = frames_dev;
  a.filtered = filtered_dev;
  a.info = info_dev;
  a.refs = refs_dev;
  a.track_offsets = track_offsets_dev;
  a.limits = limits_dev;
  cpx::launch_limits(a, n_tracks, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_crop_tile(cpx_handle* h, const uint16_t* frames_dev, const float* filtered_dev,
                  const cpx_frame_info* info_dev, const cpx_crop_req* reqs_dev, int n_reqs,
                  const cpx_track_limits* limits_dev, int frame_size, int square_width, float* out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !filtered_dev || !info_dev || !reqs_dev || !limits_dev || !out_dev || n_reqs < 0)
    return fail(h, CPX_ERR_INVALID, "cpx_crop_tile: null argument");
  if (frame_size < 1 || frame_size > 128 || square_width < 1 || square_width > 16)
    return fail(h, CPX_ERR_UNSUPPORTED, "cpx_crop_tile: frame_size must be 1..128, square_width 1..16");
  if (n_reqs == 0) return CPX_OK;
  CPX_ENTER(h);
  if (int jrc = join_medians(h)) return jrc;  // (reads cpx_frame_info.thermal_median)
  cpx::ClassifyArgs a = classify_args(h);
  a.frames = frames_dev;
  a.filtered = filtered_dev;
  a.info = info_dev;
  a.limits = const_cast<cpx_track_limits*>(limits_dev);
  a.reqs = reqs_dev;
  a.out = out_dev;
  a.frame_size = frame_size;
  a.square_width = square_width;
  if (cpx::launch_crop(a, n_reqs, h->stream) != 0) return fail(h, CPX_ERR_HIP, "cpx_crop_tile: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

// what cpx_finalize_tracks and cpx_plan_segments share: the schedule, and the per-clip scalar scratch of the end-of-clip
// kernels, double [B][2 * max_frames] + float [B][max_frames]
static int final_args(cpx_handle* h, const cpx_filter_params* params, const int32_t* clip_offsets,
                      const cpx_frame_meta* meta, int B, cpx::FinalArgs* a) {
  if (params->max_active_tracks < 1 || params->max_tracks_per_clip < 1)
    return fail(h, CPX_ERR_INVALID, "filter params: capacities must be positive");
  CPX_ENTER(h);
  cpx::Schedule sc;
  cpx::SchedLayout sl;
  int rc = build_schedule(h, clip_offsets, meta, B, &sc);
  if (rc != CPX_OK) return rc;
  rc = upload_schedule(h, sc, B, &sl);
  if (rc != CPX_OK) return rc;
  a->B = B;
  a->params = *params;
  a->max_frames = h->cfg.max_frames;
  cpx::schedule_point(*a, h->sched.as<int>(), sl);
  const size_t doubles = (size_t)B * h->cfg.max_frames * 2 * sizeof(double);
  rc = h->ws_assoc.grow(h, doubles + (size_t)B * h->cfg.max_frames * sizeof(float) + 512, "finalize workspace hipMalloc");
  if (rc != CPX_OK) return rc;
  a->scratch_d = h->ws_assoc.as<double>();
  a->scratch_f = (float*)(h->ws_assoc.as<char>() + align_up(doubles, 256));
  return CPX_OK;
}

int cpx_finalize_tracks(cpx_handle* h, const cpx_filter_params* params, const int32_t* clip_offsets,
                        const cpx_frame_meta* meta, int B, const cpx_region* pool_dev,
                        const cpx_track_record* tracks_dev, const int32_t* n_tracks_dev,
                        cpx_track_summary* summaries_dev, int32_t* counts_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!params || !clip_offsets || !meta || B <= 0 || !pool_dev || !tracks_dev || !n_tracks_dev || !summaries_dev ||
      !counts_dev)
    return fail(h, CPX_ERR_INVALID, "cpx_finalize_tracks: null argument");
  cpx::FinalArgs a{};
  const int rc = final_args(h, params, clip_offsets, meta, B, &a);
  if (rc != CPX_OK) return rc;
  a.square_width = 5;
  a.pool = pool_dev;
  a.tracks = tracks_dev;
  a.n_tracks = n_tracks_dev;
  a.summaries = summaries_dev;
  a.counts = counts_dev;
  cpx::launch_finalize(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_plan_segments(cpx_handle* h, const cpx_filter_params* params, const int32_t* clip_offsets,
                      const cpx_frame_meta* meta, int B, const cpx_region* pool_dev,
                      const cpx_track_summary* summaries_dev, const int32_t* n_tracks_dev,
                      const int32_t* prefix_dev, int square_width, cpx_region_ref* refs_dev,
                      int32_t* track_offsets_dev, cpx_crop_req* reqs_dev, int32_t* sample_track_dev,
                      int32_t* track_clip_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!params || !clip_offsets || !meta || B <= 0 || !pool_dev || !summaries_dev || !n_tracks_dev || !prefix_dev ||
      !refs_dev || !track_offsets_dev || !reqs_dev || !sample_track_dev || !track_clip_dev)
    return fail(h, CPX_ERR_INVALID, "cpx_plan_segments: null argument");
  if (square_width != 5) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_plan_segments: square_width must be 5");
  cpx::FinalArgs a{};
  const int rc = final_args(h, params, clip_offsets, meta, B, &a);
  if (rc != CPX_OK) return rc;
  a.square_width = square_width;
  a.pool = pool_dev;
  a.summaries = const_cast<cpx_track_summary*>(summaries_dev);
  a.n_tracks = n_tracks_dev;
  a.prefix = prefix_dev;
  a.refs = refs_dev;
  a.track_offsets = track_offsets_dev;
  a.reqs = reqs_dev;
  a.sample_track = sample_track_dev;
  a.track_clip = track_clip_dev;
  cpx::launch_plan(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_counts_prefix(cpx_handle* h, const int32_t* counts_dev, int B, int32_t* prefix_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!counts_dev || !prefix_dev || B <= 0) return fail(h, CPX_ERR_INVALID, "cpx_counts_prefix: bad argument");
  CPX_ENTER(h);
  cpx::launch_counts_prefix(counts_dev, B, prefix_dev, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_aggregate_predictions(cpx_handle* h, const float* probs_dev, const int32_t* sample_track_dev,
                              int n_samples, const cpx_crop_req* reqs_dev, int n_tracks, int n_labels,
                              int false_positive_index, int square_width, float* scores_dev, int32_t* best_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (n_tracks == 0) return CPX_OK;
  if (!probs_dev || !sample_track_dev || !reqs_dev || !scores_dev || !best_dev || n_samples < 0 || n_tracks < 0 ||
      n_labels < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_aggregate_predictions: bad argument");
  CPX_ENTER(h);
  cpx::AggregateArgs a{};
  a.n_samples = n_samples; a.n_tracks = n_tracks; a.n_labels = n_labels; a.fp_index = false_positive_index;
  a.square_width = square_width;
  a.probs = probs_dev; a.sample_track = sample_track_dev; a.reqs = reqs_dev; a.scores = scores_dev; a.best = best_dev;
  cpx::launch_aggregate(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_cptv_unpack(cpx_handle* h, const uint8_t* payload_dev, const int64_t* frame_offsets_dev,
                    const int32_t* bit_widths_dev, const int32_t* clip_offsets_dev, int B,
                    uint16_t* frames_out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!payload_dev || !frame_offsets_dev || !bit_widths_dev || !clip_offsets_dev || !frames_out_dev || B < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_cptv_unpack: bad argument");
  CPX_ENTER(h);
  cpx::CptvArgs a{};
  a.W = h->cfg.width;
  a.H = h->cfg.height;
  a.payload = payload_dev;
  a.frame_offsets = (const long long*)frame_offsets_dev;
  a.bit_widths = bit_widths_dev;
  a.clip_offsets = clip_offsets_dev;
  a.frames_out = frames_out_dev;
  const int rc = cpx::launch_cptv_unpack(a, B, h->stream);
  if (rc == -2) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_cptv_unpack: resolution too large for the unpack kernel");
  if (rc != 0) return fail(h, CPX_ERR_HIP, "cpx_cptv_unpack: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_cptv_inflate(cpx_handle* h, const uint8_t* in_dev, const cpx_cptv_file* files_dev, int B, uint8_t* out_dev,
                     cpx_cptv_frame_slot* slots_dev, uint8_t* header_dev, cpx_cptv_file_result* results_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!in_dev || !files_dev || !out_dev || !slots_dev || !results_dev || B < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_cptv_inflate: bad argument");
  CPX_ENTER(h);
  cpx::CptvInflateArgs a{};
  a.B = B;
  a.in = in_dev;
  a.files = files_dev;
  a.out = out_dev;
  a.slots = slots_dev;
  a.header = header_dev;
  a.results = results_dev;
  cpx::launch_cptv_inflate(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_cptv_gather_index(cpx_handle* h, const cpx_cptv_frame_slot* slots_dev, const int64_t* slot_offsets_dev,
                          const int32_t* clip_offsets_dev, int B, int64_t* frame_offsets_dev, int32_t* bit_widths_dev,
                          cpx_cptv_frame_slot* slots_out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!slots_dev || !slot_offsets_dev || !clip_offsets_dev || !frame_offsets_dev || !bit_widths_dev || B < 1)
    return fail(h, CPX_ERR_INVALID, "cpx_cptv_gather_index: bad argument");
  CPX_ENTER(h);
  cpx::CptvGatherArgs a{};
  a.slots = slots_dev;
  a.slot_offsets = (const long long*)slot_offsets_dev;
  a.clip_offsets = clip_offsets_dev;
  a.frame_offsets = (long long*)frame_offsets_dev;
  a.bit_widths = bit_widths_dev;
  a.slots_out = slots_out_dev;
  cpx::launch_cptv_gather(a, B, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_thumb_stats_ex(cpx_handle* h, const uint16_t* frames_dev, const int32_t* labels_dev,
                       const cpx_frame_info* info_dev, const cpx_region_ref* refs_dev, int n_refs,
                       cpx_thumb_stat* out_dev, int max_width, int max_height, int chain_capacity) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !labels_dev || !info_dev || !refs_dev || !out_dev || n_refs < 0 || max_width < 1 || max_height < 1 ||
      chain_capacity < 16 || chain_capacity > 32000)
    return fail(h, CPX_ERR_INVALID, "cpx_thumb_stats: bad argument");
  if (n_refs == 0) return CPX_OK;
  CPX_ENTER(h);
  if (int jrc = join_medians(h)) return jrc;  // (reads cpx_frame_info.thermal_median)
  cpx::ThumbArgs a{};
  a.W = h->cfg.width;
  a.H = h->cfg.height;
  a.chain_cap = chain_capacity;
  a.max_w = max_width < a.W ? max_width : a.W;
  a.max_h = max_height < a.H ? max_height : a.H;
  a.frames = frames_dev;
  a.labels = labels_dev;
  a.info = info_dev;
  a.refs = refs_dev;
  a.out = out_dev;
  const int rc = cpx::launch_thumb(a, n_refs, h->stream);
  if (rc == -2) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_thumb_stats: resolution too large for the contour kernel");
  if (rc != 0) return fail(h, CPX_ERR_HIP, "cpx_thumb_stats: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_thumb_stats(cpx_handle* h, const uint16_t* frames_dev, const int32_t* labels_dev,
                    const cpx_frame_info* info_dev, const cpx_region_ref* refs_dev, int n_refs,
                    cpx_thumb_stat* out_dev) {
  if (!h) return CPX_ERR_INVALID;
  return cpx_thumb_stats_ex(h, frames_dev, labels_dev, info_dev, refs_dev, n_refs, out_dev, h->cfg.width, h->cfg.height,
                            8192);
}

int cpx_trackless_thumb(cpx_handle* h, const uint16_t* frames_dev, int frame, int background, int32_t* out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !out_dev || frame < 0 || background < 0)
    return fail(h, CPX_ERR_INVALID, "cpx_trackless_thumb: bad argument");
  CPX_ENTER(h);
  cpx::TracklessArgs a{};
  a.W = h->cfg.width;
  a.H = h->cfg.height;
  a.frame = frame;
  a.background = background;
  a.frames = frames_dev;
  a.out = out_dev;
  const int rc = cpx::launch_trackless(a, h->stream);
  if (rc == -2) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_trackless_thumb: resolution outside the kernel's envelope");
  if (rc != 0) return fail(h, CPX_ERR_HIP, "cpx_trackless_thumb: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_trackless_thumb_batch(cpx_handle* h, const uint16_t* frames_dev, const int32_t* pairs_dev, int n, int32_t* out_dev) {
  if (!h) return CPX_ERR_INVALID;
  if (!frames_dev || !pairs_dev || !out_dev || n < 0)
    return fail(h, CPX_ERR_INVALID, "cpx_trackless_thumb_batch: bad argument");
  if (n == 0) return CPX_OK;
  CPX_ENTER(h);
  cpx::TracklessArgs a{};
  a.W = h->cfg.width;
  a.H = h->cfg.height;
  a.frames = frames_dev;
  a.out = out_dev;
  a.pairs = pairs_dev;
  a.n = n;
  const int rc = cpx::launch_trackless(a, h->stream);
  if (rc == -2) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_trackless_thumb_batch: resolution outside the kernel's envelope");
  if (rc != 0) return fail(h, CPX_ERR_HIP, "cpx_trackless_thumb_batch: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_last_kernel_timing(cpx_handle* h, float* total_ms, int* launches) {
  if (!h || !total_ms || !launches) return CPX_ERR_INVALID;
  if (!h->timing_valid) return fail(h, CPX_ERR_INVALID, "no batch has been run");
  CPX_HIP(h, hipEventSynchronize(h->ev1));
  CPX_HIP(h, hipEventElapsedTime(total_ms, h->ev0, h->ev1));
  *launches = h->last_launches;
  return CPX_OK;
}

}  // extern "C"
