// cpx_graph_core.h -- the arithmetic and the index maps the TFLite graph executor's kernels share (cpx_graph.hip,
// cpx_graph_q8.hip, cpx_graph_dw.hip): the activation, the hybrid operators' quantisation, parameters and finish
// (include/cpx.h fixes them "each operation in float32 as written"; the build has -ffp-contract=off), the test for views
// of aligned quads, the flattened-pixel maps of the implicit-GEMM convolutions (their walk: cpx_graph_conv_core.h), the
// window's origin and the depthwise work item.
// Host and device: tests/native/graph_core_host.cpp compiles it without HIP and tests/test_graph_core_host.py holds it,
// bit for bit, to the NumPy restatement (tests/tflite_eval_q8.py) and to divmod.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "cpx.h"

#ifndef CPX_HD
#ifdef __HIPCC__
#define CPX_HD __host__ __device__
#else
#define CPX_HD
#endif
#endif

namespace cpx {

// LOGISTIC, and the sigmoid of a swish: the ONE place it is written, so that a fused activation and the LOGISTIC launch
// are the same float32 operations.  expf(-v) overflows to inf for v < -88.7 (the result is 0, not NaN) and is 0 beyond 103.
CPX_HD inline float logistic(float v) { return 1.0f / (1.0f + expf(-v)); }

CPX_HD inline float activate(float v, int act) {
  if (act == CPX_GRAPH_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == CPX_GRAPH_ACT_RELU6) return fminf(fmaxf(v, 0.0f), 6.0f);
  if (act == CPX_GRAPH_ACT_SWISH) return v * logistic(v);
  if (act == CPX_GRAPH_ACT_LOGISTIC) return logistic(v);
  return v;
}

// ---- MEAN ----
// at this many pixels and above graph_mean_wide_kernel's order replaces the serial one (include/cpx.h: CPX_GRAPH_MEAN)
constexpr int GRAPH_MEAN_WIDE_PIXELS = 256;
constexpr int GRAPH_MEAN_STRIPES = 64;   // lanes that split the pixel range

// ---- the hybrid (dynamic-range quantised) arithmetic ----
// q = clamp(round-half-away(float32(x * inv)) + zp, -128, 127)
CPX_HD inline int quantise(float x, float inv, int zp) {
  const float v = x * inv;
  const int q = (int)roundf(v) + zp;
  return q < -128 ? -128 : q > 127 ? 127 : q;
}

// QUANT_PARAMS of one sample from lo = min(0, min x) and hi = max(0, max x): q = x * inv + zp, x ~ sx * (q - zp)
struct QuantParams {
  float sx, inv;
  int zp;
};
CPX_HD inline QuantParams quant_params(float lo, float hi, bool symmetric) {
  QuantParams p = {1.0f, 1.0f, 0};
  if (symmetric) {
    const float m = fmaxf(-lo, hi);
    if (m != 0.0f) {
      p.sx = (float)((double)m / 127.0);
      p.inv = (float)(127.0 / (double)m);
    }
  } else if (lo != hi) {
    const double s = ((double)hi - (double)lo) / 255.0;
    const double ql = (double)lo / s, qh = (double)hi / s;
    const double z = (128.0 + fabs(ql) < 127.0 + fabs(qh)) ? -128.0 - ql : 127.0 - qh;
    p.zp = (int)fmin(fmax(round(z), -128.0), 127.0);
    p.sx = (float)s;
    p.inv = (float)(1.0 / s);
  }
  return p;
}

// acc = sum q w over the taps (int32, exact in any order), wsum = sum w:
// activation(float32(acc - zp * wsum) * float32(sx * scale) + shift), three float32 operations in this order
CPX_HD inline float hybrid_finish(int acc, int zp, int wsum, float sx, float scale, float shift, int act) {
  const float m = sx * scale;
  const float v = (float)(acc - zp * wsum) * m;
  return activate(v + shift, act);
}

// ---- the fp16x2 convolution's range scaling ----
// RANGE of one sample from m = max |x| (include/cpx.h): m = f * 2^e with f in [0.5, 1), k = min(15 - e, 100) (>= -113),
// up = 2^k, down = 2^-k; m zero, infinite or NaN: 1, 1.  In integers on the float's bits, so that host and device agree
// whatever their frexp makes of a subnormal (a subnormal m has e <= -126: the clamp holds, k = 100).
struct RangeParams {
  float up, down;
};
CPX_HD inline float pow2f(int k) {   // 2^k for -126 <= k <= 127
  union {
    uint32_t u;
    float f;
  } v;
  v.u = (uint32_t)(127 + k) << 23;
  return v.f;
}
CPX_HD inline RangeParams range_params(float m) {
  union {
    float f;
    uint32_t u;
  } v;
  v.f = m;
  const int field = (int)((v.u >> 23) & 255);
  if (!(m > 0.0f) || field == 255) return RangeParams{1.0f, 1.0f};
  int k = field == 0 ? 100 : 15 - (field - 126);
  k = k > 100 ? 100 : k;
  return RangeParams{pow2f(k), pow2f(-k)};
}

// ---- views ----
// the view (GraphView's fields) can be read and written as aligned quads of channels: 16-byte loads and stores
template <class View>
inline bool quads(const View& v) {
  return v.C % 4 == 0 && v.cstride % 4 == 0 && v.sample_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0;
}

// ... and so can every group of a grouped convolution's input of Cg channels per group: the first channel of group g is
// c_offset + g * Cg, which must lie on a quad for EVERY g -- the view's own alignment does not say that
template <class View>
inline bool group_quads(const View& v, int cg) {
  return quads(v) && cg % 4 == 0;
}

// ---- the implicit-GEMM convolutions (cpx_graph_conv_core.h): M = the output pixels of the whole batch, flattened ----
// pixel p of P = N * HoWo -> sample, output row and column; p >= P (the last tile's surplus) is sample 0's pixel 0, not valid
struct ConvPixel {
  long long n;
  int oy, ox;
  bool valid;
};
CPX_HD inline ConvPixel conv_pixel(long long p, long long P, int HoWo, int Wo) {
  ConvPixel c;
  c.valid = p < P;
  c.n = c.valid ? p / HoWo : 0;
  const int rem = c.valid ? (int)(p - c.n * HoWo) : 0;
  c.oy = rem / Wo;
  c.ox = rem - c.oy * Wo;
  return c;
}

// the 32 x 32 accumulator of the MFMAs: register r (0..15) of a lane holds row acc_row, column lane & 31.  Bit 5 of `lane`
// alone is read, so a thread's index in its workgroup does as well as its lane
CPX_HD inline int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * ((lane >> 5) & 1); }

// the pixel `rem` (>= 0, it may run past the sample's HoWo) of sample n -> its own sample and pixel
struct SamplePixel {
  long long n;
  int rem;
};
CPX_HD inline SamplePixel sample_step(long long n, int rem, int HoWo) {
  while (rem >= HoWo) {
    rem -= HoWo;
    ++n;
  }
  return SamplePixel{n, rem};
}

// ---- windows ----
// the first input row (column) of the window of output row (column) o
CPX_HD inline int window_origin(int o, int stride, int pad) { return o * stride - pad; }

// ---- DWCONV / DWCONV_Q8 ----
// work item idx of N * Ho * runs * groups, channel group fastest, then run, output row and sample -> sample, output row,
// first output column (RUN columns per run) and first channel (4 per group)
struct DwGeom {
  size_t items;   // N * Ho * runs * groups
  int groups;     // quads of channels
  int runs;       // per output row
};
struct DwItem {
  size_t n;
  int c, oy, ox0;
};
// 32-bit divisions unless the batch needs more (items >= 2^32); false: idx is beyond the last item
template <int RUN>
CPX_HD inline bool dw_item(size_t idx, const DwGeom& g, int Ho, DwItem* it) {
  if (idx >= g.items) return false;
  if ((g.items >> 32) == 0) {
    const unsigned i = (unsigned)idx, t = i / (unsigned)g.groups, u = t / (unsigned)g.runs, n = u / (unsigned)Ho;
    it->c = 4 * (int)(i - t * g.groups);
    it->ox0 = RUN * (int)(t - u * g.runs);
    it->oy = (int)(u - n * Ho);
    it->n = n;
  } else {
    const size_t t = idx / g.groups, u = t / g.runs;
    it->c = 4 * (int)(idx - t * g.groups);
    it->ox0 = RUN * (int)(t - u * g.runs);
    it->n = u / Ho;
    it->oy = (int)(u - it->n * Ho);
  }
  return true;
}

}  // namespace cpx
