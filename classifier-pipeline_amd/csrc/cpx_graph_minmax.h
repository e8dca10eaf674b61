// cpx_graph_minmax.h -- the per-sample reduction QUANT_PARAMS (cpx_graph_q8.hip) and RANGE (cpx_graph_h2.hip) share: one
// workgroup of GRAPH_MINMAX_THREADS per sample finds lo = min(0, min x) and hi = max(0, max x) over a view's own channels.
// fminf / fmaxf pass a NaN element by; minimum and maximum do not depend on the order.  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "cpx_kernels.h"

namespace cpx {

constexpr int GRAPH_MINMAX_THREADS = 1024;

// VW = 4: the view's pixels are rows of C / 4 aligned quads.  A thread's (pixel, quad) advances by the workgroup's size
// without a division.  Every thread of the workgroup calls it (one barrier inside); the result is valid in thread 0 ALONE.
template <int VW>
__device__ __forceinline__ void sample_min_max(const GraphView& in, size_t n, float* lo_out, float* hi_out) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  constexpr int QT = GRAPH_MINMAX_THREADS;
  __shared__ float s_lo[QT / 64], s_hi[QT / 64];
  const int tid = threadIdx.x;
  const float* src = in.p + n * in.sample_stride;
  const int per = in.C / VW, HW = in.H * in.W;   // vectors per pixel
  const int dp = QT / per, dq = QT - dp * per;
  int pix = tid / per, q = tid - pix * per;
  float lo = 0.0f, hi = 0.0f;   // rmin = min(0, min x), rmax = max(0, max x)
  while (pix < HW) {
    const float* e = src + (unsigned)pix * (unsigned)in.cstride + VW * q;
    if (VW == 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(e);
      lo = fminf(fminf(lo, fminf(v.x, v.y)), fminf(v.z, v.w));
      hi = fmaxf(fmaxf(hi, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    } else {
      lo = fminf(lo, *e);
      hi = fmaxf(hi, *e);
    }
    pix += dp;
    q += dq;
    if (q >= per) {
      q -= per;
      ++pix;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  if ((tid & 63) == 0) {
    s_lo[tid >> 6] = lo;
    s_hi[tid >> 6] = hi;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < QT / 64; ++w) {
    lo = fminf(lo, s_lo[w]);
    hi = fmaxf(hi, s_hi[w]);
  }
  *lo_out = lo;
  *hi_out = hi;
}

}  // namespace cpx
