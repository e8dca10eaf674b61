// cpx_graph_dw.hip -- DEPTHWISE_CONV_2D of the TFLite graph executor (CPX_GRAPH_DWCONV / CPX_GRAPH_DWCONV_Q8,
// include/cpx.h): depth multiplier 1, kernels up to 7 x 7, strides 1 and 2.  A depthwise convolution does kh * kw
// multiply-adds per output element against about 8 bytes moved, far below the vector ridge: the matrix pipe has
// nothing to offer, the job is to move every byte once, 16 bytes per lane.
//
// Work item = 4 consecutive channels (one 16-byte load and store) of a run of GRAPH_DW_RUN output pixels along W of one
// output row.  Items are numbered channel group fastest, then run, row and sample -- flattened over the whole batch, as
// graph_conv_kernel's M is -- so consecutive lanes read consecutive 16 bytes of a pixel.  For every filter row the item
// loads the (RUN - 1) * stride + kw input columns the run touches once, each feeding every output it is a tap of; the filter
// row's kw quads of weights ([tap][C rounded up to 4]) are 16-byte loads every pixel of the channel group shares
// through the cache.  Borders are branch-free: a tap outside the image reads the sample's first element and is zeroed.
//
// The sum of an output is ONE chain, acc = fmaf(x, w, acc) over the taps in raster order (ky outer, kx inner) from 0,
// whichever instantiation runs it and wherever the pixel sits in a run, a sample or a batch.  The instantiations: VEC
// (16-byte loads and stores: C, the pointers and the strides are multiples of 4 floats) or channel by channel (a
// 3-channel input, an odd concatenation slice); the stride along W; kernels up to 3 or up to 7 wide (the number of
// columns kept in registers).
//
// DWCONV_Q8: the same loads; the float32 value is quantised as it is loaded, with the [sx, inv, zp] of its sample (no
// int8 copy goes to memory; a padded tap is a real 0, i.e. q = zp), plain int32 multiply-adds, and the epilogue of the
// other hybrid operators.  Weights: int8 [tap][C rounded up to 4], then int32 wsum[C rounded up to 4].
#include <hip/hip_runtime.h>

#include "cpx_kernels.h"

namespace cpx {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int CT = 256;
#ifndef GRAPH_DW_RUN
#define GRAPH_DW_RUN 4
#endif
constexpr int RUN = GRAPH_DW_RUN;   // output pixels of a work item (measured: DESIGN.md section 6)

struct DwGeom {
  size_t items;   // N * Ho * runs * groups
  int groups;     // quads of channels
  int runs;       // per output row
};

__device__ __forceinline__ float activate(float v, int act) {
  if (act == CPX_GRAPH_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == CPX_GRAPH_ACT_RELU6) return fminf(fmaxf(v, 0.0f), 6.0f);
  return v;
}

// q = clamp(round-half-away(float32(x * inv)) + zp, -128, 127), as cpx_graph_q8.hip
__device__ __forceinline__ int quantise(float x, float inv, int zp) {
  const float v = x * inv;
  const int q = (int)roundf(v) + zp;
  return min(max(q, -128), 127);
}

// Channels [c, c + 4) of the element at col + row floats from the sample's start: `col` is the column's offset in a row
// (with the channel), `row` the row's; either is -1 where the tap lies outside the image, and the value is then 0 (the
// load reads the sample's first element).  The mask travels in the two signs and is tested where the value is used: as
// one lane mask per column, worked out in front of the loop over the filter rows, it overflows the scalar registers.
// Channel by channel, a channel beyond C reads the view's last one: its sums are never stored.
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* in_n, int col, int row, int c, int C) {
  const int out = (col | row) >> 31;   // -1: masked
  const float* p = in_n + ((col + row) & ~out);
  f32x4 v;
  if (VEC) {
    v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = p[min(j, C - 1 - c)];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = out ? 0.0f : v[j];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* dst, f32x4 v, int c, int C) {
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < C) dst[j] = v[j];
  }
}

struct DwItem {
  size_t n;
  int c, oy, ox0;
};

// item -> (sample, output row, first output column, first channel); 32-bit divisions unless the batch needs more
__device__ __forceinline__ bool dw_item(const GraphOpArgs& a, const DwGeom& g, DwItem* it) {
  const size_t idx = (size_t)blockIdx.x * CT + threadIdx.x;
  if (idx >= g.items) return false;
  if ((g.items >> 32) == 0) {
    const unsigned i = (unsigned)idx, t = i / (unsigned)g.groups, u = t / (unsigned)g.runs, n = u / (unsigned)a.out.H;
    it->c = 4 * (int)(i - t * g.groups);
    it->ox0 = RUN * (int)(t - u * g.runs);
    it->oy = (int)(u - n * a.out.H);
    it->n = n;
  } else {
    const size_t t = idx / g.groups, u = t / g.runs;
    it->c = 4 * (int)(idx - t * g.groups);
    it->ox0 = RUN * (int)(t - u * g.runs);
    it->n = u / a.out.H;
    it->oy = (int)(u - it->n * a.out.H);
  }
  return true;
}

template <bool VEC, int SW, int KWM>
__global__ __launch_bounds__(CT) void graph_dw_kernel(GraphOpArgs a, DwGeom g) {
  DwItem it;
  if (!dw_item(a, g, &it)) return;
  constexpr int NC = (RUN - 1) * SW + KWM;   // columns in registers
  const int c = it.c, C = a.in0.C, H = a.in0.H, W = a.in0.W, kw = a.kw;
  const int ncols = (RUN - 1) * SW + kw;
  const int iy0 = it.oy * a.stride_h - a.pad_top, ix0 = it.ox0 * SW - a.pad_left;
  const float* in_n = a.in0.p + it.n * a.in0.sample_stride;
  const f32x4* wq = reinterpret_cast<const f32x4*>(a.weights) + (c >> 2);

  int coff[NC];   // the columns of the run's window
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int ix = ix0 + j;
    coff[j] = j < ncols && ix >= 0 && ix < W ? ix * a.in0.cstride + c : -1;
  }
  f32x4 acc[RUN];
#pragma unroll
  for (int r = 0; r < RUN; ++r) acc[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = iy0 + ky;
    const int row = iy >= 0 && iy < H ? iy * W * a.in0.cstride : -1;
    f32x4 wr[KWM];
#pragma unroll
    for (int kx = 0; kx < KWM; ++kx) wr[kx] = wq[(size_t)(ky * kw + min(kx, kw - 1)) * g.groups];
    // column j of the run's window feeds output r as tap kx = j - r * SW: for every r the taps arrive in rising kx
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const f32x4 v = load4<VEC>(in_n, coff[j], row, c, C);
#pragma unroll
      for (int r = 0; r < RUN; ++r) {
        const int kx = j - r * SW;
        if (kx >= 0 && kx < KWM && kx < kw)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[r][e] = fmaf(v[e], wr[kx < 0 ? 0 : kx < KWM ? kx : 0][e], acc[r][e]);
      }
    }
  }

  f32x4 sc, sh;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ch = min(c + j, C - 1);
    sc[j] = a.scale ? a.scale[ch] : 1.0f;
    sh[j] = a.shift ? a.shift[ch] : 0.0f;
  }
  float* out_row = a.out.p + it.n * a.out.sample_stride + c;
#pragma unroll
  for (int r = 0; r < RUN; ++r) {
    const int ox = it.ox0 + r;
    if (ox >= a.out.W) break;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = activate(acc[r][j] * sc[j] + sh[j], a.act);
    store4<VEC>(out_row + (unsigned)((it.oy * a.out.W + ox) * a.out.cstride), v, c, C);
  }
}

template <bool VEC, int SW, int KWM>
__global__ __launch_bounds__(CT) void graph_dw_q8_kernel(GraphOpArgs a, DwGeom g) {
  DwItem it;
  if (!dw_item(a, g, &it)) return;
  constexpr int NC = (RUN - 1) * SW + KWM;
  const int c = it.c, C = a.in0.C, H = a.in0.H, W = a.in0.W, kw = a.kw;
  const int ncols = (RUN - 1) * SW + kw;
  const int iy0 = it.oy * a.stride_h - a.pad_top, ix0 = it.ox0 * SW - a.pad_left;
  const float* in_n = a.in0.p + it.n * a.in0.sample_stride;
  const float* prm = a.in1.p + it.n * a.in1.sample_stride;
  const float sx = prm[0], inv = prm[1];
  const int zp = (int)prm[2];
  const int* wq = reinterpret_cast<const int*>(a.weights) + (c >> 2);   // four int8 channels per int

  int coff[NC];   // the columns of the run's window
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int ix = ix0 + j;
    coff[j] = j < ncols && ix >= 0 && ix < W ? ix * a.in0.cstride + c : -1;
  }
  i32x4 acc[RUN];
#pragma unroll
  for (int r = 0; r < RUN; ++r) acc[r] = i32x4{0, 0, 0, 0};

  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = iy0 + ky;
    const int row = iy >= 0 && iy < H ? iy * W * a.in0.cstride : -1;
    i32x4 wr[KWM];
#pragma unroll
    for (int kx = 0; kx < KWM; ++kx) {
      const int w = wq[(size_t)(ky * kw + min(kx, kw - 1)) * g.groups];
      wr[kx] = i32x4{(int)((unsigned)w << 24) >> 24, (int)((unsigned)w << 16) >> 24, (int)((unsigned)w << 8) >> 24, w >> 24};
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const f32x4 v = load4<VEC>(in_n, coff[j], row, c, C);
      i32x4 q;
#pragma unroll
      for (int e = 0; e < 4; ++e) q[e] = quantise(v[e], inv, zp);   // a masked tap is a real 0: q = zp
#pragma unroll
      for (int r = 0; r < RUN; ++r) {
        const int kx = j - r * SW;
        if (kx >= 0 && kx < KWM && kx < kw) acc[r] += q * wr[kx < 0 ? 0 : kx < KWM ? kx : 0];
      }
    }
  }

  const int* wsum = reinterpret_cast<const int*>(a.weights) + (size_t)a.kh * kw * g.groups;
  f32x4 m, sh;
  i32x4 zw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ch = min(c + j, C - 1);
    m[j] = sx * a.scale[ch];
    sh[j] = a.shift[ch];
    zw[j] = zp * wsum[ch];
  }
  float* out_row = a.out.p + it.n * a.out.sample_stride + c;
#pragma unroll
  for (int r = 0; r < RUN; ++r) {
    const int ox = it.ox0 + r;
    if (ox >= a.out.W) break;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = (float)(acc[r][j] - zw[j]) * m[j];
      v[j] = activate(p + sh[j], a.act);
    }
    store4<VEC>(out_row + (unsigned)((it.oy * a.out.W + ox) * a.out.cstride), v, c, C);
  }
}

bool quads(const GraphView& v) {
  return v.C % 4 == 0 && v.cstride % 4 == 0 && v.sample_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0;
}

template <bool Q8, bool VEC, int SW>
void launch_dw(const GraphOpArgs& a, const DwGeom& g, hipStream_t s) {
  const dim3 grid((unsigned)((g.items + CT - 1) / CT)), block(CT);
  if (Q8) {
    if (a.kw <= 3)
      hipLaunchKernelGGL((graph_dw_q8_kernel<VEC, SW, 3>), grid, block, 0, s, a, g);
    else
      hipLaunchKernelGGL((graph_dw_q8_kernel<VEC, SW, 7>), grid, block, 0, s, a, g);
  } else {
    if (a.kw <= 3)
      hipLaunchKernelGGL((graph_dw_kernel<VEC, SW, 3>), grid, block, 0, s, a, g);
    else
      hipLaunchKernelGGL((graph_dw_kernel<VEC, SW, 7>), grid, block, 0, s, a, g);
  }
}

template <bool Q8>
void launch_dw(const GraphOpArgs& a, hipStream_t s) {
  DwGeom g;
  g.groups = (a.out.C + 3) / 4;
  g.runs = (a.out.W + RUN - 1) / RUN;
  g.items = (size_t)a.N * a.out.H * g.runs * g.groups;
  const bool vec = quads(a.in0) && quads(a.out);
  if (vec) {
    if (a.stride_w == 1)
      launch_dw<Q8, true, 1>(a, g, s);
    else
      launch_dw<Q8, true, 2>(a, g, s);
  } else {
    if (a.stride_w == 1)
      launch_dw<Q8, false, 1>(a, g, s);
    else
      launch_dw<Q8, false, 2>(a, g, s);
  }
}

}  // namespace

void launch_graph_dw_op(const GraphOpArgs& a, hipStream_t s) {
  if (a.kind == CPX_GRAPH_DWCONV_Q8)
    launch_dw<true>(a, s);
  else
    launch_dw<false>(a, s);
}

}  // namespace cpx
