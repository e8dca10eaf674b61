// cpx_graph_dw.hip -- DEPTHWISE_CONV_2D of the TFLite graph executor (CPX_GRAPH_DWCONV / CPX_GRAPH_DWCONV_PRE /
// CPX_GRAPH_DWCONV_Q8, include/cpx.h): depth multiplier 1, kernels up to 7 x 7, strides 1 and 2; and CPX_GRAPH_SLICE, the
// strided, cropping, zero-padding copy that shares its work item and its borders (below the depthwise kernel).  A depthwise convolution does kh * kw
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
// DWCONV_Q8 is the same kernel with another arithmetic (DwFloat / DwHybrid below: the accumulator's type, the weight quad
// of a tap, the operand made of a loaded quad, the multiply-add, the finish): the float32 value is quantised as it is
// loaded, with the [sx, inv, zp] of its sample (no int8 copy goes to memory; a padded tap is a real 0, i.e. q = zp),
// plain int32 multiply-adds, and the finish of the other hybrid operators (cpx_graph_core.h).  Weights: int8
// [tap][C rounded up to 4], then int32 wsum[C rounded up to 4].
//
// DWCONV_PRE (PRE, float32 only) reads its input as act_pre(x), act_pre = (int)param: activate() on the loaded quad in
// front of operand(), the bits a graph_affine_kernel launch without constants would have stored.  act_pre(0) = 0, so a
// padded tap still contributes nothing.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cpx_graph_core.h"
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

// An arithmetic of graph_dw_kernel.  V: the quad an accumulator, an operand and a tap's weights are; Arith(a, n, c): for
// the item of sample n and channels [c, c + 4); weights(quad): the quad at that offset from the item's first;
// operand(v): of a loaded quad; mad(acc, x, w); channels(a, c, groups): the constants of the item's channels (a channel
// beyond C takes the last one's: its value is never stored), read behind the taps; finish(acc, channels, act): the output.
// Both take the same arguments, whichever of them an arithmetic reads.
//
// The float32 arithmetic: ONE chain acc = fmaf(x, w, acc) per output, then scale, shift (either may be absent), activation.
struct DwFloat {
  typedef f32x4 V;   // accumulator, operand and weight quad
  struct Channels { f32x4 sc, sh; };
  const f32x4* wq;
  __device__ __forceinline__ DwFloat(const GraphOpArgs& a, size_t n, int c) : wq(reinterpret_cast<const f32x4*>(a.weights) + (c >> 2)) {}
  __device__ __forceinline__ V weights(size_t quad) const { return wq[quad]; }
  __device__ __forceinline__ V operand(f32x4 v) const { return v; }
  static __device__ __forceinline__ void mad(V& acc, V x, V w) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = fmaf(x[e], w[e], acc[e]);
  }
  __device__ __forceinline__ Channels channels(const GraphOpArgs& a, int c, int groups) const {
    Channels k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = min(c + j, a.in0.C - 1);
      k.sc[j] = a.scale ? a.scale[ch] : 1.0f;
      k.sh[j] = a.shift ? a.shift[ch] : 0.0f;
    }
    return k;
  }
  __device__ __forceinline__ f32x4 finish(V acc, const Channels& k, int act) const {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = activate(acc[j] * k.sc[j] + k.sh[j], act);
    return v;
  }
};

// The hybrid arithmetic: quantise on load, int32 multiply-adds, hybrid_finish.
struct DwHybrid {
  typedef i32x4 V;
  const int* wq;   // four int8 channels per int
  float sx, inv;
  int zp;
  struct Channels { f32x4 sc, sh; i32x4 ws; };
  __device__ __forceinline__ DwHybrid(const GraphOpArgs& a, size_t n, int c) : wq(reinterpret_cast<const int*>(a.weights) + (c >> 2)) {
    const float* prm = a.in1.p + n * a.in1.sample_stride;
    sx = prm[0], inv = prm[1];
    zp = (int)prm[2];
  }
  __device__ __forceinline__ V weights(size_t quad) const {
    const int w = wq[quad];
    return i32x4{(int)((unsigned)w << 24) >> 24, (int)((unsigned)w << 16) >> 24, (int)((unsigned)w << 8) >> 24, w >> 24};
  }
  __device__ __forceinline__ V operand(f32x4 v) const {
    i32x4 q;
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = quantise(v[e], inv, zp);   // a masked tap is a real 0: q = zp
    return q;
  }
  static __device__ __forceinline__ void mad(V& acc, V x, V w) { acc += x * w; }
  __device__ __forceinline__ Channels channels(const GraphOpArgs& a, int c, int groups) const {
    const int* wsum = reinterpret_cast<const int*>(a.weights) + (size_t)a.kh * a.kw * groups;
    Channels k;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = min(c + j, a.in0.C - 1);
      k.sc[j] = a.scale[ch];
      k.sh[j] = a.shift[ch];
      k.ws[j] = wsum[ch];
    }
    return k;
  }
  __device__ __forceinline__ f32x4 finish(V acc, const Channels& k, int act) const {
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = hybrid_finish(acc[j], zp, k.ws[j], sx, k.sc[j], k.sh[j], act);
    return v;
  }
};

template <class Arith, bool VEC, int SW, int KWM, bool PRE>
__global__ __launch_bounds__(CT) void graph_dw_kernel(GraphOpArgs a, DwGeom g) {
  typedef typename Arith::V V;
  DwItem it;
  if (!dw_item<RUN>((size_t)blockIdx.x * CT + threadIdx.x, g, a.out.H, &it)) return;
  constexpr int NC = (RUN - 1) * SW + KWM;   // columns in registers
  const int c = it.c, C = a.in0.C, H = a.in0.H, W = a.in0.W, kw = a.kw;
  const int ncols = (RUN - 1) * SW + kw;
  const int iy0 = window_origin(it.oy, a.stride_h, a.pad_top), ix0 = window_origin(it.ox0, SW, a.pad_left);
  const float* in_n = a.in0.p + it.n * a.in0.sample_stride;
  Arith ar(a, it.n, c);

  int coff[NC];   // the columns of the run's window
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int ix = ix0 + j;
    coff[j] = j < ncols && ix >= 0 && ix < W ? ix * a.in0.cstride + c : -1;
  }
  V acc[RUN];
#pragma unroll
  for (int r = 0; r < RUN; ++r) acc[r] = V{0, 0, 0, 0};

  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = iy0 + ky;
    const int row = iy >= 0 && iy < H ? iy * W * a.in0.cstride : -1;
    V wr[KWM];
#pragma unroll
    for (int kx = 0; kx < KWM; ++kx) wr[kx] = ar.weights((size_t)(ky * kw + min(kx, kw - 1)) * g.groups);
    // column j of the run's window feeds output r as tap kx = j - r * SW: for every r the taps arrive in rising kx
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      f32x4 xin = load4<VEC>(in_n, coff[j], row, c, C);
      if (PRE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) xin[e] = activate(xin[e], (int)a.param);
      }
      const V x = ar.operand(xin);
#pragma unroll
      for (int r = 0; r < RUN; ++r) {
        const int kx = j - r * SW;
        if (kx >= 0 && kx < KWM && kx < kw) Arith::mad(acc[r], x, wr[kx < 0 ? 0 : kx < KWM ? kx : 0]);
      }
    }
  }

  const typename Arith::Channels k = ar.channels(a, c, g.groups);
  float* out_row = a.out.p + it.n * a.out.sample_stride + c;
#pragma unroll
  for (int r = 0; r < RUN; ++r) {
    const int ox = it.ox0 + r;
    if (ox >= a.out.W) break;
    store4<VEC>(out_row + (unsigned)((it.oy * a.out.W + ox) * a.out.cstride), ar.finish(acc[r], k, a.act), c, C);
  }
}

// the instantiation by [16-byte path][stride 2 along W][more than 3 columns]
template <class Arith, bool PRE>
void launch_dw(const GraphOpArgs& a, hipStream_t s) {
  typedef void (*Kernel)(GraphOpArgs, DwGeom);
  static const Kernel kernels[2][2][2] = {
      {{graph_dw_kernel<Arith, false, 1, 3, PRE>, graph_dw_kernel<Arith, false, 1, 7, PRE>},
       {graph_dw_kernel<Arith, false, 2, 3, PRE>, graph_dw_kernel<Arith, false, 2, 7, PRE>}},
      {{graph_dw_kernel<Arith, true, 1, 3, PRE>, graph_dw_kernel<Arith, true, 1, 7, PRE>},
       {graph_dw_kernel<Arith, true, 2, 3, PRE>, graph_dw_kernel<Arith, true, 2, 7, PRE>}}};
  DwGeom g;
  g.groups = (a.out.C + 3) / 4;
  g.runs = (a.out.W + RUN - 1) / RUN;
  g.items = (size_t)a.N * a.out.H * g.runs * g.groups;
  const bool vec = quads(a.in0) && quads(a.out);
  hipLaunchKernelGGL(kernels[vec][a.stride_w != 1][a.kw > 3], dim3((unsigned)((g.items + CT - 1) / CT)), dim3(CT), 0, s, a, g);
}

// SLICE: out[n, y, x, c] = act(in0[n, y * stride_h - pad_top, x * stride_w - pad_left, c]), 0 outside the input (a signed
// pad: negative crops, positive pads with zeros; act(0) = 0).  A copy: the depthwise work item with a run of one pixel
// and its branch-free border, one 16-byte load and store per item (VEC) or channel by channel; no LDS.  param 1: the
// value goes through v + 0.0f behind the activation, which is what graph_pool_kernel's sum from 0 makes of the one
// element of a 1 x 1 AVERAGE_POOL_2D: a -0.0 becomes +0.0, every other value is itself.  The grid is
// capped and strided over: a large batch re-uses its workgroups instead of launching millions of them.
constexpr unsigned SLICE_MAX_BLOCKS = 16384;

template <bool VEC>
__global__ __launch_bounds__(CT) void graph_slice_kernel(GraphOpArgs a, DwGeom g) {
  const int C = a.in0.C, H = a.in0.H, W = a.in0.W;
  for (size_t idx = (size_t)blockIdx.x * CT + threadIdx.x; idx < g.items; idx += (size_t)gridDim.x * CT) {
    DwItem it;
    dw_item<1>(idx, g, a.out.H, &it);
    const int iy = window_origin(it.oy, a.stride_h, a.pad_top), ix = window_origin(it.ox0, a.stride_w, a.pad_left);
    const int col = ix >= 0 && ix < W ? ix * a.in0.cstride + it.c : -1;
    const int row = iy >= 0 && iy < H ? iy * W * a.in0.cstride : -1;
    f32x4 v = load4<VEC>(a.in0.p + it.n * a.in0.sample_stride, col, row, it.c, C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = activate(v[e], a.act);
      v[e] = a.param != 0.0f ? v[e] + 0.0f : v[e];
    }
    store4<VEC>(a.out.p + it.n * a.out.sample_stride + it.c + (unsigned)((it.oy * a.out.W + it.ox0) * a.out.cstride), v, it.c, C);
  }
}

void launch_slice(const GraphOpArgs& a, hipStream_t s) {
  DwGeom g;
  g.groups = (a.out.C + 3) / 4;
  g.runs = a.out.W;
  g.items = (size_t)a.N * a.out.H * g.runs * g.groups;
  const unsigned blocks = (unsigned)std::min<size_t>((g.items + CT - 1) / CT, SLICE_MAX_BLOCKS);
  if (quads(a.in0) && quads(a.out))
    hipLaunchKernelGGL(graph_slice_kernel<true>, dim3(blocks), dim3(CT), 0, s, a, g);
  else
    hipLaunchKernelGGL(graph_slice_kernel<false>, dim3(blocks), dim3(CT), 0, s, a, g);
}

}  // namespace

void launch_graph_dw_op(const GraphOpArgs& a, hipStream_t s) {
  if (a.kind == CPX_GRAPH_SLICE)
    launch_slice(a, s);
  else if (a.kind == CPX_GRAPH_DWCONV_Q8)
    launch_dw<DwHybrid, false>(a, s);
  else if (a.kind == CPX_GRAPH_DWCONV_PRE)
    launch_dw<DwFloat, true>(a, s);
  else
    launch_dw<DwFloat, false>(a, s);
}

}  // namespace cpx
