// cpx_graph.hip -- the float32 kernels of the TFLite graph executor (cpx_graph_forward, include/cpx.h; what the
// reference's LiteInterpreter hands to the TFLite runtime, ml_tools/interpreter.py:520-560; the hybrid operators are
// cpx_graph_q8.hip's, the fp16x2 convolution is cpx_graph_h2.hip's, DEPTHWISE_CONV_2D is cpx_graph_dw.hip's, what they share is cpx_graph_core.h and cpx_graph_conv_core.h).  One launch per planned
// operator; every kernel reads and writes NHWC views with a channel offset and a row stride, so that the producers of a
// CONCATENATION write straight into their slice of the concatenated tensor.
//
// CONV_2D is an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact float32 in, float32 accumulate: a k-ordered fmaf chain
// per output, the same chain wherever the pixel sits in a tile or a batch) over the shared walk (cpx_graph_conv_core.h),
// K as (tap) x (chunk of 16 input channels) x (pair of channels), NTN = 1 or 2 tiles per wave.
// Weights arrive [tap][Cin rounded up to 16][Cout rounded up to 32] with zeros beyond, so only the activation side is
// masked.  Scale / shift (bias, folded MUL / ADD), the activation and the channel-sliced store happen from the accumulators.
// CONV_PRE is the same kernel with a prologue: the pre-activation act(x * pre_scale[c] + pre_shift[c]) of a DenseNet /
// ResNetV2 block is applied to the patch on its way from memory to LDS, as the WR-ResNet kernels do (cpx_cnn_bf3.hip), so
// the AFFINE launch in front of the convolution and its round trip through memory go away.
// CONV_GROUPED is the same kernel once more: one launch for all groups, each with its own weight image (include/cpx.h).
#include <hip/hip_runtime.h>

#include "cpx_graph_conv_core.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

constexpr int KC = GRAPH_CONV_KC;  // input channels per staged chunk
constexpr int AP = BM + 4;         // row stride of the k-major patch image: the two 8-channel halves of a pixel land 32 banks apart

// PRE: the input is read as activate(x * pre_scale[c] + pre_shift[c], (int)a.param), the two float32 operations and the
// activation of graph_affine_kernel; the constants sit behind the filter image, pre_scale[cin_pad] then pre_shift[cin_pad]
// GRP (CONV_GROUPED): blockIdx.z is the group.  The walk is CONV's over the group's own Cg input channels, with the group's
// own weight image; only the base channel of the loads, the image and the channel bound / base of the store differ, so a
// group's outputs are CONV's of that channel slice bit for bit.  scale / shift are indexed by the absolute channel.
template <int NTN, bool PRE, bool GRP = false>
__global__ __launch_bounds__(CT) void graph_conv_kernel(GraphOpArgs a, ConvGeom g) {
  static_assert(!(PRE && GRP), "there is no grouped CONV_PRE");
  constexpr int BN = 32 * NTN;
  __shared__ __attribute__((aligned(16))) float s_a[KC * AP];   // [k][pixel]
  __shared__ __attribute__((aligned(16))) float s_b[KC * BN];   // [k][channel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * BM;
  const int cout0 = blockIdx.y * BN;
  const int grp = GRP ? (int)blockIdx.z : 0;
  const int Cin = GRP ? g.cg : a.in0.C;     // the channels of the K walk
  const int Cout = GRP ? g.cog : a.out.C, ch_base = GRP ? grp * g.cog : 0;
  const int cin_pad = g.nchunks * KC, cout_pad = g.ntiles * GRAPH_CONV_CO;   // the filter image's
  const float* wimg = GRP ? a.weights + (size_t)grp * a.kh * a.kw * cin_pad * cout_pad : a.weights;

  const ConvStager<float> st = conv_stager(a, g, a.in0.p, p0, tid, GRP ? grp * g.cg : 0);
  const int spx = st.spx, half = st.half;
  // weight staging: KC rows of BN channels = KC * BN / 4 float4 (one per thread with NTN = 2)
  constexpr int WQ = BN / 4;
  const int wk = tid / WQ, wc4 = tid - wk * WQ;
  const bool wload = tid < KC * WQ;

  const int steps = a.kh * a.kw * g.nchunks;

  f32x16 acc[NTN];
#pragma unroll
  for (int t = 0; t < NTN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  float pre[8];
  f32x4 pre_w = {0.0f, 0.0f, 0.0f, 0.0f};
  const float* pre_scale = a.weights + (size_t)a.kh * a.kw * cin_pad * cout_pad;
  // activate() for the two codes a pre-activation has, without its branches: fminf(fmaxf(v, 0), 6 or inf), the same bits
  const float pre_hi = (int)a.param == CPX_GRAPH_ACT_RELU6 ? 6.0f : INFINITY;
  f32x4 pre_sc[2], pre_sh[2];
  bool pre_in = false;

  // global -> registers of step s
  auto fetch = [&](int s) {
    const ConvPatch f = conv_patch(a, st, s, g.nchunks, KC);
    if (g.vec) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const bool ok = f.inside && (f.c + 4 * q) < Cin;   // Cin % 4 == 0: a quad is valid as a whole
        const f32x4 v = *reinterpret_cast<const f32x4*>(st.in_n + (ok ? f.pix + f.c + 4 * q : 0));
        pre[4 * q + 0] = ok ? v.x : 0.0f;
        pre[4 * q + 1] = ok ? v.y : 0.0f;
        pre[4 * q + 2] = ok ? v.z : 0.0f;
        pre[4 * q + 3] = ok ? v.w : 0.0f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool ok = f.inside && (f.c + j) < Cin;
        const float v = st.in_n[ok ? f.pix + f.c + j : 0];
        pre[j] = ok ? v : 0.0f;
      }
    }
    if (PRE) {
      // the constants of this step's channels travel with the patch, and whether the mask let the pixel through: the
      // prologue itself waits until the values are needed (below), so the loads stay in flight under the MFMAs.
      // c + 8 <= cin_pad and the image in front is a multiple of 16 x 32 floats: the quads are in bounds and aligned
      pre_in = f.inside;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        pre_sc[q] = *reinterpret_cast<const f32x4*>(pre_scale + f.c + 4 * q);
        pre_sh[q] = *reinterpret_cast<const f32x4*>(pre_scale + cin_pad + f.c + 4 * q);
      }
    }
    if (wload)
      pre_w = *reinterpret_cast<const f32x4*>(wimg + ((size_t)(f.tap * cin_pad + f.c0 + wk) * cout_pad + cout0 + 4 * wc4));
  };

  fetch(0);
  for (int s = 0; s < steps; ++s) {
    if (PRE) {
      // the prologue, behind the mask: a padded tap and a pixel beyond the batch stay exactly 0, not act(pre_shift); a
      // channel beyond Cin was fetched as 0 and its constants are the image's zero padding: 0 * 0 + 0
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = pre[j];
        v *= pre_sc[j >> 2][j & 3];
        v += pre_sh[j >> 2][j & 3];
        v = fminf(fmaxf(v, 0.0f), pre_hi);
        pre[j] = pre_in ? v : 0.0f;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s_a[(8 * half + j) * AP + spx] = pre[j];
    if (wload) *reinterpret_cast<f32x4*>(s_b + wk * BN + 4 * wc4) = pre_w;
    __syncthreads();
    if (s + 1 < steps) fetch(s + 1);   // in flight while the matrix cores work on step s
    const float* ap = s_a + (lane >> 5) * AP + 32 * wave + (lane & 31);
    const float* bp = s_b + (lane >> 5) * BN + (lane & 31);
#pragma unroll
    for (int k2 = 0; k2 < KC / 2; ++k2) {
      const float av = ap[2 * k2 * AP];
#pragma unroll
      for (int t = 0; t < NTN; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * k2 * BN + 32 * t], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }

  // epilogue: accumulator register r of a lane is pixel acc_row(r, tid) of the wave's 32, channel lane & 31 of the
  // tile: 32 lanes store 128 contiguous bytes of one pixel
  const long long pb = p0 + 32 * wave;
  if (pb >= g.P) return;
  const long long nb = pb / g.HoWo;
  const int remb = (int)(pb - nb * g.HoWo);
#pragma unroll
  for (int t = 0; t < NTN; ++t) {
    const int chl = cout0 + 32 * t + (lane & 31);   // within the group: the bound is the group's own
    if (chl >= Cout) continue;
    const int ch = ch_base + chl;
    const float sc = a.scale ? a.scale[ch] : 1.0f;
    const float sh = a.shift ? a.shift[ch] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(r, tid);
      if (pb + i >= g.P) continue;
      const SamplePixel o = sample_step(nb, remb + i, g.HoWo);
      a.out.p[(size_t)o.n * a.out.sample_stride + (unsigned)(o.rem * a.out.cstride + ch)] = activate(acc[t][r] * sc + sh, a.act);
    }
  }
}

// one thread per output element, channel fastest
__device__ __forceinline__ bool out_coords(const GraphOpArgs& a, size_t idx, size_t* n, int* y, int* x, int* c) {
  const size_t total = (size_t)a.N * a.out.H * a.out.W * a.out.C;
  if (idx >= total) return false;
  *c = (int)(idx % a.out.C);
  size_t p = idx / a.out.C;
  *x = (int)(p % a.out.W);
  p /= a.out.W;
  *y = (int)(p % a.out.H);
  *n = p / a.out.H;
  return true;
}

__device__ __forceinline__ float* at(const GraphView& v, size_t n, int y, int x, int c) {
  return v.p + n * v.sample_stride + (unsigned)((y * v.W + x) * v.cstride + c);
}

template <bool MAX>
__global__ __launch_bounds__(CT) void graph_pool_kernel(GraphOpArgs a) {
  size_t n;
  int oy, ox, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &oy, &ox, &c)) return;
  const int iy0 = oy * a.stride_h - a.pad_top, ix0 = ox * a.stride_w - a.pad_left;
  float v = MAX ? -INFINITY : 0.0f;
  int count = 0;
  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = iy0 + ky;
    if (iy < 0 || iy >= a.in0.H) continue;
    for (int kx = 0; kx < a.kw; ++kx) {
      const int ix = ix0 + kx;
      if (ix < 0 || ix >= a.in0.W) continue;
      const float e = *at(a.in0, n, iy, ix, c);
      v = MAX ? fmaxf(v, e) : v + e;
      ++count;
    }
  }
  if (!MAX) v = v / (float)max(count, 1);   // the divisor leaves the padding out, as TFLite's AVERAGE_POOL_2D
  *at(a.out, n, oy, ox, c) = activate(v, a.act);
}

__global__ __launch_bounds__(CT) void graph_add_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  *at(a.out, n, y, x, c) = activate(*at(a.in0, n, y, x, c) + a.param * *at(a.in1, n, y, x, c), a.act);
}

__global__ __launch_bounds__(CT) void graph_affine_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  float v = *at(a.in0, n, y, x, c);
  if (a.scale) v *= a.scale[c];
  if (a.shift) v += a.shift[c];
  *at(a.out, n, y, x, c) = activate(v, a.act);
}

__global__ __launch_bounds__(CT) void graph_pad_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  const int iy = y - a.pad_top, ix = x - a.pad_left;
  const bool inside = iy >= 0 && iy < a.in0.H && ix >= 0 && ix < a.in0.W;
  *at(a.out, n, y, x, c) = inside ? *at(a.in0, n, iy, ix, c) : 0.0f;
}

__global__ __launch_bounds__(CT) void graph_channel_map_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  *at(a.out, n, y, x, c) = *at(a.in0, n, y, x, a.map[c]);
}

// INPUT: the channel map with the 'caffe' / 'torch' arithmetic of keras.applications' preprocess_input, each operation
// one correctly rounded float32 operation as written (include/cpx.h); a NULL scale: no second division
__global__ __launch_bounds__(CT) void graph_input_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  float v = *at(a.in0, n, y, x, a.map[c]) / a.param;
  v -= a.shift[c];
  if (a.scale) v = v / a.scale[c];
  *at(a.out, n, y, x, c) = v;
}

// MEAN over H and W below GRAPH_MEAN_WIDE_PIXELS pixels: one thread per (sample, channel), pixels in order
// (channel-contiguous loads across the wave)
__global__ __launch_bounds__(CT) void graph_mean_kernel(GraphOpArgs a) {
  const size_t idx = (size_t)blockIdx.x * CT + threadIdx.x;
  if (idx >= (size_t)a.N * a.in0.C) return;
  const int c = (int)(idx % a.in0.C);
  const size_t n = idx / a.in0.C;
  const float* src = a.in0.p + n * a.in0.sample_stride + c;
  const int hw = a.in0.H * a.in0.W;
  float sum = 0.0f;
  for (int i = 0; i < hw; ++i) sum += src[(unsigned)(i * a.in0.cstride)];
  a.out.p[n * a.out.sample_stride + c] = sum / (float)hw;
}

// MEAN over H and W from GRAPH_MEAN_WIDE_PIXELS pixels on (the 80 x 80 map in front of an EfficientNet's first
// squeeze-and-excite block: 6400 dependent loads per thread of the kernel above, a few dozen threads at N = 1).  A
// workgroup per (sample, MEAN_QG quads of channels); thread = (stripe, quad), quad fastest, so the MEAN_QG lanes of a
// stripe read 16 * MEAN_QG contiguous bytes of a pixel.  Stripe i of GRAPH_MEAN_STRIPES sums the pixels i, i + 64, ... in
// that order (independent loads, one chain of adds); the tree s[i] += s[i + d], d = 32 .. 1, combines them in LDS --
// 16-byte reads of consecutive threads, no bank conflict.  The order depends on H * W alone: not on N, on the channel
// slice, on VEC or on where the workgroup runs.  VEC: 16-byte loads; otherwise channel by channel, a channel beyond C
// reads the view's last one and is not stored.
constexpr int MEAN_QG = CT / GRAPH_MEAN_STRIPES;   // quads of channels per workgroup

template <bool VEC>
__global__ __launch_bounds__(CT) void graph_mean_wide_kernel(GraphOpArgs a, int groups) {
  __shared__ __attribute__((aligned(16))) f32x4 s_sum[CT];
  const int tid = threadIdx.x, stripe = tid / MEAN_QG, q = tid - stripe * MEAN_QG;
  const size_t n = blockIdx.x / (unsigned)groups;
  const int grp = (int)(blockIdx.x - n * (unsigned)groups);
  const int c = 4 * (grp * MEAN_QG + q), C = a.in0.C;
  const int hw = a.in0.H * a.in0.W;
  f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
  if (c < C) {
    const float* src = a.in0.p + n * a.in0.sample_stride + c;
    auto load = [&](int i) {
      const float* p = src + (unsigned)(i * a.in0.cstride);
      f32x4 v;
      if (VEC) {
        v = *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[min(j, C - 1 - c)];
      }
      return v;
    };
    // four loads in flight, added in the stripe's order
    constexpr int S = GRAPH_MEAN_STRIPES;
    int i = stripe;
    for (; i + 3 * S < hw; i += 4 * S) {
      const f32x4 v0 = load(i), v1 = load(i + S), v2 = load(i + 2 * S), v3 = load(i + 3 * S);
      sum += v0;
      sum += v1;
      sum += v2;
      sum += v3;
    }
    for (; i < hw; i += S) sum += load(i);
  }
  s_sum[tid] = sum;
  __syncthreads();
#pragma unroll
  for (int d = GRAPH_MEAN_STRIPES / 2; d >= 1; d >>= 1) {
    if (stripe < d) s_sum[tid] += s_sum[tid + d * MEAN_QG];
    __syncthreads();
  }
  if (stripe == 0 && c < C) {
    const f32x4 v = s_sum[tid];
    float* dst = a.out.p + n * a.out.sample_stride + c;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c + j < C) dst[j] = v[j] / (float)hw;
  }
}

// MUL of two activations: in1 has in0's shape, or is the 1 x 1 x C gate of its sample.  HBM-bound: 8 bytes moved per
// element with a gate (the gate's C floats per sample come from the cache), 12 with a same-shape in1.
// The 16-byte path: an item is a quad of channels of a pixel, quad fastest, pixels flattened over the batch.
__global__ __launch_bounds__(CT) void graph_mul_quad_kernel(GraphOpArgs a, size_t items, int gate) {
  const size_t idx = (size_t)blockIdx.x * CT + threadIdx.x;
  if (idx >= items) return;
  const int C4 = a.out.C >> 2, hw = a.out.H * a.out.W;
  size_t n;
  int c, pix;
  if ((items >> 32) == 0) {   // 32-bit divisions unless the batch needs more
    const unsigned i = (unsigned)idx, p = i / (unsigned)C4, nn = p / (unsigned)hw;
    c = 4 * (int)(i - p * C4);
    pix = (int)(p - nn * hw);
    n = nn;
  } else {
    const size_t p = idx / C4;
    c = 4 * (int)(idx - p * C4);
    n = p / hw;
    pix = (int)(p - n * hw);
  }
  const f32x4 x = *reinterpret_cast<const f32x4*>(a.in0.p + n * a.in0.sample_stride + (unsigned)(pix * a.in0.cstride + c));
  const f32x4 g = *reinterpret_cast<const f32x4*>(a.in1.p + n * a.in1.sample_stride + (unsigned)(gate ? c : pix * a.in1.cstride + c));
  f32x4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = activate(x[j] * g[j], a.act);
  *reinterpret_cast<f32x4*>(a.out.p + n * a.out.sample_stride + (unsigned)(pix * a.out.cstride + c)) = v;
}

// ... and element by element (an odd C, a concatenation slice off the 16-byte grid)
__global__ __launch_bounds__(CT) void graph_mul_kernel(GraphOpArgs a, int gate) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  const float g = gate ? *at(a.in1, n, 0, 0, c) : *at(a.in1, n, y, x, c);
  *at(a.out, n, y, x, c) = activate(*at(a.in0, n, y, x, c) * g, a.act);
}

// FULLY_CONNECTED: one wave per (sample, output); lanes stride over the inputs, a fixed butterfly sums them
__global__ __launch_bounds__(CT) void graph_fc_kernel(GraphOpArgs a) {
  const int lane = threadIdx.x & 63;
  const size_t wid = (size_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (wid >= (size_t)a.N * a.out.C) return;
  const int o = (int)(wid % a.out.C);
  const size_t n = wid / a.out.C;
  const float* x = a.in0.p + n * a.in0.sample_stride;
  const float* w = a.weights + (size_t)o * a.in0.C;
  float sum = 0.0f;
  for (int k = lane; k < a.in0.C; k += 64) sum += x[k] * w[k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if (lane == 0) a.out.p[n * a.out.sample_stride + o] = activate(sum + (a.shift ? a.shift[o] : 0.0f), a.act);
}

__global__ __launch_bounds__(CT) void graph_logistic_kernel(GraphOpArgs a) {
  size_t n;
  int y, x, c;
  if (!out_coords(a, (size_t)blockIdx.x * CT + threadIdx.x, &n, &y, &x, &c)) return;
  *at(a.out, n, y, x, c) = logistic(*at(a.in0, n, y, x, c));
}

// SOFTMAX over the channels of every pixel: one thread per pixel (the heads this runs have tens of labels)
__global__ __launch_bounds__(CT) void graph_softmax_kernel(GraphOpArgs a) {
  const size_t idx = (size_t)blockIdx.x * CT + threadIdx.x;
  const size_t hw = (size_t)a.in0.H * a.in0.W;
  if (idx >= (size_t)a.N * hw) return;
  const size_t n = idx / hw;
  const unsigned pix = (unsigned)(idx - n * hw);
  const float* src = a.in0.p + n * a.in0.sample_stride + pix * a.in0.cstride;
  float* dst = a.out.p + n * a.out.sample_stride + pix * a.out.cstride;
  float m = -INFINITY;
  for (int c = 0; c < a.in0.C; ++c) m = fmaxf(m, src[c]);
  float sum = 0.0f;
  for (int c = 0; c < a.in0.C; ++c) sum += expf(a.param * (src[c] - m));
  for (int c = 0; c < a.in0.C; ++c) dst[c] = expf(a.param * (src[c] - m)) / sum;
}

}  // namespace

void launch_graph_op(const GraphOpArgs& a, hipStream_t s) {
  const size_t out_elems = (size_t)a.N * a.out.H * a.out.W * a.out.C;
  switch (a.kind) {
    case CPX_GRAPH_CONV:
    case CPX_GRAPH_CONV_PRE:
    case CPX_GRAPH_CONV_GROUPED: {
      typedef void (*Kernel)(GraphOpArgs, ConvGeom);
      // [CONV, CONV_PRE, CONV_GROUPED][an even number of tiles: two per wave]
      static const Kernel kernels[3][2] = {{graph_conv_kernel<1, false>, graph_conv_kernel<2, false>},
                                           {graph_conv_kernel<1, true>, graph_conv_kernel<2, true>},
                                           {graph_conv_kernel<1, false, true>, graph_conv_kernel<2, false, true>}};
      const int which = a.kind == CPX_GRAPH_CONV ? 0 : a.kind == CPX_GRAPH_CONV_PRE ? 1 : 2;
      const ConvGeom g = conv_geom(a.N, a.in0, a.out, GRAPH_CONV_KC, which == 2 ? a.n_map : 1, group_quads<GraphView>);
      const int two = g.ntiles % 2 == 0;   // (the padded output channels are a multiple of 64)
      const dim3 grid((unsigned)((g.P + BM - 1) / BM), g.ntiles / (two ? 2 : 1), g.G);
      hipLaunchKernelGGL(kernels[which][two], grid, dim3(CT), 0, s, a, g);
      break;
    }
    case CPX_GRAPH_MAX_POOL:
      hipLaunchKernelGGL(graph_pool_kernel<true>, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_AVG_POOL:
      hipLaunchKernelGGL(graph_pool_kernel<false>, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_ADD:
      hipLaunchKernelGGL(graph_add_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_AFFINE:
      hipLaunchKernelGGL(graph_affine_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_PAD:
      hipLaunchKernelGGL(graph_pad_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_CHANNEL_MAP:
      hipLaunchKernelGGL(graph_channel_map_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_INPUT:
      hipLaunchKernelGGL(graph_input_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_MEAN:
      if (a.in0.H * a.in0.W < GRAPH_MEAN_WIDE_PIXELS) {
        hipLaunchKernelGGL(graph_mean_kernel, dim3(blocks_for((size_t)a.N * a.in0.C)), dim3(CT), 0, s, a);
      } else {
        const int groups = (a.in0.C + 4 * MEAN_QG - 1) / (4 * MEAN_QG);
        const dim3 grid((unsigned)((size_t)a.N * groups));
        if (quads(a.in0))
          hipLaunchKernelGGL(graph_mean_wide_kernel<true>, grid, dim3(CT), 0, s, a, groups);
        else
          hipLaunchKernelGGL(graph_mean_wide_kernel<false>, grid, dim3(CT), 0, s, a, groups);
      }
      break;
    case CPX_GRAPH_MUL: {
      const int gate = a.in1.H * a.in1.W == 1 && a.in0.H * a.in0.W != 1;
      if (quads(a.in0) && quads(a.in1) && quads(a.out)) {
        const size_t items = out_elems / 4;
        hipLaunchKernelGGL(graph_mul_quad_kernel, dim3(blocks_for(items)), dim3(CT), 0, s, a, items, gate);
      } else {
        hipLaunchKernelGGL(graph_mul_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a, gate);
      }
      break;
    }
    case CPX_GRAPH_FC:
      hipLaunchKernelGGL(graph_fc_kernel, dim3((unsigned)(((size_t)a.N * a.out.C + 3) / 4)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_LOGISTIC:
      hipLaunchKernelGGL(graph_logistic_kernel, dim3(blocks_for(out_elems)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_SOFTMAX:
      hipLaunchKernelGGL(graph_softmax_kernel, dim3(blocks_for((size_t)a.N * a.in0.H * a.in0.W)), dim3(CT), 0, s, a);
      break;
    case CPX_GRAPH_CONV_Q8:
    case CPX_GRAPH_CONV_Q8_GROUPED:
    case CPX_GRAPH_FC_Q8:
    case CPX_GRAPH_QUANT_PARAMS:
      launch_graph_q8_op(a, s);
      break;
    case CPX_GRAPH_SLICE:
      if (a.in0_int8) {
        launch_graph_i8_op(a, s);
        break;
      }
      /* fall through */
    case CPX_GRAPH_DWCONV:
    case CPX_GRAPH_DWCONV_PRE:
    case CPX_GRAPH_DWCONV_Q8:
      launch_graph_dw_op(a, s);
      break;
    case CPX_GRAPH_QUANTIZE:
    case CPX_GRAPH_DEQUANTIZE:
    case CPX_GRAPH_CONV_I8:
    case CPX_GRAPH_CONV_I8_GROUPED:
    case CPX_GRAPH_DWCONV_I8:
    case CPX_GRAPH_FC_I8:
    case CPX_GRAPH_ADD_I8:
    case CPX_GRAPH_MUL_I8:
    case CPX_GRAPH_MAX_POOL_I8:
    case CPX_GRAPH_AVG_POOL_I8:
    case CPX_GRAPH_MEAN_I8:
    case CPX_GRAPH_LUT_I8:
      launch_graph_i8_op(a, s);
      break;
    case CPX_GRAPH_RANGE:
    case CPX_GRAPH_CONV_F16X2:
      launch_graph_h2_op(a, s);
      break;
    default:
      break;
  }
}

}  // namespace cpx
