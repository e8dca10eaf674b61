// cpx_graph_i8.hip -- the full-integer operators of the TFLite graph executor: int8 activations between a QUANTIZE and a
// DEQUANTIZE, int8 filters, int32 biases.  The arithmetic is fixed in include/cpx.h ("The full-integer arithmetic") and
// written once in cpx_graph_i8_core.h; every step is integer, so a NumPy restatement reproduces a whole network bit for
// bit.  No int8 tensor is ever expanded to float32 in memory.
//
// An int8 view is a GraphView whose `p` points at BYTES (the entry point adds the channel offset in bytes) and whose
// sample_stride counts bytes.  Every kernel has two instantiations: VW = 16 moves sixteen channels of a pixel per lane with
// one 16-byte load / store where the views allow (bytes16 / floats16: channels, row stride, sample stride and pointer all
// multiples of 16 elements), VW = 1 goes element by element.  Both run the same arithmetic on the same integers.
//
// CONV_I8 is graph_conv_q8_kernel's implicit GEMM on v_mfma_i32_32x32x32_i8 (cpx_graph_q8.hip; the walk: cpx_graph_conv_core.h;
// the filter fragment image and its wsum unchanged) with the A
// image staged FROM BYTES -- a thread takes its pixel's 16 channels with one 16-byte load, or byte by byte; a masked
// element is z_in, nothing is quantised -- and an epilogue that requantises in registers and stores bytes.
//
// A unary int8 -> int8 function (an interior LOGISTIC, a swish) is a 256-entry table behind the header (include/cpx.h,
// "Tables"): LUT_I8 looks every byte up, and CONV_I8 / CONV_I8_GROUPED / DWCONV_I8 with CPX_GRAPH_ACT_LUT send their
// requantised byte through it (the LUT template parameter).  The table sits in 256 bytes of LDS.
#include <hip/hip_runtime.h>

#include "cpx_graph_conv_core.h"
#include "cpx_graph_i8_core.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

constexpr int KQ = GRAPH_CONV_Q8_KC;  // input channels (bytes of a row of the A image) per step

__device__ __forceinline__ int byte_of(int word, int j) { return (int)(word << (24 - 8 * j)) >> 24; }   // sign extended

__device__ __forceinline__ const int8_t* bytes_of(const GraphView& v) { return reinterpret_cast<const int8_t*>(v.p); }
__device__ __forceinline__ int8_t* bytes_of_out(const GraphView& v) { return reinterpret_cast<int8_t*>(v.p); }
__device__ __forceinline__ const I8Header& header_of(const GraphOpArgs& a) { return *reinterpret_cast<const I8Header*>(a.shift); }

template <int VW>
__device__ __forceinline__ void load_q(const int8_t* p, int (&q)[VW]) {
  if constexpr (VW == 16) {
    const i32x4 v = *reinterpret_cast<const i32x4*>(p);
#pragma unroll
    for (int j = 0; j < 16; ++j) q[j] = byte_of(v[j >> 2], j & 3);
  } else {
    q[0] = p[0];
  }
}
template <int VW>
__device__ __forceinline__ void store_q(int8_t* p, const int (&q)[VW]) {
  if constexpr (VW == 16) {
    i32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = pack4(q[4 * k], q[4 * k + 1], q[4 * k + 2], q[4 * k + 3]);
    *reinterpret_cast<i32x4*>(p) = v;
  } else {
    p[0] = (int8_t)q[0];
  }
}
template <int VW>
__device__ __forceinline__ void load_f(const float* p, float (&x)[VW]) {
  if constexpr (VW == 16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x4 v = reinterpret_cast<const f32x4*>(p)[k];
      x[4 * k] = v.x, x[4 * k + 1] = v.y, x[4 * k + 2] = v.z, x[4 * k + 3] = v.w;
    }
  } else {
    x[0] = p[0];
  }
}
template <int VW>
__device__ __forceinline__ void store_f(float* p, const float (&x)[VW]) {
  if constexpr (VW == 16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x4 v;
      v.x = x[4 * k], v.y = x[4 * k + 1], v.z = x[4 * k + 2], v.w = x[4 * k + 3];
      reinterpret_cast<f32x4*>(p)[k] = v;
    }
  } else {
    p[0] = x[0];
  }
}

// work item i of N * H * W * (C / VW), channel group fastest -> sample, pixel of the sample, first channel
struct PixelItem {
  size_t n;
  int rem, c;
};
template <int VW>
__device__ __forceinline__ PixelItem pixel_item(size_t i, int C, int HW) {
  const int groups = C / VW;
  const size_t pix = i / groups;
  PixelItem it;
  it.c = (int)(i - pix * groups) * VW;
  it.n = pix / HW;
  it.rem = (int)(pix - it.n * HW);
  return it;
}
__device__ __forceinline__ size_t at(const GraphView& v, size_t n, int rem, int c) {
  return n * v.sample_stride + (size_t)rem * v.cstride + c;
}

// ---- the element-wise operators: the two QUANTIZE forms, DEQUANTIZE, ADD_I8, MUL_I8 (in1 of one shape, the constant, or
// MUL_I8's per-sample gate) ----
enum { EW_QUANT = 0, EW_REQUANT = 1, EW_DEQUANT = 2, EW_ADD = 3, EW_MUL = 4 };

template <int VW, int OP>
__global__ __launch_bounds__(CT) void graph_i8_ew_kernel(GraphOpArgs a, size_t items) {
  const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;
  if (i >= items) return;
  const I8Header& h = header_of(a);
  const PixelItem it = pixel_item<VW>(i, a.out.C, a.out.H * a.out.W);
  int q[VW];
  if constexpr (OP == EW_QUANT) {
    float x[VW];
    load_f<VW>(a.in0.p + at(a.in0, it.n, it.rem, it.c), x);
    const int z = h.v[CPX_GRAPH_I8_HDR_Z_OUT];
#pragma unroll
    for (int j = 0; j < VW; ++j) q[j] = quantize_f32(x[j], a.param, z);
    store_q<VW>(bytes_of_out(a.out) + at(a.out, it.n, it.rem, it.c), q);
  } else if constexpr (OP == EW_DEQUANT) {
    load_q<VW>(bytes_of(a.in0) + at(a.in0, it.n, it.rem, it.c), q);
    float x[VW];
    const int z = h.v[CPX_GRAPH_I8_HDR_Z_IN];
#pragma unroll
    for (int j = 0; j < VW; ++j) x[j] = dequantize_i8(q[j], a.param, z);
    store_f<VW>(a.out.p + at(a.out, it.n, it.rem, it.c), x);
  } else {
    load_q<VW>(bytes_of(a.in0) + at(a.in0, it.n, it.rem, it.c), q);
    if constexpr (OP == EW_REQUANT) {
#pragma unroll
      for (int j = 0; j < VW; ++j) q[j] = requantize_i8(q[j], h);
    } else {
      int b[VW];
      if (a.in1.p)   // (MUL_I8's 1 x 1 x C gate: pixel 0 of its sample, whatever the output's pixel)
        load_q<VW>(bytes_of(a.in1) + at(a.in1, it.n, OP == EW_MUL && a.in1.H * a.in1.W == 1 ? 0 : it.rem, it.c), b);
      else
        load_q<VW>(reinterpret_cast<const int8_t*>(a.weights) + it.c, b);   // the constant, per channel
      const int sign = a.param < 0.0f ? -1 : 1;
#pragma unroll
      for (int j = 0; j < VW; ++j) q[j] = OP == EW_ADD ? add_i8(q[j], b[j], sign, h) : mul_i8(q[j], b[j], h);
    }
    store_q<VW>(bytes_of_out(a.out) + at(a.out, it.n, it.rem, it.c), q);
  }
}

// ---- the 256-entry table of LUT_I8 and of CPX_GRAPH_ACT_LUT: one byte per thread into LDS (CT == 256); the caller's next
// barrier publishes it
static_assert(CT == 256, "a workgroup stages the table one entry per thread");
__device__ __forceinline__ void stage_table(int8_t (&s_t)[256], const GraphOpArgs& a) {
  s_t[threadIdx.x] = table_of(&header_of(a))[threadIdx.x];
}

// LUT_I8: the element-wise kernel's walk with sixteen lookups per lane between one 16-byte load and one 16-byte store.
// A lookup is one LDS byte read: 16 of them per 32 bytes of HBM traffic, from a table of 64 dwords -- two dwords per
// bank, so a read is at worst a two-way conflict (DESIGN.md section 5 has the arithmetic)
template <int VW>
__global__ __launch_bounds__(CT) void graph_i8_lut_kernel(GraphOpArgs a, size_t items) {
  __shared__ int8_t s_t[256];
  stage_table(s_t, a);
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;
  if (i >= items) return;
  const PixelItem it = pixel_item<VW>(i, a.out.C, a.out.H * a.out.W);
  int q[VW];
  load_q<VW>(bytes_of(a.in0) + at(a.in0, it.n, it.rem, it.c), q);
#pragma unroll
  for (int j = 0; j < VW; ++j) q[j] = lut_i8(s_t, q[j]);
  store_q<VW>(bytes_of_out(a.out) + at(a.out, it.n, it.rem, it.c), q);
}

// ---- the window operators: DWCONV_I8, MAX_POOL_I8, AVG_POOL_I8 and SLICE on bytes ----
enum { WIN_DW = 0, WIN_MAX = 1, WIN_AVG = 2, WIN_SLICE = 3 };

// One output pixel and VW channels per lane.  Every read is masked by the input's size (SLICE's pads are signed).
// DWCONV_I8 sums (q - z_in) * w over the in-bounds taps: a padded tap contributes nothing and no wsum is needed.
// LUT (DWCONV_I8 with CPX_GRAPH_ACT_LUT): the finished byte goes through the table, staged before any thread leaves.
template <int VW, int OP, bool LUT = false>
__global__ __launch_bounds__(CT) void graph_i8_window_kernel(GraphOpArgs a, size_t items) {
  __shared__ int8_t s_t[LUT ? 256 : 1];
  if constexpr (LUT) {
    stage_table(s_t, a);
    __syncthreads();
  }
  const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;
  if (i >= items) return;
  const I8Header& h = header_of(a);
  const int C = a.out.C, H = a.in0.H, W = a.in0.W;
  const PixelItem it = pixel_item<VW>(i, C, a.out.H * a.out.W);
  const int oy = it.rem / a.out.W, ox = it.rem - oy * a.out.W;
  const int iy0 = window_origin(oy, a.stride_h, a.pad_top), ix0 = window_origin(ox, a.stride_w, a.pad_left);
  const int8_t* in_n = bytes_of(a.in0) + it.n * a.in0.sample_stride + it.c;
  const int z_in = h.v[CPX_GRAPH_I8_HDR_Z_IN];
  const int cp = (C + 3) / 4 * 4;   // DWCONV_I8: the filter's row of channels
  int acc[VW], count = 0;
#pragma unroll
  for (int j = 0; j < VW; ++j) acc[j] = OP == WIN_MAX ? -128 : OP == WIN_SLICE ? z_in : 0;
  for (int ky = 0; ky < a.kh; ++ky) {
    const int iy = iy0 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < a.kw; ++kx) {
      const int ix = ix0 + kx;
      if (ix < 0 || ix >= W) continue;
      int q[VW];
      load_q<VW>(in_n + (size_t)(iy * W + ix) * a.in0.cstride, q);
      ++count;
      if constexpr (OP == WIN_DW) {
        int w[VW];
        load_q<VW>(reinterpret_cast<const int8_t*>(a.weights) + (size_t)(ky * a.kw + kx) * cp + it.c, w);
#pragma unroll
        for (int j = 0; j < VW; ++j) acc[j] += (q[j] - z_in) * w[j];
      } else {
#pragma unroll
        for (int j = 0; j < VW; ++j) acc[j] = OP == WIN_MAX ? max(acc[j], q[j]) : OP == WIN_AVG ? acc[j] + q[j] : q[j];
      }
    }
  }
  const int lo = h.v[CPX_GRAPH_I8_HDR_LO], hi = h.v[CPX_GRAPH_I8_HDR_HI];
  const int* prm = reinterpret_cast<const int*>(a.scale);   // DWCONV_I8: M[C], shift[C], bias[C]
#pragma unroll
  for (int j = 0; j < VW; ++j) {
    if constexpr (OP == WIN_DW) {
      // (wsum 0: the zero point is already out of the sum)
      acc[j] = filter_finish_i8(acc[j], 0, prm[2 * C + it.c + j], prm[it.c + j], prm[C + it.c + j], h);
      if constexpr (LUT) acc[j] = lut_i8(s_t, acc[j]);
    } else if constexpr (OP == WIN_MAX) {
      acc[j] = clamp_i8(acc[j], lo, hi);
    } else if constexpr (OP == WIN_AVG) {
      acc[j] = clamp_i8(round_div(acc[j], count > 0 ? count : 1), lo, hi);
    }
  }
  store_q<VW>(bytes_of_out(a.out) + at(a.out, it.n, it.rem, it.c), acc);
}

// ---- MEAN_I8: one wave per (sample, VW channels); the lanes split the pixels, an integer butterfly follows (the sum is
// exact in any order)
template <int VW>
__global__ __launch_bounds__(CT) void graph_i8_mean_kernel(GraphOpArgs a, size_t items) {
  const int lane = threadIdx.x & 63;
  const size_t wid = (size_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (wid >= items) return;
  const int groups = a.in0.C / VW, HW = a.in0.H * a.in0.W;
  const size_t n = wid / groups;
  const int c = (int)(wid - n * groups) * VW;
  const int8_t* in_n = bytes_of(a.in0) + n * a.in0.sample_stride + c;
  int sum[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) sum[j] = 0;
  for (int p = lane; p < HW; p += 64) {
    int q[VW];
    load_q<VW>(in_n + (size_t)p * a.in0.cstride, q);
#pragma unroll
    for (int j = 0; j < VW; ++j) sum[j] += q[j];
  }
#pragma unroll
  for (int j = 0; j < VW; ++j)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum[j] += __shfl_xor(sum[j], d, 64);
  if (lane != 0) return;
  const I8Header& h = header_of(a);
#pragma unroll
  for (int j = 0; j < VW; ++j) sum[j] = mean_i8(sum[j], HW, h);
  store_q<VW>(bytes_of_out(a.out) + n * a.out.sample_stride + c, sum);
}

// ---- FC_I8: one wave per (sample, output), FC_Q8 minus the quantisation.  Weights [Cout][Cin rounded up to 4] int8 (zeros
// beyond), wsum[Cout] behind.  WORDS: the input row is read as aligned 32-bit words (a word beyond Cin meets zero weights
// only where it lies inside the row: the last, partial word is put together from bytes)
template <bool WORDS>
__global__ __launch_bounds__(CT) void graph_fc_i8_kernel(GraphOpArgs a) {
  const int lane = threadIdx.x & 63;
  const size_t wid = (size_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (wid >= (size_t)a.N * a.out.C) return;
  const int o = (int)(wid % a.out.C);
  const size_t n = wid / a.out.C;
  const int C = a.in0.C, groups = (C + 3) / 4;
  const int8_t* x = bytes_of(a.in0) + n * a.in0.sample_stride;
  const int* w = reinterpret_cast<const int*>(a.weights) + (size_t)o * groups;
  const int* wsum = reinterpret_cast<const int*>(a.weights) + (size_t)a.out.C * groups;
  int acc = 0;
  for (int gidx = lane; gidx < groups; gidx += 64) {
    int word;
    if (WORDS && 4 * gidx + 4 <= C) {
      word = reinterpret_cast<const int*>(x)[gidx];
    } else {
      int q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * gidx + j;
        q[j] = k < C ? x[k] : 0;   // (beyond Cin the weights are zero)
      }
      word = pack4(q[0], q[1], q[2], q[3]);
    }
    acc = __builtin_amdgcn_sdot4(word, w[gidx], acc, false);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane != 0) return;
  const int* prm = reinterpret_cast<const int*>(a.scale);
  const int Co = a.out.C;
  bytes_of_out(a.out)[n * a.out.sample_stride + o] =
      (int8_t)filter_finish_i8(acc, wsum[o], prm[2 * Co + o], prm[o], prm[Co + o], header_of(a));
}

// ---- CONV_I8 / CONV_I8_GROUPED ----
// V16: the view's channel count per group, channel offsets, row stride and sample stride are multiples of 16 and its
// pointer is 16-byte aligned -- a thread's 16 channels are one aligned 16-byte load and valid or masked as a whole.
// LUT (CPX_GRAPH_ACT_LUT): the table is staged in front of the K walk -- the walk's first barrier publishes it -- and read
// in the epilogue behind filter_finish_i8.
template <int NTN, bool GRP, bool V16, bool LUT>
__global__ __launch_bounds__(CT) void graph_conv_i8_kernel(GraphOpArgs a, ConvGeom g) {
  __shared__ __attribute__((aligned(16))) int s_a[2][BM * KQ / 4];   // [pixel][k], bytes
  __shared__ int8_t s_t[LUT ? 256 : 1];
  if constexpr (LUT) stage_table(s_t, a);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * BM;
  const int tile0 = blockIdx.y * NTN;
  const int grp = GRP ? (int)blockIdx.z : 0;
  const int Cin = g.cg;   // the channels of the K walk
  const int Cout = g.cog;
  const I8Header& h = header_of(a);
  const int z_in = h.v[CPX_GRAPH_I8_HDR_Z_IN];
  const int zword = pack4(z_in, z_in, z_in, z_in);

  const ConvStager<int8_t> st = conv_stager(a, g, bytes_of(a.in0), p0, tid, grp * g.cg);
  const int8_t* in_n = st.in_n;
  const int steps = a.kh * a.kw * g.nchunks;
  const i32x4* wq0 = reinterpret_cast<const i32x4*>(a.weights);
  const i32x4* wq = wq0 + (size_t)grp * steps * g.ntiles * 64;   // the group's image

  i32x16 acc[NTN];
#pragma unroll
  for (int t = 0; t < NTN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0;

  i32x4 pre;
  i32x4 bnext[NTN];

  // global -> registers of step s.  A masked element (outside the image or the tile, beyond Cin) is z_in: a real 0, what
  // TFLite's padding contributes (acc - z_in * wsum takes it out again); beyond Cin the weights are zero
  auto fetch = [&](int s) {
    const ConvPatch f = conv_patch(a, st, s, g.nchunks, KQ);
    const bool inside = f.inside;
    const int c = f.c;
    const size_t pix = f.pix;
    if (V16) {
      const bool ok = inside && c < Cin;   // Cin % 16 == 0: the sixteen are valid as a whole
      const i32x4 v = *reinterpret_cast<const i32x4*>(in_n + (ok ? pix + c : 0));
#pragma unroll
      for (int k = 0; k < 4; ++k) pre[k] = ok ? v[k] : zword;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool ok = inside && (c + 4 * k + j) < Cin;
          const int v = in_n[ok ? pix + c + 4 * k + j : 0];
          q[j] = ok ? v : z_in;
        }
        pre[k] = pack4(q[0], q[1], q[2], q[3]);
      }
    }
    prefetch_fragments<NTN>(wq, s, g.ntiles, tile0, 64, lane, bnext);
  };

  fetch(0);
  for (int s = 0; s < steps; ++s) {
    int* buf = s_a[s & 1];
    *reinterpret_cast<i32x4*>(buf + 4 * tid) = pre;
    i32x4 bcur[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t) bcur[t] = bnext[t];
    __syncthreads();   // (the other buffer is free: every wave read it before it reached this barrier)
    if (s + 1 < steps) fetch(s + 1);   // in flight while the matrix cores work on step s
    const i32x4 af = *reinterpret_cast<const i32x4*>(buf + (32 * wave + (lane & 31)) * (KQ / 4) + 4 * (lane >> 5));
#pragma unroll
    for (int t = 0; t < NTN; ++t)
      if (tile0 + t < g.ntiles) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bcur[t], acc[t], 0, 0, 0);
  }

  // epilogue: accumulator register r of a lane is pixel acc_row(r, tid) of the wave's 32, channel lane & 31 of the tile
  const long long pb = p0 + 32 * wave;
  if (pb >= g.P) return;
  const int* wsum = reinterpret_cast<const int*>(wq0 + (size_t)g.G * steps * g.ntiles * 64) + grp * g.ntiles * 32;
  const int* prm = reinterpret_cast<const int*>(a.scale);   // M, shift, bias: [3][out C], by the absolute channel
  const int Ctot = a.out.C;
  int8_t* out = bytes_of_out(a.out);
  const long long nb = pb / g.HoWo;
  const int remb = (int)(pb - nb * g.HoWo);
#pragma unroll
  for (int t = 0; t < NTN; ++t) {
    const int chl = (tile0 + t) * 32 + (lane & 31);   // within the group: the bound is the group's own
    if (tile0 + t >= g.ntiles || chl >= Cout) continue;
    const int ch = grp * g.cog + chl;
    const int M = prm[ch], sh = prm[Ctot + ch], bias = prm[2 * Ctot + ch];
    const int ws = wsum[chl];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(r, tid);
      if (pb + i >= g.P) continue;
      const SamplePixel o = sample_step(nb, remb + i, g.HoWo);
      int v = filter_finish_i8(acc[t][r], ws, bias, M, sh, h);
      if constexpr (LUT) v = lut_i8(s_t, v);
      out[(size_t)o.n * a.out.sample_stride + (size_t)o.rem * a.out.cstride + ch] = (int8_t)v;
    }
  }
}

// the view can be read and written sixteen channels at a time with aligned 16-byte accesses
bool bytes16(const GraphView& v) {
  return v.C % 16 == 0 && v.cstride % 16 == 0 && v.sample_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0;
}
bool floats16(const GraphView& v) { return quads(v) && v.C % 16 == 0; }

template <int OP>
void launch_ew(const GraphOpArgs& a, bool wide, hipStream_t s) {
  const size_t elems = (size_t)a.N * a.out.H * a.out.W * a.out.C;
  if (wide)
    hipLaunchKernelGGL((graph_i8_ew_kernel<16, OP>), dim3(blocks_for(elems / 16)), dim3(CT), 0, s, a, elems / 16);
  else
    hipLaunchKernelGGL((graph_i8_ew_kernel<1, OP>), dim3(blocks_for(elems)), dim3(CT), 0, s, a, elems);
}

template <int OP, bool LUT = false>
void launch_window(const GraphOpArgs& a, hipStream_t s) {
  const size_t elems = (size_t)a.N * a.out.H * a.out.W * a.out.C;
  const bool wide = bytes16(a.in0) && bytes16(a.out) && (OP != WIN_DW || (reinterpret_cast<uintptr_t>(a.weights) & 15) == 0);
  if (wide)
    hipLaunchKernelGGL((graph_i8_window_kernel<16, OP, LUT>), dim3(blocks_for(elems / 16)), dim3(CT), 0, s, a, elems / 16);
  else
    hipLaunchKernelGGL((graph_i8_window_kernel<1, OP, LUT>), dim3(blocks_for(elems)), dim3(CT), 0, s, a, elems);
}

template <bool GRP, bool LUT>
void launch_conv(const GraphOpArgs& a, hipStream_t s) {
  const ConvGeom g = conv_geom(a.N, a.in0, a.out, KQ, GRP ? a.n_map : 1, group_bytes16<GraphView>);
  const unsigned gx = (unsigned)((g.P + BM - 1) / BM);
  conv_dispatch_ntn(g.ntiles, [&](auto ntn, int rows) {
    constexpr int NTN = decltype(ntn)::value;
    if (g.vec)
      hipLaunchKernelGGL((graph_conv_i8_kernel<NTN, GRP, true, LUT>), dim3(gx, rows, g.G), dim3(CT), 0, s, a, g);
    else
      hipLaunchKernelGGL((graph_conv_i8_kernel<NTN, GRP, false, LUT>), dim3(gx, rows, g.G), dim3(CT), 0, s, a, g);
  });
}

}  // namespace

void launch_graph_i8_op(const GraphOpArgs& a, hipStream_t s) {
  switch (a.kind) {
    case CPX_GRAPH_QUANTIZE:
      if (a.in0_int8)
        launch_ew<EW_REQUANT>(a, bytes16(a.in0) && bytes16(a.out), s);
      else
        launch_ew<EW_QUANT>(a, floats16(a.in0) && bytes16(a.out), s);
      break;
    case CPX_GRAPH_DEQUANTIZE:
      launch_ew<EW_DEQUANT>(a, bytes16(a.in0) && floats16(a.out), s);
      break;
    case CPX_GRAPH_ADD_I8:
    case CPX_GRAPH_MUL_I8: {
      const bool wide = bytes16(a.in0) && bytes16(a.out) &&
                        (a.in1.p ? bytes16(a.in1) : (reinterpret_cast<uintptr_t>(a.weights) & 15) == 0);
      if (a.kind == CPX_GRAPH_ADD_I8)
        launch_ew<EW_ADD>(a, wide, s);
      else
        launch_ew<EW_MUL>(a, wide, s);
      break;
    }
    case CPX_GRAPH_DWCONV_I8:
      if (a.act == CPX_GRAPH_ACT_LUT)
        launch_window<WIN_DW, true>(a, s);
      else
        launch_window<WIN_DW>(a, s);
      break;
    case CPX_GRAPH_LUT_I8: {
      const size_t elems = (size_t)a.N * a.out.H * a.out.W * a.out.C;
      if (bytes16(a.in0) && bytes16(a.out))
        hipLaunchKernelGGL(graph_i8_lut_kernel<16>, dim3(blocks_for(elems / 16)), dim3(CT), 0, s, a, elems / 16);
      else
        hipLaunchKernelGGL(graph_i8_lut_kernel<1>, dim3(blocks_for(elems)), dim3(CT), 0, s, a, elems);
      break;
    }
    case CPX_GRAPH_MAX_POOL_I8:
      launch_window<WIN_MAX>(a, s);
      break;
    case CPX_GRAPH_AVG_POOL_I8:
      launch_window<WIN_AVG>(a, s);
      break;
    case CPX_GRAPH_SLICE:
      launch_window<WIN_SLICE>(a, s);
      break;
    case CPX_GRAPH_MEAN_I8: {
      const bool wide = bytes16(a.in0) && bytes16(a.out);
      const size_t items = (size_t)a.N * (a.in0.C / (wide ? 16 : 1));
      if (wide)
        hipLaunchKernelGGL(graph_i8_mean_kernel<16>, dim3((unsigned)((items + 3) / 4)), dim3(CT), 0, s, a, items);
      else
        hipLaunchKernelGGL(graph_i8_mean_kernel<1>, dim3((unsigned)((items + 3) / 4)), dim3(CT), 0, s, a, items);
      break;
    }
    case CPX_GRAPH_FC_I8: {
      const dim3 grid((unsigned)(((size_t)a.N * a.out.C + 3) / 4));
      if (a.in0.sample_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(a.in0.p) & 3) == 0)
        hipLaunchKernelGGL(graph_fc_i8_kernel<true>, grid, dim3(CT), 0, s, a);
      else
        hipLaunchKernelGGL(graph_fc_i8_kernel<false>, grid, dim3(CT), 0, s, a);
      break;
    }
    case CPX_GRAPH_CONV_I8:
      if (a.act == CPX_GRAPH_ACT_LUT)
        launch_conv<false, true>(a, s);
      else
        launch_conv<false, false>(a, s);
      break;
    case CPX_GRAPH_CONV_I8_GROUPED:
      if (a.act == CPX_GRAPH_ACT_LUT)
        launch_conv<true, true>(a, s);
      else
        launch_conv<true, false>(a, s);
      break;
    default:
      break;
  }
}

}  // namespace cpx
