// cpx_graph_q8.hip -- the hybrid (dynamic-range quantised) operators of the TFLite graph executor: int8 filters, float32
// activations that are quantised to 8 bits per sample where an operator reads them, int32 accumulation on the int8
// matrix pipe.  The arithmetic is fixed in include/cpx.h (CPX_GRAPH_QUANT_PARAMS / CONV_Q8 / FC_Q8) so that a NumPy
// restatement reproduces it bit for bit: every float32 operation is written as one operation in cpx_graph_core.h
// (quantise, quant_params, hybrid_finish; the build has -ffp-contract=off), the integer sums are exact in any order.
//
// CONV_Q8 is an implicit GEMM on v_mfma_i32_32x32x32_i8 over the walk of cpx_graph_conv_core.h (M, N, K, the staging role,
// the step ahead), K in chunks of 32 input channels: one MFMA per step and tile.
// A: two threads per pixel load 16 float32 channels each (4 x 128 bits), quantise them with their pixel's sample's
//    parameters and write 16 bytes with one ds_write_b128 into a [pixel][k] image of 32-byte rows.  Thread t writes bytes
//    [16 t, 16 t + 16) and lane l of wave w reads bytes [1024 w + 32 (l & 31) + 16 (l >> 5), + 16): both sides touch one
//    contiguous span per wave, so the 32-byte row needs no padding to stay clear of bank conflicts.  The image is double
//    buffered: one barrier per step.  No int8 copy of the activation goes to memory.
// B: the host packs the filter in fragment order ([tap][chunk][tile][lane][16 bytes], GRAPH_CONV_Q8_KC), so a lane takes
//    its fragment from global memory with one 128-bit load, a step ahead; the four waves share it through the cache.
// Lane map (checked with exact integers by tests/test_tflite_q8_gpu.py::test_operand_map_exact): lane l holds row / column
// l & 31 and sixteen consecutive k of half l >> 5 of A and of B; C / D is the map of the other 32 x 32 forms.
#include <hip/hip_runtime.h>

#include "cpx_graph_conv_core.h"
#include "cpx_graph_minmax.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

constexpr int KQ = GRAPH_CONV_Q8_KC;  // input channels (bytes of a row of the A image) per step

// QUANT_PARAMS: one workgroup per sample; out = [sx, inv, zp, 0].  The reduction is sample_min_max (cpx_graph_minmax.h),
// which RANGE shares.
constexpr int QT = GRAPH_MINMAX_THREADS;

template <int VW>
__global__ __launch_bounds__(QT) void graph_quant_params_kernel(GraphOpArgs a) {
  const size_t n = blockIdx.x;
  float lo, hi;
  sample_min_max<VW>(a.in0, n, &lo, &hi);
  if (threadIdx.x != 0) return;
  const QuantParams q8 = quant_params(lo, hi, a.param != 0.0f);
  float* out = a.out.p + n * a.out.sample_stride;
  out[0] = q8.sx;
  out[1] = q8.inv;
  out[2] = (float)q8.zp;
  out[3] = 0.0f;
}

// GRP (CONV_Q8_GROUPED): blockIdx.z is the group.  The parameters are the whole view's (in1), the walk is CONV_Q8's over
// the group's own Cg channels with the group's own fragment image; wsum, scale and shift are indexed by the absolute
// channel (wsum by the padded one: [G][Cog rounded up to 32], behind all G images), the store is bounded by the group.
template <int NTN, bool GRP = false>
__global__ __launch_bounds__(CT) void graph_conv_q8_kernel(GraphOpArgs a, ConvGeom g) {
  __shared__ __attribute__((aligned(16))) int s_a[2][BM * KQ / 4];   // [pixel][k], bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * BM;
  const int tile0 = blockIdx.y * NTN;
  const int grp = GRP ? (int)blockIdx.z : 0;
  const int Cin = GRP ? g.cg : a.in0.C;   // the channels of the K walk
  const int Cout = GRP ? g.cog : a.out.C;

  // the stager's 16 channels of every chunk; its sample's parameters are worked out once
  const ConvStager<float> st = conv_stager(a, g, a.in0.p, p0, tid, GRP ? grp * g.cg : 0);
  const float* in_n = st.in_n;
  const float* sprm = a.in1.p + (size_t)st.px.n * a.in1.sample_stride;
  const float inv = sprm[1];
  const int zp = (int)sprm[2];
  const int steps = a.kh * a.kw * g.nchunks;
  const i32x4* wq0 = reinterpret_cast<const i32x4*>(a.weights);
  const i32x4* wq = GRP ? wq0 + (size_t)grp * steps * g.ntiles * 64 : wq0;   // the group's image

  i32x16 acc[NTN];
#pragma unroll
  for (int t = 0; t < NTN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0;

  f32x4 pre[4];
  i32x4 bnext[NTN];

  // global -> registers of step s.  A masked element (outside the image or the tile, beyond Cin) is a real 0, which
  // quantises to zp: what TFLite's padding contributes; beyond Cin the weights are zero and any value would do
  auto fetch = [&](int s) {
    const ConvPatch f = conv_patch(a, st, s, g.nchunks, KQ);
    const bool inside = f.inside;
    const int c = f.c, pix = f.pix;
    if (g.vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = inside && (c + 4 * q) < Cin;   // Cin % 4 == 0: a quad is valid as a whole
        const f32x4 v = *reinterpret_cast<const f32x4*>(in_n + (ok ? pix + c + 4 * q : 0));
        pre[q].x = ok ? v.x : 0.0f;
        pre[q].y = ok ? v.y : 0.0f;
        pre[q].z = ok ? v.z : 0.0f;
        pre[q].w = ok ? v.w : 0.0f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const bool ok = inside && (c + j) < Cin;
        const float v = in_n[ok ? pix + c + j : 0];
        pre[j >> 2][j & 3] = ok ? v : 0.0f;
      }
    }
    prefetch_fragments<NTN>(wq, s, g.ntiles, tile0, 64, lane, bnext);
  };

  fetch(0);
  for (int s = 0; s < steps; ++s) {
    int* buf = s_a[s & 1];
    i32x4 packed;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      packed[q] = pack4(quantise(pre[q].x, inv, zp), quantise(pre[q].y, inv, zp), quantise(pre[q].z, inv, zp),
                        quantise(pre[q].w, inv, zp));
    *reinterpret_cast<i32x4*>(buf + 4 * tid) = packed;
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

  // epilogue: accumulator register r of a lane is pixel acc_row(r, tid) of the wave's 32, channel lane & 31 of the
  // tile; every pixel takes its own sample's sx and zp
  const long long pb = p0 + 32 * wave;
  if (pb >= g.P) return;
  const int* wsum = reinterpret_cast<const int*>(wq0 + (size_t)(GRP ? g.G : 1) * steps * g.ntiles * 64) + (GRP ? grp * g.ntiles * 32 : 0);
  const long long nb = pb / g.HoWo;
  const int remb = (int)(pb - nb * g.HoWo);
#pragma unroll
  for (int t = 0; t < NTN; ++t) {
    const int chl = (tile0 + t) * 32 + (lane & 31);   // within the group: the bound is the group's own
    if (tile0 + t >= g.ntiles || chl >= Cout) continue;
    const int ch = (GRP ? grp * g.cog : 0) + chl;
    const float sc = a.scale[ch];
    const float sh = a.shift[ch];
    const int ws = wsum[chl];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(r, tid);
      if (pb + i >= g.P) continue;
      const SamplePixel o = sample_step(nb, remb + i, g.HoWo);
      const float* prm = a.in1.p + (size_t)o.n * a.in1.sample_stride;
      a.out.p[(size_t)o.n * a.out.sample_stride + (unsigned)(o.rem * a.out.cstride + ch)] =
          hybrid_finish(acc[t][r], (int)prm[2], ws, prm[0], sc, sh, a.act);
    }
  }
}

// FC_Q8: one wave per (sample, output).  Weights [Cout][Cin rounded up to 4] int8 (zeros beyond), wsum[Cout] int32 behind.
// A lane quantises four inputs at a time and sums them against four weights with v_dot4_i32_i8; an integer butterfly follows.
__global__ __launch_bounds__(CT) void graph_fc_q8_kernel(GraphOpArgs a) {
  const int lane = threadIdx.x & 63;
  const size_t wid = (size_t)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
  if (wid >= (size_t)a.N * a.out.C) return;
  const int o = (int)(wid % a.out.C);
  const size_t n = wid / a.out.C;
  const int C = a.in0.C, groups = (C + 3) / 4;
  const float* x = a.in0.p + n * a.in0.sample_stride;
  const float* prm = a.in1.p + n * a.in1.sample_stride;
  const float sx = prm[0], inv = prm[1];
  const int zp = (int)prm[2];
  const int* w = reinterpret_cast<const int*>(a.weights) + (size_t)o * groups;
  const int* wsum = reinterpret_cast<const int*>(a.weights) + (size_t)a.out.C * groups;
  int acc = 0;
  for (int gidx = lane; gidx < groups; gidx += 64) {
    int q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * gidx + j;
      q[j] = quantise(k < C ? x[k] : 0.0f, inv, zp);   // (beyond Cin the weights are zero)
    }
    acc = __builtin_amdgcn_sdot4(pack4(q[0], q[1], q[2], q[3]), w[gidx], acc, false);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) a.out.p[n * a.out.sample_stride + o] = hybrid_finish(acc, zp, wsum[o], sx, a.scale[o], a.shift[o], a.act);
}

}  // namespace

void launch_graph_q8_op(const GraphOpArgs& a, hipStream_t s) {
  const int vec4 = quads(a.in0);
  switch (a.kind) {
    case CPX_GRAPH_QUANT_PARAMS:
      if (vec4)
        hipLaunchKernelGGL(graph_quant_params_kernel<4>, dim3((unsigned)a.N), dim3(QT), 0, s, a);
      else
        hipLaunchKernelGGL(graph_quant_params_kernel<1>, dim3((unsigned)a.N), dim3(QT), 0, s, a);
      break;
    case CPX_GRAPH_CONV_Q8:
    case CPX_GRAPH_CONV_Q8_GROUPED: {
      const bool grouped = a.kind == CPX_GRAPH_CONV_Q8_GROUPED;
      const ConvGeom g = conv_geom(a.N, a.in0, a.out, KQ, grouped ? a.n_map : 1, group_quads<GraphView>);
      const unsigned gx = (unsigned)((g.P + BM - 1) / BM);
      conv_dispatch_ntn(g.ntiles, [&](auto ntn, int rows) {
        constexpr int NTN = decltype(ntn)::value;
        if (grouped)
          hipLaunchKernelGGL((graph_conv_q8_kernel<NTN, true>), dim3(gx, rows, g.G), dim3(CT), 0, s, a, g);
        else
          hipLaunchKernelGGL((graph_conv_q8_kernel<NTN, false>), dim3(gx, rows), dim3(CT), 0, s, a, g);
      });
      break;
    }
    case CPX_GRAPH_FC_Q8:
      hipLaunchKernelGGL(graph_fc_q8_kernel, dim3((unsigned)(((size_t)a.N * a.out.C + 3) / 4)), dim3(CT), 0, s, a);
      break;
    default:
      break;
  }
}

}  // namespace cpx
