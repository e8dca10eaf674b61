// cpx_graph_h2.hip -- the fp16x2 convolution of the TFLite graph executor: CONV_2D with float32 in and float32 out, every
// operand as two fp16 planes (11 + 11 significand bits), three plane products per K block on the fp16 matrix pipe with
// float32 accumulation, and RANGE, which measures the per-sample power of two that keeps the planes inside fp16.  The
// arithmetic is fixed in include/cpx.h (CPX_GRAPH_RANGE / CONV_F16X2) so that a NumPy restatement can follow it
// (tests/tflite_eval_h2.py); the build has -ffp-contract=off.
//
// CONV_F16X2 is an implicit GEMM on v_mfma_f32_32x32x16_f16 over the walk of cpx_graph_conv_core.h, K in chunks of 32 input
// channels; a chunk is two K blocks m = 0, 1 of 16 channels, a block three MFMAs per tile: wl * xh, wh * xl, wh * xh, the
// small terms first.
// A: two threads per pixel load 16 float32 channels each (4 x 128 bits), multiply by their pixel's own sample's `up`,
//    split into xh and xl and write 4 x 16 bytes into a [pixel][plane][k] image of 128-byte rows, double buffered: one
//    barrier per step.  No fp16 copy of the activation goes to memory.
// B: the host packs both filter planes in fragment order ([tap][chunk][tile][plane][m][lane][16 bytes],
//    GRAPH_CONV_H2_KC): a step's four fragments of a tile are 256 consecutive 16-byte pieces, one per thread.  The
//    workgroup takes them from global memory with 128-bit loads a step ahead, ONCE (each wave loading all of them for
//    itself moved 64 KB per step through the vector memory path, four times the patch: measured, the step then took the
//    loads' time, not the products'), and parks them in LDS beside the patch, double buffered under the same barrier.
//    Thread t writes piece t and lane l reads piece 64 f + l: consecutive lanes, consecutive 16 bytes, no bank conflict.
// Lane map (checked with exact operands by tests/test_tflite_h2_gpu.py::test_operand_map_exact): lane l holds row /
// column l & 31 and the eight consecutive k = 8 * (l >> 5) + j of a 16-channel K block of A and of B; C / D is the map
// of the other 32 x 32 forms (acc_row).
// LDS banks.  A row is 8 slots of 16 bytes: slot 4 * plane + 2 * m + h holds k = 16 m + 8 h .. + 8 of the plane.  Pixel r
// stores slot s at slot s ^ swz(r), swz(r) = ((r >> 1) & 7) ^ ((r & 1) << 2).  A ds_read_b128 is served in four groups
// of 16 lanes whose rows r = lane & 31 cover all residues mod 16, all at one s; its bank row is 256 bytes = 16 slots, so
// pixel r lands on bank slot 8 * (r & 1) + (s ^ swz(r)).  For a fixed r & 1 the eight values of (r >> 1) & 7 give eight
// different slots, and r & 1 picks the half: 16 lanes, 16 slots, no conflict.  A ds_write_b128 is served in groups of 8
// consecutive threads = 4 consecutive pixels x 2 halves (s and s ^ 2) on a bank row of 128 bytes = 8 slots, slot
// s ^ swz(r): over the four pixels (bit 0 of (r >> 1), r & 1) takes all four values and lands in bits 0 and 2 of swz,
// which together with the half in bit 1 makes 8 different slots: no conflict either.
#include <hip/hip_runtime.h>

#include "cpx_graph_conv_core.h"
#include "cpx_graph_minmax.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int KH = GRAPH_CONV_H2_KC;  // input channels per step
constexpr int ROW = 32;               // dwords of a pixel's row of the A image: 2 planes x KH fp16

// two float32 -> their two fp16 planes as packed pairs, the form of split_pair2_h (cpx_cnn_bf3.hip): hi is rounded to
// nearest even (v_cvt_pk_f16_f32); x - hi is exact in float32, so ONE mixed-precision fused multiply-add per element
// (x * 1.0 - hi, float32 inside, rounded to nearest fp16 once) is convert-back, subtract, convert
__device__ __forceinline__ void split_pair2_h(float a, float b, unsigned& p0, unsigned& p1) {
  const f16x2 v = {(_Float16)a, (_Float16)b};
  p0 = __builtin_bit_cast(unsigned, v);
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(p1) : "v"(a), "v"(p0));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(p1) : "v"(b), "v"(p0));
}

__device__ __forceinline__ int swz(int r) { return ((r >> 1) & 7) ^ ((r & 1) << 2); }

// RANGE: one workgroup per sample; out = [up, down, 0, 0]
template <int VW>
__global__ __launch_bounds__(GRAPH_MINMAX_THREADS) void graph_range_kernel(GraphOpArgs a) {
  const size_t n = blockIdx.x;
  float lo, hi;
  sample_min_max<VW>(a.in0, n, &lo, &hi);
  if (threadIdx.x != 0) return;
  const RangeParams p = range_params(fmaxf(-lo, hi));
  float* out = a.out.p + n * a.out.sample_stride;
  out[0] = p.up;
  out[1] = p.down;
  out[2] = 0.0f;
  out[3] = 0.0f;
}

template <int NTN>
__global__ __launch_bounds__(CT) void graph_conv_h2_kernel(GraphOpArgs a, ConvGeom g) {
  __shared__ __attribute__((aligned(16))) unsigned s_a[2][BM * ROW];   // [pixel][plane][k], swizzled slots
  __shared__ __attribute__((aligned(16))) u32x4 s_b[2][NTN * CT];      // [tile][2 * plane + m][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * BM;
  const int tile0 = blockIdx.y * NTN;
  const int Cin = a.in0.C;

  // the stager's 16 channels are K block m = half; its sample's `up` is read once
  const ConvStager<float> st = conv_stager(a, g, a.in0.p, p0, tid, 0);
  const int spx = st.spx, half = st.half;
  const float* in_n = st.in_n;
  const float up = a.in1.p[(size_t)st.px.n * a.in1.sample_stride];
  const u32x4* wq = reinterpret_cast<const u32x4*>(a.weights);
  const int wbase = spx * ROW, wsw = swz(spx);
  // fragment role: row 32 * wave + (lane & 31), k half lane >> 5 (32 * wave changes no bit that swz reads)
  const int rbase = (32 * wave + (lane & 31)) * ROW, rsw = swz(lane & 31), kh8 = lane >> 5;

  const int steps = a.kh * a.kw * g.nchunks;

  f32x16 acc[NTN];
#pragma unroll
  for (int t = 0; t < NTN; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  f32x4 pre[4];
  u32x4 bnext[NTN];   // piece tid of every tile's four fragments

  // global -> registers of step s.  A masked element (outside the image or the tile, beyond Cin) is 0 in both planes
  auto fetch = [&](int s) {
    const ConvPatch f = conv_patch(a, st, s, g.nchunks, KH);
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
    prefetch_fragments<NTN>(wq, s, g.ntiles, tile0, CT, tid, bnext);
  };

  fetch(0);
  for (int s = 0; s < steps; ++s) {
    unsigned* buf = s_a[s & 1];
    // scale (exact), split, store: the thread's 16 channels are K block `half`, slots 2 * half + {0, 1} of each plane
    u32x4 hi[2], lo[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned h0, l0, h1, l1;
      split_pair2_h(pre[q].x * up, pre[q].y * up, h0, l0);
      split_pair2_h(pre[q].z * up, pre[q].w * up, h1, l1);
      hi[q >> 1][2 * (q & 1)] = h0;
      hi[q >> 1][2 * (q & 1) + 1] = h1;
      lo[q >> 1][2 * (q & 1)] = l0;
      lo[q >> 1][2 * (q & 1) + 1] = l1;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      *reinterpret_cast<u32x4*>(buf + wbase + 4 * ((2 * half + h) ^ wsw)) = hi[h];
      *reinterpret_cast<u32x4*>(buf + wbase + 4 * ((4 + 2 * half + h) ^ wsw)) = lo[h];
    }
    u32x4* bbuf = s_b[s & 1];
#pragma unroll
    for (int t = 0; t < NTN; ++t) bbuf[t * CT + tid] = bnext[t];
    __syncthreads();   // (the other buffers are free: every wave read them before it reached this barrier)
    if (s + 1 < steps) fetch(s + 1);   // in flight while the matrix cores work on step s
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const f16x8 xh = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(buf + rbase + 4 * ((2 * m + kh8) ^ rsw)));
      const f16x8 xl = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(buf + rbase + 4 * ((4 + 2 * m + kh8) ^ rsw)));
#pragma unroll
      for (int t = 0; t < NTN; ++t) {
        if (tile0 + t >= g.ntiles) continue;
        const f16x8 wh = __builtin_bit_cast(f16x8, bbuf[t * CT + 64 * m + lane]);
        const f16x8 wl = __builtin_bit_cast(f16x8, bbuf[t * CT + 64 * (2 + m) + lane]);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh, acc[t], 0, 0, 0);
      }
    }
  }

  // epilogue: accumulator register r of a lane is pixel acc_row(r, tid) of the wave's 32, channel lane & 31 of the
  // tile; every pixel takes its own sample's `down`
  const long long pb = p0 + 32 * wave;
  if (pb >= g.P) return;
  const float* wdown = reinterpret_cast<const float*>(wq + (size_t)steps * g.ntiles * 4 * 64);
  const long long nb = pb / g.HoWo;
  const int remb = (int)(pb - nb * g.HoWo);
#pragma unroll
  for (int t = 0; t < NTN; ++t) {
    const int ch = (tile0 + t) * 32 + (lane & 31);
    if (tile0 + t >= g.ntiles || ch >= a.out.C) continue;
    const float sc = a.scale ? a.scale[ch] : 1.0f;
    const float sh = a.shift ? a.shift[ch] : 0.0f;
    const float wd = wdown[ch];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = acc_row(r, tid);
      if (pb + i >= g.P) continue;
      const SamplePixel o = sample_step(nb, remb + i, g.HoWo);
      const float f = a.in1.p[(size_t)o.n * a.in1.sample_stride + 1] * wd;   // an exact power of two
      const float v = acc[t][r] * f;
      a.out.p[(size_t)o.n * a.out.sample_stride + (unsigned)(o.rem * a.out.cstride + ch)] = activate(v * sc + sh, a.act);
    }
  }
}

}  // namespace

void launch_graph_h2_op(const GraphOpArgs& a, hipStream_t s) {
  const int vec4 = quads(a.in0);
  switch (a.kind) {
    case CPX_GRAPH_RANGE:
      if (vec4)
        hipLaunchKernelGGL(graph_range_kernel<4>, dim3((unsigned)a.N), dim3(GRAPH_MINMAX_THREADS), 0, s, a);
      else
        hipLaunchKernelGGL(graph_range_kernel<1>, dim3((unsigned)a.N), dim3(GRAPH_MINMAX_THREADS), 0, s, a);
      break;
    case CPX_GRAPH_CONV_F16X2: {
      const ConvGeom g = conv_geom(a.N, a.in0, a.out, KH, 1, group_quads<GraphView>);
      const unsigned gx = (unsigned)((g.P + BM - 1) / BM);
      conv_dispatch_ntn(g.ntiles, [&](auto ntn, int rows) {
        hipLaunchKernelGGL(graph_conv_h2_kernel<decltype(ntn)::value>, dim3(gx, rows), dim3(CT), 0, s, a, g);
      });
      break;
    }
    default:
      break;
  }
}

}  // namespace cpx
