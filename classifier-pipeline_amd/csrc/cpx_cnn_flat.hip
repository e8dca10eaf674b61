// cpx_cnn_flat.hip -- conv_flat16_kernel: stage 4's stride-1 3x3 layer (128 -> 128 channels per group on maps small enough for
// the flattened tiling) in fp16x2 on v_mfma_f32_16x16x32_f16.
//
// Same flattened bands (cpx_flat_band_core.h) and the same arithmetic as conv_bf3flat_kernel<2, 256, 2, true> (cpx_cnn_bf3.hip):
// two fp16 planes per operand, three products x0 w1 + x1 w0 + x0 w0, power-of-two scaling, the overflow word, float32
// accumulators.  The split-operand loops are bound by the clock the chip holds under load (profiles/r01_conv_power_probe.md), so
// what differs is work the result does not need, taken out:
//   shape    16x16x32 holds a higher clock than 32x32x16 at equal cycles (profiles/r04_mfma_shape_probe.txt).  K = 32 = the 32
//            channels of one tap; A = weights (M = 16 output channels), B = 16 consecutive flattened positions, as in
//            conv_bf3w_kernel and conv_rw_kernel: a lane's four accumulator values are four consecutive channels of one position
//   patch    ONE workgroup computes all 128 columns of a group for its band: the patch is fetched, normalised, range-tested and
//            split once per band (conv_bf3flat_kernel: once per 64-column slice), in four chunks of 32 channels instead of eight
//            of 16.  Two patch buffers: one barrier per chunk, four per band (sixteen before)
//   weights  A fragments come straight from the layer's `half` image in L2 into registers, one tap ahead of their products: a
//            K = 32 fragment pairs two neighbouring 16-channel chunks of the image, lanes 0-15 / 16-31 / 32-47 / 48-63 on four
//            256-byte runs.  No LDS round trip and no barrier for the weights; a group's image (576 KB) stays in the XCD's L2
//   epilogue affine, residual, ReLU and store are 16-byte accesses from the registers: no transpose through LDS, no barrier
//            behind the last products
// Geometry: 256 threads, band = 128 positions; wave (wp, wc) owns PT position tiles x 16 / PT channel tiles of 16 x 16, 64
// accumulator registers.  Shipped: PT = 8, all 128 positions x 32 channels -- per tap and chunk 4 global + 16 LDS fragment reads
// feed 48 products and no weight is read by two waves; PT = 4 (64 x 64: 8 + 8 reads, every weight read by two waves) measured
// 2 % slower, PT = 2 needs scratch.  LDS: two patch buffers [plane][quarter pair][F_NPXP pixels][2] of 16-byte entries = 2 x
// 32.75 KB, + 2 KB of BatchNorm scale / shift: two workgroups per CU, two waves per SIMD on 256 registers each.
// Measurements: profiles/stage4_flat16_experiments.md.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cpx_cnn_dev.h"
#include "cpx_conv_layout_core.h"
#include "cpx_flat_band_core.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

constexpr int F_CT = 256, F_BAND = 128, F_COLS = 128;  // threads, positions and columns of a workgroup
constexpr int F_NPXC = 256;                            // staged pixels a band may need (flat_band_max_pixels)
// pixels per (plane, quarter pair) region: >= F_NPXC, and 262 * 32 B = 64 mod 128 so that the two quarter pairs of a pixel
// use different banks (conv_bf3w_kernel's patch layout); a buffer also holds the shortcut's operand (below)
constexpr int F_NPXP = 262;
constexpr int F_PLANE = 2 * F_NPXP * 2;  // entries of a plane: [quarter pair][pixel][2]
constexpr int F_BUF = 2 * F_PLANE;       // entries of a patch buffer
// the fused shortcut's operand: [chunk of 32][plane][quarter pair][F_BANDP positions][2]
constexpr int F_BANDP = 130;  // 130 * 32 B = 64 mod 128
constexpr int F_SCPLANE = 2 * F_BANDP * 2;
static_assert(F_NPXP >= F_NPXC && 2 * 2 * F_SCPLANE <= F_BUF, "a patch buffer holds a band's patch, or the shortcut's operand");
// behind the buffers: the BatchNorm prologue's scale and shift of the group's input channels (times act_scale), read back at
// each commit instead of living in sixteen registers under the products
constexpr int F_BNC = 256;  // input channels per group they hold
// experiment builds (scratch/build_variant.sh): the wave split, and the loads left to the scheduler
#ifndef CPX_FLAT16_PT
#define CPX_FLAT16_PT 8
#endif
#ifndef CPX_FLAT16_AHEAD
#define CPX_FLAT16_AHEAD 1
#endif
constexpr size_t F_LDS = (size_t)2 * F_BUF * 16 + (size_t)2 * F_BNC * sizeof(float);
static_assert(2 * F_LDS <= 160 * 1024, "two workgroups per CU");

// SC: the fused 1x1 shortcut of a.sc_in (64 channels per group, stride a.sc_stride) as fp16x2 products from a.sc_planes, behind
// the last chunk like two more chunks with a single tap.  PT: position tiles of a wave (8: 128 positions x 32 channels; 4: 64 x 64)
template <bool SC, int PT>
__global__ __launch_bounds__(F_CT) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_flat16_kernel(ConvArgs a, const uint4* __restrict__ wimg, Tiles td) {
  constexpr int CTN = 16 / PT;  // channel tiles of a wave
  constexpr int NWP = 8 / PT;   // waves along the band's positions
  constexpr int NP = 4 * F_NPXC / F_CT;  // staging items of a thread: (pixel, 8 channels)
  static_assert(PT * CTN == 16 && NWP * (F_COLS / (16 * CTN)) == F_CT / 64, "four waves cover 8 x 8 tiles");
  static_assert(NP * F_CT == 8 * F_BAND, "the shortcut's operand is staged through the same registers");
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  if (*a.ovf != 0) return;  // (the three-plane rerun computes the layer)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int wp = wave % NWP, wc = wave / NWP;
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);  // XCD-contiguous tiles (cpx_cnn.hip)
  const int ti = tile_split(bid, td.m_tx, td.tiles_x);  // band inside the sample
  const int n = bid;
  const int g = blockIdx.y;
  const int cin_g = a.Cin / a.groups;
  const int M = a.Ho * a.Wo;
  const FlatBand fb = flat_band(ti, F_BAND, a.Ho, a.Wo);
  const float* in_n = a.in + (size_t)n * a.H * a.W * a.Cin + (size_t)g * cin_g;
  const int nchunks = cin_g / 32;
  const int chw = g * F_COLS + wc * (16 * CTN) + 4 * lq;  // this lane's first channel (of tile 0: + 16 per tile)
  const int pw0 = fb.p0 + wp * (16 * PT) + l15;           // this lane's position (of tile 0: + 16 per tile)

  // The residual goes INTO the accumulators before the first product when the output is not scaled (conv_bf3_kernel); the
  // accumulators hold act_scale * w_scale[channel] times the sum, so must the residual
  const bool res_in_acc = a.residual != nullptr && a.out_scale == nullptr;
  f32x4 acc[PT][CTN];
  if (res_in_acc) {
    const float* res_n = a.residual + (size_t)n * M * a.Cout;
    f32x4 rs[CTN];
#pragma unroll
    for (int ct = 0; ct < CTN; ++ct) rs[ct] = *reinterpret_cast<const f32x4*>(a.w_scale + chw + ct * 16) * a.act_scale;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const unsigned ro = (__umul24((unsigned)min(pw0 + pt * 16, M - 1), (unsigned)a.Cout) + (unsigned)chw) << 2;
#pragma unroll
      for (int ct = 0; ct < CTN; ++ct) acc[pt][ct] = *reinterpret_cast<const f32x4*>(at_off(res_n, ro + ct * 64)) * rs[ct];
    }
  } else {
#pragma unroll
    for (int pt = 0; pt < PT; ++pt)
#pragma unroll
      for (int ct = 0; ct < CTN; ++ct) acc[pt][ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  // B fragments: quarter lq of the chunk's 32 channels at this lane's position -- entry of tile pt and tap (ky, kx), plane 0
  int bb[PT];
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) bb[pt] = ((lq >> 1) * F_NPXP + flat_patch_base(fb, pw0 + pt * 16, M, a.Wo)) * 2 + (lq & 1);
  // A fragments: the image is [g][chunk of 16][plane][9][2][cout_g]; quarter lq = chunk 2 c + (lq >> 1), half lq & 1
  const uint4* wg = wimg + (size_t)g * (cin_g / 16) * 36 * F_COLS;
  const unsigned wlane = (unsigned)(((lq >> 1) * 36 + (lq & 1)) * F_COLS + wc * (16 * CTN) + l15) << 4;
  u32x4 wf[2][CTN][2];
  const auto load_w = [&](u32x4 (&w)[CTN][2], int cc, int tap) {
    const u32x4* wt = reinterpret_cast<const u32x4*>(wg + (size_t)(cc * 72 + tap * 2) * F_COLS);  // (uniform)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int ct = 0; ct < CTN; ++ct) w[ct][p] = *at_off(wt, wlane + (unsigned)((p * 18 * F_COLS + ct * 16) << 4));
  };

  // staging: an item is 8 channels (one quarter) of a patch pixel's 32-channel chunk; the four quarters of a pixel sit on
  // adjacent lanes (128 contiguous bytes).  A thread keeps its quarter; surplus threads repeat the last pixel
  const int my_q = tid & 3;
  unsigned soff[NP], inside = 0;
  int se[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int px = min((tid + i * F_CT) >> 2, fb.npx - 1);
    int iy, ix;
    flat_item_pixel(fb, px, iy, ix);
    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) inside |= 1u << i;
    // the loads are unconditional (clamped addresses); padding is zeroed at commit, after the prologue
    soff[i] = (pix_off(min(max(iy, 0), a.H - 1), min(max(ix, 0), a.W - 1), a.W, a.Cin) + (unsigned)(8 * my_q)) << 2;
    se[i] = ((my_q >> 1) * F_NPXP + px) * 2 + (my_q & 1);
  }
  f32x4 pre_p[NP][2];
  f32x4* s_bn = reinterpret_cast<f32x4*>(lds4 + 2 * F_BUF);  // [scale | shift][F_BNC / 4]
  if (a.in_scale && tid < cin_g / 4) {  // relu(x s + b) 2^k = relu(x (s 2^k) + b 2^k), exactly
    s_bn[tid] = *reinterpret_cast<const f32x4*>(a.in_scale + g * cin_g + 4 * tid) * a.act_scale;
    s_bn[F_BNC / 4 + tid] = *reinterpret_cast<const f32x4*>(a.in_shift + g * cin_g + 4 * tid) * a.act_scale;
  }
  const auto load_patch = [&](int cc) {
    const int cn = cc * 32;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      pre_p[i][0] = *reinterpret_cast<const f32x4*>(at_off(in_n + cn, soff[i]));
      pre_p[i][1] = *reinterpret_cast<const f32x4*>(at_off(in_n + cn, soff[i] + 16));
    }
  };
  // eight scaled float32 -> the entry of each fp16 plane; the largest magnitude goes into vmax
  const auto split_entry = [](const float (&v)[8], float& vmax, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) vmax = fmaxf(fmaxf(fabsf(v[j]), fabsf(v[j + 1])), vmax);
    unsigned q0[4], q1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split2<true>(v[2 * j], v[2 * j + 1], q0[j], q1[j]);
    hi = u32x4{q0[0], q0[1], q0[2], q0[3]};
    lo = u32x4{q1[0], q1[1], q1[2], q1[3]};
  };

  load_patch(0);
  __syncthreads();  // (s_bn)
  for (int cc = 0; cc < nchunks; ++cc) {
    load_w(wf[0], cc, 0);  // (in flight under the commit and the barrier)
    u32x4* buf = reinterpret_cast<u32x4*>(lds4) + (cc & 1) * F_BUF;
    {
      // ---- registers -> LDS: BatchNorm + ReLU prologue, padding zeroed, range test, split into fp16 planes ----
      float vmax = 0.0f;
      f32x4 psc[2], psh[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        psc[k] = s_bn[cc * 8 + my_q * 2 + k];
        psh[k] = s_bn[F_BNC / 4 + cc * 8 + my_q * 2 + k];
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const bool in = (inside >> i) & 1;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = pre_p[i][j >> 2][j & 3];
        if (a.in_scale) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = fmaxf(__fmaf_rn(v[j], psc[j >> 2][j & 3], psh[j >> 2][j & 3]), 0.0f);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= a.act_scale;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = in ? v[j] : 0.0f;
        u32x4 hi, lo;
        split_entry(v, vmax, hi, lo);
        buf[se[i]] = hi;
        buf[F_PLANE + se[i]] = lo;
      }
      if (vmax > F16_MAX) atomicOr(a.ovf, 1);  // out of fp16's range: the three-plane kernel reruns the layer
    }
    // one barrier per chunk: the other buffer was last read a chunk ago, and every wave is past those products here
    __syncthreads();
    if (cc + 1 < nchunks) {
      load_patch(cc + 1);  // (in flight under this chunk's products)
    } else if (SC) {
      // the shortcut's operand through the same registers: item = 8 channels (block tid & 7 of the 64) of band position
      // (tid + i 256) >> 3, the strided pixel of the block input
      const float* sc_n = a.sc_in + (size_t)n * a.sc_H * a.sc_W * a.sc_cin + g * 64 + 8 * (tid & 7);
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int sp = min(fb.p0 + ((tid + i * F_CT) >> 3), M - 1);
        const int sy = sp / a.Wo, sx = sp - sy * a.Wo;
        const float* src = sc_n + ((size_t)(sy * a.sc_stride) * a.sc_W + sx * a.sc_stride) * a.sc_cin;
        pre_p[i][0] = *reinterpret_cast<const f32x4*>(src);
        pre_p[i][1] = *reinterpret_cast<const f32x4*>(src + 4);
      }
    }
    // Steps of one (tap, position tile): 3 CTN products each.  The A fragments stay a tap ahead and the B fragments a step
    // ahead of their products; the scheduling barrier in front of a step's products keeps them there (left to itself the
    // scheduler sinks every load to its first use, to save registers, and each step then waits for L2 or LDS)
    u32x4 bv[2][2];
    const auto read_b = [&](u32x4 (&b)[2], int tap, int pt) {
      const int e = bb[pt] + flat_tap_offset(fb, tap / 3, tap % 3) * 2;
#pragma unroll
      for (int p = 0; p < 2; ++p) b[p] = buf[p * F_PLANE + e];
    };
    read_b(bv[0], 0, 0);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap + 1 < 9) load_w(wf[(tap + 1) & 1], cc, tap + 1);
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int st = tap * PT + pt;
        if (st + 1 < 9 * PT) read_b(bv[(st + 1) & 1], (st + 1) / PT, (st + 1) % PT);
        if (CPX_FLAT16_AHEAD) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ct = 0; ct < CTN; ++ct) plane_products16<2, true>(bv[st & 1], wf[tap & 1][ct], acc[pt][ct]);
      }
    }
  }

  if constexpr (SC) {
    // The fused 1x1 shortcut: K = 64 = two chunks of 32, one tap.  Weights [g][chunk of 32][plane][quarter][cout_g]
    // (split_shortcut_kernel) straight into the fragment registers; the operand -- times sc_xscale, split like an activation,
    // the same range test -- into the buffer the last chunk did not use; one barrier
    const u32x4* scw = reinterpret_cast<const u32x4*>(a.sc_planes) + (size_t)g * 16 * F_COLS;
    const unsigned sclane = (unsigned)(lq * F_COLS + wc * (16 * CTN) + l15) << 4;
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int ct = 0; ct < CTN; ++ct) wf[c][ct][p] = *at_off(scw, sclane + (unsigned)((((c * 2 + p) * 4) * F_COLS + ct * 16) << 4));
    u32x4* sbuf = reinterpret_cast<u32x4*>(lds4) + (nchunks & 1) * F_BUF;
    {
      const int j = tid & 7, c = j >> 2, qq = j & 3;
      float vmax = 0.0f;
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = pre_p[i][k >> 2][k & 3] * a.sc_xscale;
        u32x4 hi, lo;
        split_entry(v, vmax, hi, lo);
        const int e = ((c * 2 * 2 + (qq >> 1)) * F_BANDP + ((tid + i * F_CT) >> 3)) * 2 + (qq & 1);
        sbuf[e] = hi;
        sbuf[F_SCPLANE + e] = lo;
      }
      if (!(vmax <= F16_MAX)) atomicOr(a.ovf, 1);  // (out of fp16's range, or not a number: the rerun computes the layer)
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      u32x4 bv[PT][2];
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int p = 0; p < 2; ++p)
          bv[pt][p] = sbuf[((c * 2 + p) * 2 + (lq >> 1)) * (F_BANDP * 2) + (wp * (16 * PT) + pt * 16 + l15) * 2 + (lq & 1)];
#pragma unroll
      for (int pt = 0; pt < PT; ++pt)
#pragma unroll
        for (int ct = 0; ct < CTN; ++ct) plane_products16<2, true>(bv[pt], wf[c][ct], acc[pt][ct]);
    }
  }

  // ---- epilogue, from the registers: a lane holds channels chw + 16 ct .. + 3 of position pw0 + 16 pt; the NHWC offset of
  // flattened position p is p * Cout ----
  float* out_n = a.out + (size_t)n * M * a.Cout;
  const float* res_n = (a.residual && !res_in_acc) ? a.residual + (size_t)n * M * a.Cout : nullptr;
  f32x4 os[CTN], ob[CTN];
#pragma unroll
  for (int ct = 0; ct < CTN; ++ct) {
    const int ch = chw + ct * 16;
    const f32x4 one = {1.0f, 1.0f, 1.0f, 1.0f}, zero = {0.0f, 0.0f, 0.0f, 0.0f};
    os[ct] = a.out_scale ? *reinterpret_cast<const f32x4*>(a.out_scale + ch) : one;
    os[ct] *= *reinterpret_cast<const f32x4*>(a.w_unscale + ch) * a.act_unscale;  // (powers of two: exact)
    ob[ct] = (a.out_shift ? *reinterpret_cast<const f32x4*>(a.out_shift + ch) : zero) +
             (a.sc_in && a.sc_bias ? *reinterpret_cast<const f32x4*>(a.sc_bias + ch) : zero);
  }
#pragma unroll
  for (int pt = 0; pt < PT; ++pt) {
    const int p = pw0 + pt * 16;
    if (p < M) {
      const unsigned o = (__umul24((unsigned)p, (unsigned)a.Cout) + (unsigned)chw) << 2;  // inside one sample: < 2^32 bytes
      f32x4 v[CTN];
#pragma unroll
      for (int ct = 0; ct < CTN; ++ct) v[ct] = acc[pt][ct] * os[ct] + ob[ct];
      if (res_n) {  // (the loads of a position's tiles first, then its stores: see conv_bf3_kernel)
        f32x4 rv[CTN];
#pragma unroll
        for (int ct = 0; ct < CTN; ++ct) rv[ct] = *reinterpret_cast<const f32x4*>(at_off(res_n, o + ct * 64));
#pragma unroll
        for (int ct = 0; ct < CTN; ++ct) v[ct] += rv[ct];
      }
#pragma unroll
      for (int ct = 0; ct < CTN; ++ct) {
        if (a.relu) {
          v[ct].x = relu_bits(v[ct].x); v[ct].y = relu_bits(v[ct].y); v[ct].z = relu_bits(v[ct].z); v[ct].w = relu_bits(v[ct].w);
        }
        *reinterpret_cast<f32x4*>(at_off(out_n, o + ct * 64)) = v[ct];
      }
    }
  }
}

template <bool SC, int PT>
int launch_flat16_t(const ConvArgs& a, const uint4* wimg, hipStream_t s) {
  Tiles td{};
  if (const int rc = fill_tiles(td, flat_bands(F_BAND, a.Ho, a.Wo), 1, a.N, TILES_PER_LAUNCH)) return rc;
  static bool lds_ready[64];
  if (!cpx_dyn_lds_ready(reinterpret_cast<const void*>(conv_flat16_kernel<SC, PT>), lds_ready, 160 * 1024 - 1024)) return -1;
  hipLaunchKernelGGL((conv_flat16_kernel<SC, PT>), dim3((unsigned)td.total, (unsigned)a.groups), dim3(F_CT), F_LDS, s, a, wimg, td);
  return 0;
}

}  // namespace

// the launches conv_flat16_kernel takes: fp16x2 (a.half, two planes, the overflow word; w_scale / w_unscale / act_scale set) of a
// stride-1 SAME 3x3 layer with 128 columns and 32-channel chunks per group whose bands fit the patch buffer, float32 in and out,
// not the guarded rerun; a fused shortcut only as fp16 planes.  `wimg`: the layer's `half` image.  -2: not such a launch
// (conv_bf3flat_kernel has it)
int launch_conv_flat16(const ConvArgs& a, const void* wimg, hipStream_t s) {
  if (!a.flat16 || !a.half || a.planes != 2 || a.ovf == nullptr || a.guard != nullptr || a.in_planes || a.out_planes) return -2;
  if (a.ksize != 3 || a.stride != 1 || a.pad_top != 1 || a.pad_left != 1 || a.H != a.Ho || a.W != a.Wo || a.groups < 1) return -2;
  if (a.Cout != F_COLS * a.groups || a.Cin % (32 * a.groups) || a.Cin < 32 * a.groups || a.Cin > F_BNC * a.groups) return -2;
  if (flat_band_max_pixels(F_BAND, a.Wo) > F_NPXC) return -2;
  // byte offsets inside a sample are 32-bit, pixel offsets formed with 24-bit multiplies (pix_off)
  if ((long long)a.H * a.W >= (1 << 24) || a.Cin >= (1 << 24) || (long long)a.H * a.W * std::max(a.Cin, a.Cout) >= (1ll << 30)) return -2;
  const uint4* wi = reinterpret_cast<const uint4*>(wimg);
  if (a.sc_in) {
    if (!a.sc_planes || !conv_shortcut_planes_layer(a, a.sc_cin / a.groups) || a.residual || a.sc_stride < 1 || !(a.sc_xscale > 0.0f) ||
        (a.sc_H - 1) / a.sc_stride + 1 != a.Ho || (a.sc_W - 1) / a.sc_stride + 1 != a.Wo || (long long)a.sc_H * a.sc_W * a.sc_cin >= (1ll << 31))
      return -2;  // (the float32 side product stays with conv_bf3flat_kernel)
    return launch_flat16_t<true, CPX_FLAT16_PT>(a, wi, s);
  }
  return launch_flat16_t<false, CPX_FLAT16_PT>(a, wi, s);
}

}  // namespace cpx
