// cpx_cnn_blk.hip -- a stage-2 residual block in one launch, its two convolutions on DIFFERENT WAVES (round 6).
//
// conv_block32_kernel (cpx_cnn_bf3.hip) keeps `mid` in LDS but runs a tile's phases one after the other on all eight waves:
// patch commit, first convolution, mid epilogue, second convolution, output epilogue, four barriers -- the matrix pipe is busy
// 49 % of the cycles (profiles/r06_conv_sq_counters.json), 31 % of a tile's time is spent in the phases that issue no product
// (profiles/r05_block32_experiments.md, cycle stamps), and a second workgroup that would fill them does not fit: patch / mid
// 51 KB + both weight images 74 KB = 125 KB of LDS.
//
// Here the workgroup is a two-stage pipeline over tiles.  Waves 0-3 ("A") compute the FIRST convolution of tile k + 1 while
// waves 4-7 ("B") compute the SECOND convolution of tile k; wave w and wave w + 4 share a SIMD, so every SIMD always has two
// independent product streams, and a step has two barriers:
//   phase 1   A: products of conv a (patch P -> accumulators)        B: products of conv b (mid M[k & 1] -> accumulators)
//             both: the global loads of tile k + 2's patch are issued between the products; B: tile k's residual rows
//   phase 2   A: mid epilogue (folded BatchNorm + ReLU, fp16 split) -> M[(k + 1) & 1]
//             B: output epilogue (unscale, bias, residual, ReLU, 16-byte stores)
//             both: tile k + 2's patch takes its prologue + split and lands in P (free: A has read it)
// Each wave holds ONE convolution's weights for ITS 16 output channels in registers (9 taps x 2 planes x 16 bytes = 72
// VGPRs, the conv_rw_kernel idea), so the weight images leave LDS: P (51.5 KB) + two mid buffers (2 x 41.7 KB) = 135 KB.
// Fragments: a wave owns whole pixel rows, so the row read for tap row 0 of output row o is tap row 1 of o - 1 and tap row 2
// of o - 2 (cpx_cnn_rw.hip): A reads 11 patch rows per kx for 9 mid rows (+ the two extra mid columns as three 16-pixel edge
// groups without reuse), B 10 mid rows per kx for 8 output rows.
// The halo carry: the two extra mid columns of a tile at ox are image columns ox + 15 and ox + 16 -- mid columns 0 and 1 of
// the tile at ox + 16, the same sums of the same taps in the same order.  Where a workgroup walks a tile row right to left
// (cpx_conv_layout_core.h: WALK_ROWS), that tile is the one B works on while A starts this one, so A copies the 36 pixels
// (4.6 KB) from M[k & 1] to M[(k + 1) & 1] instead of computing them: 243 products instead of 297 on A's longer half, no
// edge epilogue.  `carry` is decided from the two tiles' coordinates alone, whatever the walk; CPX_BLOCK32_CARRY=0 turns it off.
// Hazards, with no barrier beyond the step's two: the source columns were written by A in step k - 1 and B only reads them
// in step k; the destination buffer was last read by B in step k - 1 and is read again in step k + 1; a barrier lies
// between each pair.  The overflow word is unchanged: the carried planes were range-checked by the tile that computed them.
// Arithmetic: conv_block32_kernel's (fp16x2, the same planes and scales); the taps are summed kx-major, another float32
// order of the same terms -- logits within 1e-5 of the two-launch form (tests/test_cnn_gpu.py).
// Reference semantics: /root/reference/src/ml_tools/resnet/wr_resnet.py:49-98 (wr_block).
// The device vocabulary (vector types, at_off / pix_off, split_pair2_h, mfma16<true>, pk_max_u16, med3, static_for) is
// cpx_cnn_dev.h's, the tiles, their walk and the grid's width cpx_conv_layout_core.h's: shared with cpx_cnn_bf3.hip and cpx_cnn_rw.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "cpx_cnn_dev.h"
#include "cpx_conv_layout_core.h"
#include "cpx_kernels.h"

namespace cpx {

namespace {

constexpr int K_T = 16;                          // output tile: 16 x 16
constexpr int K_PP = 20, K_PNPX = 400;           // the staged input patch: 20 x 20
constexpr int K_PNPXP = 402;                     // pixels per (plane, quarter pair) region, x 32 B = 64 mod 128 (cpx_cnn_bf3.hip: B_NPXP)
constexpr int K_MP = 18;                         // mid: 18 x 18 (324 pixels)
constexpr int K_MNPXP = 326;
constexpr int K_PBUF = 2 * 2 * K_PNPXP * 2;      // 16-byte entries: [plane][quarter pair][pixel][2]
constexpr int K_MBUF = 2 * 2 * K_MNPXP * 2;
constexpr int K_CT = 512;
constexpr int K_NP = 7;                          // staging items per thread: 400 pixels x 8 pieces = 3,200 = 6 x 512 + 128
constexpr int K_PPI = K_CT / 8;                  // patch pixels per staging round
constexpr int K_WROW = 2 * 3 * 4 * 32;           // entries of one kernel row of a group's fp16 image: [plane][kx][quarter][32]
constexpr int K_WIMG = 3 * K_WROW;
// staged items are converted (BatchNorm, padding, split) and stored in phase 2.  Converting them between the products of phase 1
// measured slower (scratch/cnn_probe.py 1536, six launches: 57.7 against 50.9 ms): the conversion's 245 vector instructions per
// wave compete with the two product streams for the SIMD's issue slots, and a second tile in the registers pushes the residual
// rows behind the products
constexpr size_t K_LDS = (size_t)(K_PBUF + 2 * K_MBUF) * 16;

__global__ __launch_bounds__(K_CT) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_block32s_kernel(ConvArgs a, ConvArgs b, const uint4* __restrict__ wa, const uint4* __restrict__ wb, BlkTiles td, int carry_on) {
  if (*a.ovf != 0) return;  // (the block's guarded three-plane launches follow)
  extern __shared__ __attribute__((aligned(16))) uint4 lds4[];
  uint4* s_P = lds4;
  uint4* s_M = lds4 + K_PBUF;  // two buffers of K_MBUF entries
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i16 = lane & 15, q = lane >> 4;
  const bool is_a = wave < 4;                       // (wave-uniform) first or second convolution
  const int ct = wave & 1, hh = (wave >> 1) & 1;    // the wave's 16 of the group's 32 output channels; upper / lower half of the rows
  const int g = blockIdx.y;
  const int C = b.Cout, H = a.H, W = a.W;

  // ---- the wave's weights: ONE convolution's fp16 image [ky][plane][kx][quarter][32] of its group, its 16 columns ----
  u32x4 Wr[9][2];
  {
    const u32x4* wg = reinterpret_cast<const u32x4*>(is_a ? wa : wb) + (size_t)g * K_WIMG + q * 32 + ct * 16 + i16;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int p = 0; p < 2; ++p) Wr[ky * 3 + kx][p] = wg[ky * K_WROW + (p * 3 + kx) * 128];
  }
  // per-channel epilogue parameters of the wave's role (channels g 32 + ct 16 + 4 q ..)
  const int ch_l = g * 32 + ct * 16 + 4 * q;
  f32x4 os, ob, rs = {1.0f, 1.0f, 1.0f, 1.0f};
  if (is_a) {  // mid = relu(acc os + ob): the folded BatchNorm, times the second convolution's range scale
    os = *reinterpret_cast<const f32x4*>(a.w_unscale + ch_l) * (a.act_unscale * b.act_scale);  // (powers of two: exact)
    if (a.out_scale) os *= *reinterpret_cast<const f32x4*>(a.out_scale + ch_l);
    ob = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (a.out_shift) ob = *reinterpret_cast<const f32x4*>(a.out_shift + ch_l) * b.act_scale;
  } else {
    rs = *reinterpret_cast<const f32x4*>(b.w_scale + ch_l) * b.act_scale;  // (the residual's scale: what the sums carry)
    os = *reinterpret_cast<const f32x4*>(b.w_unscale + ch_l) * b.act_unscale;
    ob = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (b.out_shift) ob = *reinterpret_cast<const f32x4*>(b.out_shift + ch_l);
  }

  // ---- tiles: every XCD walks its own contiguous eighth of the tiles or of the tile rows (cpx_conv_layout_core.h: walk_tile) ----
  // tile j of this workgroup -> (n, oy, ox); false: it has fewer
  auto get_tile = [&](int j, int& n_, int& oy_, int& ox_) {
    int ty, tx;
    if (!walk_tile(td, (int)blockIdx.x, (int)gridDim.x, j, n_, ty, tx)) return false;
    oy_ = ty * K_T;
    ox_ = tx * K_T;
    return true;
  };

  // ---- staging: item i of a thread = one 16-byte piece (4 channels) of patch pixel (tid >> 3) + 64 i, piece tid & 7 ----
  u32x4 pre_p[K_NP];
  const int q8 = tid & 7;
  int ipos[K_NP];  // patch row << 8 | column
#pragma unroll
  for (int i = 0; i < K_NP; ++i) {
    const int px = min((tid >> 3) + K_PPI * i, K_PNPX - 1);
    const int py = px / K_PP;
    ipos[i] = (py << 8) | (px - py * K_PP);
  }
  const unsigned st_base = (unsigned)((((q8 >> 2) * K_PNPXP + (tid >> 3)) * 4 + (q8 & 3)) * 8);
  f32x4 psc, psh;  // relu(x s + b) 2^k = relu(x (s 2^k) + b 2^k), exactly
  psc = *reinterpret_cast<const f32x4*>(a.in_scale + g * 32 + 4 * q8) * a.act_scale;
  psh = *reinterpret_cast<const f32x4*>(a.in_shift + g * 32 + 4 * q8) * a.act_scale;
  const unsigned coff0 = (unsigned)(g * 32 + 4 * q8);
  const int Hm1 = H - 1, Wm1 = W - 1;
  auto issue_item = [&](const int i, const int n_, const int oy_, const int ox_) __attribute__((always_inline)) {
    const float* in_n = a.in + (size_t)n_ * H * W * a.Cin;  // (uniform)
    const int iy = oy_ - 2 + (ipos[i] >> 8), ix = ox_ - 2 + (ipos[i] & 0xFF);
    const int cy = med3(iy, 0, Hm1), cx = med3(ix, 0, Wm1);  // a clamped address is always loaded; padding is zeroed at commit
    pre_p[i] = *reinterpret_cast<const u32x4*>(at_off(in_n, (pix_off(cy, cx, W, a.Cin) + coff0) << 2));
  };
  unsigned hmax = 0u;  // out of fp16's range = a high plane that came out infinite (every staged value is >= 0: ReLU)
  // a staged item's way into P has a register half and an LDS half.  convert: BatchNorm + ReLU prologue, zero padding, fp16
  // split; store: the two 8-byte LDS stores
  auto convert_item = [&](const int i, const int oy_, const int ox_) __attribute__((always_inline)) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(__fmaf_rn(__uint_as_float(pre_p[i][j]), psc[j], psh[j]), 0.0f);
    const int iy = oy_ - 2 + (ipos[i] >> 8), ix = ox_ - 2 + (ipos[i] & 0xFF);
    const bool inside = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;  // zero padding, as TensorFlow pads the activated tensor
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = inside ? v[j] : 0.0f;
    unsigned h0, h1, l0, l1;
    split_pair2_h(v[0], v[1], h0, l0);
    split_pair2_h(v[2], v[3], h1, l1);
    hmax = pk_max_u16(pk_max_u16(hmax, h0), h1);
    pre_p[i] = u32x4{h0, h1, l0, l1};  // (in place: the store follows at once)
  };
  auto store_item = [&](const int i) __attribute__((always_inline)) {
    if (i == K_NP - 1 && tid >= K_PNPX * 8 - (K_NP - 1) * K_CT) return;
    const u32x4 v = pre_p[i];
    unsigned char* sp = reinterpret_cast<unsigned char*>(s_P) + st_base;
    *reinterpret_cast<uint2*>(sp + i * (K_PPI * 32)) = make_uint2(v[0], v[1]);
    *reinterpret_cast<uint2*>(sp + 2 * K_PNPXP * 32 + i * (K_PPI * 32)) = make_uint2(v[2], v[3]);
  };

  // ---- accumulators (both roles use the same registers): A 9 mid rows + up to 2 edge groups, B 8 output rows ----
  f32x4 acc[11];
  constexpr int AHEAD = 3, RING = 4;

  // A: first convolution of the tile whose patch is in P.  Rows: mid rows 9 hh .. 9 hh + 8 (16 columns each) from patch rows
  // 9 hh .. 9 hh + 10; edge groups: mid columns 16, 17 of all 18 rows = 36 pixels in groups of 16 (e -> row e >> 1, column
  // 16 + (e & 1)); the half hh = 1 takes groups 0 and 1, hh = 0 the third (4 pixels).  `between(s)`: staging hooks, step s of 33 + 9
  // `carry`: mid columns 16 and 17 come from the previous tile's buffer (carry_load / carry_store) -- no edge groups
  auto conv_a = [&](const bool carry, auto&& between) __attribute__((always_inline)) {
    const uint4* pb = s_P + ((q >> 1) * K_PNPXP + (9 * hh) * K_PP + i16) * 2 + (q & 1);
#pragma unroll
    for (int o = 0; o < 11; ++o) acc[o] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 xh[RING], xl[RING];
    auto frag = [&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, kx = s / 11, i = s - 11 * kx, bf = s % RING;
      xh[bf] = __builtin_bit_cast(u32x4, pb[(i * K_PP + kx) * 2]);
      xl[bf] = __builtin_bit_cast(u32x4, pb[4 * K_PNPXP + (i * K_PP + kx) * 2]);
    };
    static_for<0, AHEAD>(frag);
    static_for<0, 33>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, kx = s / 11, i = s - 11 * kx, bf = s % RING;
      if constexpr (s + AHEAD < 33) frag(std::integral_constant<int, s + AHEAD>{});
      static_for<0, 3>([&](auto pc) __attribute__((always_inline)) {
        constexpr int pr = decltype(pc)::value;
        static_for<0, 3>([&](auto rc) __attribute__((always_inline)) {
          constexpr int r = decltype(rc)::value, o = i - r;
          if constexpr (o >= 0 && o < 9) {
            if constexpr (pr == 0) acc[o] = mfma16<true>(Wr[r * 3 + kx][1], xh[bf], acc[o]);
            if constexpr (pr == 1) acc[o] = mfma16<true>(Wr[r * 3 + kx][0], xl[bf], acc[o]);
            if constexpr (pr == 2) acc[o] = mfma16<true>(Wr[r * 3 + kx][0], xh[bf], acc[o]);
          }
        });
      });
      between(sc);
      __builtin_amdgcn_sched_barrier(0);  // (pins the fragment reads three steps ahead of their products: cpx_cnn_rw.hip)
    });
    if (carry) return;  // (uniform)
    // the edge groups: per-lane pixel, no reuse across taps.  (hh == 0: one group, 32 + i16; hh == 1: two)
    int eb[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = min((hh ? 16 * k : 32) + i16, 35);
      eb[k] = ((q >> 1) * K_PNPXP + (e >> 1) * K_PP + 16 + (e & 1)) * 2 + (q & 1);
    }
    static_for<0, 9>([&](auto tc) __attribute__((always_inline)) {
      constexpr int tp = decltype(tc)::value, kx = tp / 3, ky = tp - 3 * kx;  // (kx-major, as the rows)
      u32x4 eh[2], el[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k == 0 || hh) {  // (uniform)
          eh[k] = __builtin_bit_cast(u32x4, s_P[eb[k] + (ky * K_PP + kx) * 2]);
          el[k] = __builtin_bit_cast(u32x4, s_P[4 * K_PNPXP + eb[k] + (ky * K_PP + kx) * 2]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k == 0 || hh) {
          acc[9 + k] = mfma16<true>(Wr[ky * 3 + kx][1], eh[k], acc[9 + k]);
          acc[9 + k] = mfma16<true>(Wr[ky * 3 + kx][0], el[k], acc[9 + k]);
          acc[9 + k] = mfma16<true>(Wr[ky * 3 + kx][0], eh[k], acc[9 + k]);
        }
      }
      between(std::integral_constant<int, 33 + tp>{});
    });
  };
  // A, phase 2: mid = relu(acc os + ob) as the second convolution's fp16 planes in M[par]; pixels outside the image are
  // that convolution's zero padding.  (oy, ox): the tile's output origin; mid pixel (r, c) is image pixel (oy - 1 + r, ox - 1 + c)
  auto mid_put = [&](const int par, const int oy_, const int ox_, const f32x4 accv, const int mrow, const int mcol, const bool valid) __attribute__((always_inline)) {
    unsigned char* mb = reinterpret_cast<unsigned char*>(s_M + par * K_MBUF);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(__fmaf_rn(accv[j], os[j], ob[j]), 0.0f);
    const bool inside = (unsigned)(oy_ - 1 + mrow) < (unsigned)H && (unsigned)(ox_ - 1 + mcol) < (unsigned)W;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = inside ? v[j] : 0.0f;
    unsigned h0, h1, l0, l1;
    split_pair2_h(v[0], v[1], h0, l0);
    split_pair2_h(v[2], v[3], h1, l1);
    hmax = pk_max_u16(pk_max_u16(hmax, h0), h1);
    // channels ct 16 + 4 q .. of the 32: piece 4 ct + q -> quarter pair ct, 8-byte slot q of the pixel's 32 bytes
    const unsigned off = (unsigned)(((ct * K_MNPXP + mrow * K_MP + mcol) * 4 + q) * 8);
    if (valid) {
      *reinterpret_cast<uint2*>(mb + off) = make_uint2(h0, h1);
      *reinterpret_cast<uint2*>(mb + off + 2 * K_MNPXP * 32) = make_uint2(l0, l1);
    }
  };
  // (a mid row is complete once its last tap column has passed: row o after step 24 + o of the 33 -- its epilogue rides on the
  // steps behind that one, under the remaining products, instead of behind all of them)
  auto mid_row = [&](const int par, const int oy_, const int ox_, const int o) __attribute__((always_inline)) {
    mid_put(par, oy_, ox_, acc[o], 9 * hh + o, i16, true);
  };
  auto mid_edges = [&](const int par, const int oy_, const int ox_) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (k == 0 || hh) {
        const int e = (hh ? 16 * k : 32) + i16;
        mid_put(par, oy_, ox_, acc[9 + k], min(e, 35) >> 1, 16 + (e & 1), e < 36);
      }
    }
  };
  // A, carried tile: its mid columns 16 and 17 are image columns ox + 15 and ox + 16, mid columns 0 and 1 of the tile to its
  // right -- the same float32 sums of the same taps in the same order (kx-major with ky inside, planes w_lo x_hi, w_hi x_lo,
  // w_hi x_hi in conv_a's row loop and in its edge loop alike), range-checked into hmax when that tile computed them.  When
  // that tile is the one B works on, they lie in M[par ^ 1]: 18 rows x 2 columns x 2 planes x 2 quarter pairs x 32 B = 288
  // entries, one per A thread and a second one for the first 32; two columns of a row are four consecutive entries
  auto carry_idx = [&](const int e) { return (((e >> 2) / K_MP) * K_MNPXP + ((e >> 2) % K_MP) * K_MP) * 2 + (e & 3); };
  u32x4 cc[2];
  auto carry_load = [&](const int par) __attribute__((always_inline)) {
    const uint4* src = s_M + (par ^ 1) * K_MBUF;
    cc[0] = __builtin_bit_cast(u32x4, src[carry_idx(tid)]);
    if (tid < 32) cc[1] = __builtin_bit_cast(u32x4, src[carry_idx(256 + tid)]);
  };
  auto carry_store = [&](const int par) __attribute__((always_inline)) {
    uint4* dst = s_M + par * K_MBUF + K_T * 2;
    dst[carry_idx(tid)] = __builtin_bit_cast(uint4, cc[0]);
    if (tid < 32) dst[carry_idx(256 + tid)] = __builtin_bit_cast(uint4, cc[1]);
  };
  // B: second convolution of the tile whose mid is in M[par]: output rows 8 hh .. 8 hh + 7 from mid rows 8 hh .. 8 hh + 9
  auto conv_b = [&](const int par, auto&& between) __attribute__((always_inline)) {
    const uint4* mbp = s_M + par * K_MBUF + ((q >> 1) * K_MNPXP + (8 * hh) * K_MP + i16) * 2 + (q & 1);
    // the accumulators hold the tile's residual rows (requested at the end of the previous step: preload_res): they take the
    // scale of the sums, act_scale * w_scale[channel], and the products go on top -- no registers beside the accumulators
#pragma unroll
    for (int o = 0; o < 8; ++o) acc[o] = acc[o] * rs;
    u32x4 xh[RING], xl[RING];
    auto frag = [&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, kx = s / 10, i = s - 10 * kx, bf = s % RING;
      xh[bf] = __builtin_bit_cast(u32x4, mbp[(i * K_MP + kx) * 2]);
      xl[bf] = __builtin_bit_cast(u32x4, mbp[4 * K_MNPXP + (i * K_MP + kx) * 2]);
    };
    static_for<0, AHEAD>(frag);
    static_for<0, 30>([&](auto sc) __attribute__((always_inline)) {
      constexpr int s = decltype(sc)::value, kx = s / 10, i = s - 10 * kx, bf = s % RING;
      if constexpr (s + AHEAD < 30) frag(std::integral_constant<int, s + AHEAD>{});
      static_for<0, 3>([&](auto pc) __attribute__((always_inline)) {
        constexpr int pr = decltype(pc)::value;
        static_for<0, 3>([&](auto rc) __attribute__((always_inline)) {
          constexpr int r = decltype(rc)::value, o = i - r;
          if constexpr (o >= 0 && o < 8) {
            if constexpr (pr == 0) acc[o] = mfma16<true>(Wr[r * 3 + kx][1], xh[bf], acc[o]);
            if constexpr (pr == 1) acc[o] = mfma16<true>(Wr[r * 3 + kx][0], xl[bf], acc[o]);
            if constexpr (pr == 2) acc[o] = mfma16<true>(Wr[r * 3 + kx][0], xh[bf], acc[o]);
          }
        });
      });
      between(sc);
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  auto preload_res = [&](const int n_, const int oy_, const int ox_) __attribute__((always_inline)) {
    const float* res_n = b.residual + (size_t)n_ * H * W * C;  // (uniform)
    const int ox = min(ox_ + i16, Wm1);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      const int oy = min(oy_ + 8 * hh + o, Hm1);
      acc[o] = *reinterpret_cast<const f32x4*>(at_off(res_n, (pix_off(oy, ox, W, C) + (unsigned)ch_l) << 2));
    }
  };
  // B: out = relu(acc os + ob (+ residual)), one 16-byte store per row; a row is complete after step 22 + o of the 30
  auto out_row = [&](const int n_, const int oy_, const int ox_, const int o) __attribute__((always_inline)) {
    float* out_n = b.out + (size_t)n_ * H * W * C;
    const int ox = min(ox_ + i16, Wm1);
    const int oy = oy_ + 8 * hh + o;
    const unsigned off = (pix_off(min(oy, Hm1), ox, W, C) + (unsigned)ch_l) << 2;
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __fmaf_rn(acc[o][j], os[j], ob[j]);
    v.x = relu_bits(v.x); v.y = relu_bits(v.y); v.z = relu_bits(v.z); v.w = relu_bits(v.w);
    if (ox_ + i16 < W && oy < H) *reinterpret_cast<f32x4*>(at_off(out_n, off)) = v;
  };

  // ---- the pipeline.  Step k: A on tile k + 1, B on tile k; the staging requests tile k + 2 in phase 1, converts and stores
  //      it in phase 2; k = -1 fills it ----
  int n0 = 0, oy0 = 0, ox0 = 0, n1 = 0, oy1 = 0, ox1 = 0, n2 = 0, oy2 = 0, ox2 = 0;
  bool v0 = false;                               // tile k     (B)
  bool v1 = get_tile(0, n1, oy1, ox1);           // tile k + 1 (A)
  if (!v1) return;                               // (the whole workgroup: no tile at all)
  bool v2 = get_tile(1, n2, oy2, ox2);           // tile k + 2 (converted, stored)
  // the first tile's patch goes through the registers with nothing beside it; the second one's requests follow
#pragma unroll
  for (int i = 0; i < K_NP; ++i) issue_item(i, n1, oy1, ox1);
#pragma unroll
  for (int i = 0; i < K_NP; ++i) {
    convert_item(i, oy1, ox1);
    store_item(i);
  }
  __syncthreads();
  for (int k = -1;; ++k) {
    // ---- phase 1: products, and each role's own epilogue right behind them (A writes M[(k + 1) & 1] while B still reads
    //      M[k & 1]; B's stores touch no LDS): vector work under the other role's products ----
    // a tile that does not exist is replaced by the last one that does (its requests and planes are never stored)
    const int oyc = v2 ? oy2 : oy1, oxc = v2 ? ox2 : ox1;
    auto stage = [&](const int i) __attribute__((always_inline)) {  // (the request of tile k + 2; its conversion and store follow in phase 2)
      issue_item(i, v2 ? n2 : n1, oyc, oxc);
    };
    if (is_a) {
      if (v1) {
        // tile k + 1 is the left neighbour of tile k: decided from the coordinates alone, whatever the walk (k = -1, a run's
        // first tile and a tile whose right neighbour was another workgroup's compute their own columns)
        const bool carry = carry_on && v0 && n0 == n1 && oy0 == oy1 && ox1 + K_T == ox0;  // (uniform)
        conv_a(carry, [&](auto sc) __attribute__((always_inline)) {
          constexpr int s = decltype(sc)::value;
          if constexpr (s % 5 == 2 && s / 5 < K_NP) stage(s / 5);
          // (the carried columns' LDS reads three steps ahead of their stores, as the fragments: no wait beside the products)
          if constexpr (s == 24) {
            if (carry) carry_load((k + 1) & 1);
          }
          if constexpr (s == 27) {
            if (carry) carry_store((k + 1) & 1);
          }
          if constexpr (s >= 25 && s <= 32) mid_row((k + 1) & 1, oy1, ox1, s - 25);  // (one step behind the row's last product)
        });
        mid_row((k + 1) & 1, oy1, ox1, 8);
        if (!carry) mid_edges((k + 1) & 1, oy1, ox1);
      } else {
#pragma unroll
        for (int i = 0; i < K_NP; ++i) stage(i);
      }
    } else {
      if (v0) {
        conv_b(k & 1, [&](auto sc) __attribute__((always_inline)) {
          constexpr int s = decltype(sc)::value;
          if constexpr (s % 4 == 1 && s / 4 < K_NP) stage(s / 4);
          if constexpr (s >= 23 && s <= 29) out_row(n0, oy0, ox0, s - 23);
        });
        out_row(n0, oy0, ox0, 7);
      } else {
#pragma unroll
        for (int i = 0; i < K_NP; ++i) stage(i);
      }
      // the NEXT tile's residual rows (= the block's input at its output pixels) into the accumulators, now free: in flight
      // across the barriers and phase 2
      if (v1) preload_res(n1, oy1, ox1);
    }
    __syncthreads();
    // ---- phase 2: tile k + 2's planes -> P (free: A has read tile k + 1's) ----
    if (v2) {  // (uniform)
#pragma unroll
      for (int i = 0; i < K_NP; ++i) {
        if (is_a) {  // (one copy per role, as the kernel was measured: merged, the two compile to different code)
          convert_item(i, oy2, ox2);
          store_item(i);
        } else {
          convert_item(i, oy2, ox2);
          store_item(i);
        }
      }
    }
    if (!v1) break;  // (uniform) tile k was the workgroup's last
    __syncthreads();
    n0 = n1; oy0 = oy1; ox0 = ox1; v0 = v1;
    n1 = n2; oy1 = oy2; ox1 = ox2; v1 = v2;
    v2 = v1 && get_tile(k + 3, n2, oy2, ox2);  // (the next step is k + 1: its staging tile is k + 3)
  }
  if ((hmax & 0xFFFFu) >= 0x7C00u || (hmax >> 16) >= 0x7C00u) atomicOr(a.ovf, 1);  // (infinity or NaN: out of fp16's range)
}


}  // namespace

// `a` / `b`: the block's two convolutions as launch_conv_block32 has prepared them (w_scale / w_unscale set); wa / wb: their
// fp16 plane images ([g][ky][plane][kx][quarter][32])
int launch_conv_block32s(const ConvArgs& a, const ConvArgs& b, const void* wa, const void* wb, hipStream_t s) {
  BlkTiles td{};
  if (const int rc = fill_tiles(td, (a.W + K_T - 1) / K_T, (a.H + K_T - 1) / K_T, a.N, TILES_PERSISTENT)) return rc;
  static bool lds_ready[64];
  if (!cpx_dyn_lds_ready(reinterpret_cast<const void*>(conv_block32s_kernel), lds_ready, 160 * 1024 - 1024)) return -1;
  const int gx = persistent_grid(cpx_device_cus(), a.groups, td.total, "CPX_BLOCK32_GRID");
  if (gx < 0) return -1;
  // CPX_BLOCK32_CARRY=0: every tile computes its own halo columns; CPX_BLOCK32_WALK=0 | 1: the tile-interleaved walk or the
  // row runs whatever choose_walk says (both read at every launch, as the grid: for the bitwise tests and the timing)
  const char* ec = std::getenv("CPX_BLOCK32_CARRY");
  const char* ew = std::getenv("CPX_BLOCK32_WALK");
  set_walk(td, ew ? (std::atoi(ew) ? WALK_ROWS : WALK_TILES) : choose_walk(td, gx));
  hipLaunchKernelGGL(conv_block32s_kernel, dim3((unsigned)gx, a.groups), dim3(K_CT), K_LDS, s, a, b, reinterpret_cast<const uint4*>(wa),
                     reinterpret_cast<const uint4*>(wb), td, ec ? (std::atoi(ec) != 0) : 1);
  return 0;
}

}  // namespace cpx
