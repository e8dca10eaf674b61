// TEST INFRASTRUCTURE ONLY: host build of classifier-pipeline_amd/csrc/cpx_graph_core.h and of the host part of
// cpx_graph_conv_core.h (tests/test_graph_core_host.py),
// with -ffp-contract=off as the product.  As a shared object it hands the hybrid arithmetic (over arrays) and the index
// maps of the graph executor's kernels to Python; with -DGRAPH_CORE_HOST_MAIN it is a program of its own that walks the
// same ground, for a sanitizer build.  The product never loads either.
#include <stdint.h>
#include <stdio.h>

#include "cpx_graph_conv_core.h"

namespace {
constexpr int RUN = 4;  // cpx_graph_dw.hip's GRAPH_DW_RUN
struct View {           // the fields of GraphView that quads and conv_geom read
  const float* p;
  int C, cstride;
  size_t sample_stride;
  int H, W;
};
}  // namespace

extern "C" void quantise_host(const float* x, const float* inv, int zp, int n, int* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::quantise(x[i], inv[i], zp);
}

extern "C" void quant_params_host(const float* lo, const float* hi, int symmetric, int n, float* sx, float* inv, int* zp) {
  for (int i = 0; i < n; ++i) {
    const cpx::QuantParams p = cpx::quant_params(lo[i], hi[i], symmetric != 0);
    sx[i] = p.sx, inv[i] = p.inv, zp[i] = p.zp;
  }
}

extern "C" void hybrid_finish_host(const int* acc, const int* zp, const int* wsum, const float* sx, const float* scale,
                                   const float* shift, int act, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::hybrid_finish(acc[i], zp[i], wsum[i], sx[i], scale[i], shift[i], act);
}

extern "C" int quads_host(int C, int cstride, unsigned long long sample_stride, unsigned long long address) {
  return cpx::quads(View{reinterpret_cast<const float*>((uintptr_t)address), C, cstride, (size_t)sample_stride, 1, 1});
}

// out: n, oy, ox, valid
extern "C" void conv_pixel_host(long long p, long long P, int HoWo, int Wo, long long* out) {
  const cpx::ConvPixel c = cpx::conv_pixel(p, P, HoWo, Wo);
  out[0] = c.n, out[1] = c.oy, out[2] = c.ox, out[3] = c.valid;
}
extern "C" int window_origin_host(int o, int stride, int pad) { return cpx::window_origin(o, stride, pad); }
extern "C" int acc_row_host(int r, int lane) { return cpx::acc_row(r, lane); }
// out: n, rem
extern "C" void sample_step_host(long long n, int rem, int HoWo, long long* out) {
  const cpx::SamplePixel s = cpx::sample_step(n, rem, HoWo);
  out[0] = s.n, out[1] = s.rem;
}

// the geometry of a convolution's launch over dense views at `address`; bytes: the int8 path's 16-byte test, else the
// float32 one.  out: P, HoWo, nchunks, ntiles, vec, cg, cog, G
extern "C" void conv_geom_host(int N, int Ho, int Wo, int Cin, int Cout, int kc, int G, int bytes, unsigned long long address,
                               long long* out) {
  const float* p = reinterpret_cast<const float*>((uintptr_t)address);
  const View in{p, Cin, Cin, (size_t)Cin * 49, 7, 7}, y{p, Cout, Cout, (size_t)Cout * Ho * Wo, Ho, Wo};
  const cpx::ConvGeom g = bytes ? cpx::conv_geom(N, in, y, kc, G, cpx::group_bytes16<View>) : cpx::conv_geom(N, in, y, kc, G, cpx::group_quads<View>);
  out[0] = g.P, out[1] = g.HoWo, out[2] = g.nchunks, out[3] = g.ntiles, out[4] = g.vec, out[5] = g.cg, out[6] = g.cog, out[7] = g.G;
}
// out: tap, c0, ky, kx
extern "C" void conv_step_host(int s, int nchunks, int kw, int kc, int* out) {
  const cpx::ConvStep k = cpx::conv_step(s, nchunks, kw, kc);
  out[0] = k.tap, out[1] = k.c0, out[2] = k.ky, out[3] = k.kx;
}
// what conv_dispatch_ntn hands its launch: out = NTN, grid rows
extern "C" void conv_tiling_host(int ntiles, int* out) {
  cpx::conv_dispatch_ntn(ntiles, [&](auto ntn, int rows) { out[0] = decltype(ntn)::value, out[1] = rows; });
}

// `items` below 2^32 takes the 32-bit divisions, from 2^32 on the 64-bit ones (whatever idx is).  out: n, oy, ox0, c.
// Returns 0 where idx is beyond the last item.
extern "C" int dw_item_host(unsigned long long idx, unsigned long long items, int groups, int runs, int Ho,
                            unsigned long long* out) {
  cpx::DwItem it{};
  if (!cpx::dw_item<RUN>((size_t)idx, cpx::DwGeom{(size_t)items, groups, runs}, Ho, &it)) return 0;
  out[0] = it.n, out[1] = (unsigned long long)it.oy, out[2] = (unsigned long long)it.ox0, out[3] = (unsigned long long)it.c;
  return 1;
}

#ifdef GRAPH_CORE_HOST_MAIN
namespace {
int failures = 0;
#define EXPECT(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
      ++failures;                                        \
    }                                                    \
  } while (0)
}  // namespace

int main() {
  {  // ties round away from zero, both clamps, the degenerate parameters
    const float x[] = {0.5f, -0.5f, 1.5f, -2.5f, 126.5f, 127.5f, -128.5f, 1000.0f, -1000.0f, 0.0f, -0.0f};
    const int want[] = {1, -1, 2, -3, 127, 127, -128, 127, -128, 0, 0};
    for (int i = 0; i < 11; ++i) EXPECT(cpx::quantise(x[i], 1.0f, 0) == want[i]);
    EXPECT(cpx::quantise(0.0f, 1.0f, -128) == -128 && cpx::quantise(1.0f, 300.0f, 127) == 127);
    cpx::QuantParams p = cpx::quant_params(0.0f, 0.0f, false);
    EXPECT(p.sx == 1.0f && p.inv == 1.0f && p.zp == 0);
    p = cpx::quant_params(0.0f, 0.0f, true);
    EXPECT(p.sx == 1.0f && p.inv == 1.0f && p.zp == 0);
    p = cpx::quant_params(0.0f, 255.0f, false);
    EXPECT(p.sx == 1.0f && p.inv == 1.0f && p.zp == -128);
    p = cpx::quant_params(-255.0f, 0.0f, false);
    EXPECT(p.zp == 127);
    p = cpx::quant_params(-127.0f, 128.0f, false);  // equal costs: the second candidate
    EXPECT(p.zp == -1);
    p = cpx::quant_params(-3e38f, 3e38f, false);
    EXPECT(p.zp == -1 || p.zp == 0);
    p = cpx::quant_params(-2.0f, 1.0f, true);
    EXPECT(p.zp == 0 && p.sx == (float)(2.0 / 127.0));
  }
  {  // the finish: the int-to-float rounding at 2^24 + 1, the largest sum the planner lets through
    EXPECT(cpx::hybrid_finish(16777217, 0, 0, 1.0f, 1.0f, 0.0f, CPX_GRAPH_ACT_NONE) == 16777216.0f);
    const int k = 66310;  // k * 127 * 255 < 2^31
    EXPECT(cpx::hybrid_finish(k * 127 * 127, -128, k * 127, 1.0f, 1.0f, 0.0f, CPX_GRAPH_ACT_NONE) == (float)(k * 127 * 255));
    EXPECT(cpx::hybrid_finish(-5, 0, 0, 1.0f, 1.0f, 0.0f, CPX_GRAPH_ACT_RELU) == 0.0f);
    EXPECT(cpx::hybrid_finish(50, 1, 2, 0.5f, 0.5f, 1.0f, CPX_GRAPH_ACT_RELU6) == 6.0f);
  }
  {  // the pixel walks against / and %, HoWo = 1 included
    const int howo[] = {1, 3, 64, 289}, wo[] = {1, 3, 8, 17};
    for (int k = 0; k < 4; ++k) {
      const long long P = 5ll * howo[k] + (howo[k] > 1);
      for (long long p = 0; p < (P + 127) / 128 * 128; ++p) {
        const cpx::ConvPixel c = cpx::conv_pixel(p, P, howo[k], wo[k]);
        if (p < P)
          EXPECT(c.valid && c.n == p / howo[k] && c.oy == (int)(p % howo[k]) / wo[k] && c.ox == (int)(p % howo[k]) % wo[k]);
        else
          EXPECT(!c.valid && c.n == 0 && c.oy == 0 && c.ox == 0);
      }
      for (long long pb = 0; pb < P; pb += 32)
        for (int i = 0; i < 32; ++i) {
          const cpx::SamplePixel s = cpx::sample_step(pb / howo[k], (int)(pb % howo[k]) + i, howo[k]);
          EXPECT(s.n == (pb + i) / howo[k] && s.rem == (int)((pb + i) % howo[k]));
        }
    }
    unsigned seen = 0;
    for (int r = 0; r < 16; ++r)
      for (int lane = 0; lane < 64; lane += 32) seen |= 1u << cpx::acc_row(r, lane);
    EXPECT(cpx::acc_row(5, 255) == cpx::acc_row(5, 63) && cpx::acc_row(5, 192) == cpx::acc_row(5, 0));
    EXPECT(seen == 0xffffffffu);
  }
  {  // the convolutions' launch geometry, K steps and tiles
    long long g[8];
    conv_geom_host(3, 5, 4, 33, 65, 32, 1, 0, 4096, g);
    EXPECT(g[0] == 60 && g[1] == 20 && g[2] == 2 && g[3] == 3 && g[4] == 0 && g[5] == 33 && g[6] == 65 && g[7] == 1);
    conv_geom_host(1, 1, 1, 48, 96, 16, 3, 1, 4096, g);
    EXPECT(g[2] == 1 && g[3] == 1 && g[4] == 1 && g[5] == 16 && g[6] == 32 && g[7] == 3);
    int k[4], n[2];
    for (int s = 0; s < 3 * 7 * 5; ++s) {
      conv_step_host(s, 5, 7, 16, k);
      EXPECT(k[0] == s / 5 && k[1] == 16 * (s % 5) && k[2] == s / 35 && k[3] == s / 5 % 7);
    }
    const int tiles[] = {1, 2, 3, 4, 5, 9}, ntn[] = {1, 2, 4, 4, 4, 4}, rows[] = {1, 1, 1, 1, 2, 3};
    for (int i = 0; i < 6; ++i) {
      conv_tiling_host(tiles[i], n);
      EXPECT(n[0] == ntn[i] && n[1] == rows[i]);
    }
  }
  {  // the depthwise item: both paths below 2^32, the 64-bit one above
    unsigned long long a[4], b[4];
    const unsigned long long items = 7ull * 9 * 3 * 5;
    for (unsigned long long idx = 0; idx < items; ++idx) {
      EXPECT(dw_item_host(idx, items, 5, 3, 9, a) && dw_item_host(idx, items + (1ull << 32), 5, 3, 9, b));
      for (int i = 0; i < 4; ++i) EXPECT(a[i] == b[i]);
      EXPECT(a[3] == 4 * (idx % 5) && a[2] == RUN * (idx / 5 % 3) && a[1] == idx / 15 % 9 && a[0] == idx / 135);
    }
    EXPECT(!dw_item_host(items, items, 5, 3, 9, a));
    const unsigned long long big = (1ull << 33) + 12345, bitems = 1ull << 34;
    EXPECT(dw_item_host(big, bitems, 48, 28, 112, a));
    EXPECT(a[3] == 4 * (big % 48) && a[2] == RUN * (big / 48 % 28) && a[1] == big / (48 * 28) % 112 && a[0] == big / (48ull * 28 * 112));
  }
  alignas(16) float buf[8];
  EXPECT(cpx::quads(View{buf, 8, 8, 64, 1, 1}) && !cpx::quads(View{buf + 1, 8, 8, 64, 1, 1}) && !cpx::quads(View{buf, 6, 8, 64, 1, 1}) &&
         !cpx::quads(View{buf, 8, 10, 64, 1, 1}) && !cpx::quads(View{buf, 8, 8, 66, 1, 1}));
  return failures ? 1 : 0;
}
#endif
