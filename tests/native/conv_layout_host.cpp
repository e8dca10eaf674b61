// TEST INFRASTRUCTURE ONLY: host build of classifier-pipeline_amd/csrc/cpx_conv_layout_core.h (tests/test_conv_layout_host.py).
// As a shared object it hands a layer's class and weight-image layout, the tile filler and the persistent grid width to
// Python; with -DCONV_LAYOUT_HOST_MAIN it is a program of its own that walks the same ground, for a sanitizer build.
// The product never loads either.
#include <stdint.h>
#include <stdio.h>

#include "cpx_conv_layout_core.h"

namespace {
struct Layer {  // the fields of ConvArgs that conv_shape_of reads
  int Cin, Cout, groups, ksize, stride;
};
struct SplitTiles {  // TileDiv's fields (cpx_cnn_bf3.hip): cpx::Tiles's and the column split, in that struct's order
  unsigned long long m_nsplit, m_tx, m_ty;
  int nsplit, tiles_x, tiles_y, total;
};
}  // namespace

// out: class (ConvClass's order), chunk, planes3, planes2, half, scales, rw_half, bytes; -1 = absent.  Returns conv_rw_kind.
extern "C" int conv_layout_host(int Cin, int Cout, int groups, int ksize, int stride, int64_t* out) {
  const cpx::ConvShape s = cpx::conv_shape_of(Layer{Cin, Cout, groups, ksize, stride});
  const cpx::WeightImages l = cpx::WeightImages::of(s);
  const size_t v[6] = {l.planes3, l.planes2, l.half, l.scales, l.rw_half, l.bytes};
  out[0] = (int64_t)l.cls;
  out[1] = l.chunk;
  for (int i = 0; i < 6; ++i) out[2 + i] = v[i] == cpx::WeightImages::absent ? -1 : (int64_t)v[i];
  return cpx::conv_rw_kind_of(s);
}

// persistent = 0: the limit of the one-unit-per-workgroup launches, 1: of the persistent ones.  nsplit = 0: the form without
// a column split.  out: m_nsplit, m_tx, m_ty, nsplit, tiles_x, tiles_y, total.
extern "C" int tile_fill_host(int tiles_x, int tiles_y, long long n, int nsplit, int persistent, uint64_t* out) {
  SplitTiles td{};
  const long long limit = persistent ? cpx::TILES_PERSISTENT : cpx::TILES_PER_LAUNCH;
  int rc;
  if (nsplit) {
    rc = cpx::fill_tiles(td, tiles_x, tiles_y, n, nsplit, limit);
  } else {  // the struct the kernels without a column split take
    cpx::Tiles t{};
    rc = cpx::fill_tiles(t, tiles_x, tiles_y, n, limit);
    td.m_tx = t.m_tx, td.m_ty = t.m_ty, td.tiles_x = t.tiles_x, td.tiles_y = t.tiles_y, td.total = t.total;
  }
  const uint64_t v[7] = {td.m_nsplit, td.m_tx, td.m_ty, (uint64_t)td.nsplit, (uint64_t)td.tiles_x, (uint64_t)td.tiles_y, (uint64_t)td.total};
  for (int i = 0; i < 7; ++i) out[i] = v[i];
  return rc;
}

extern "C" uint64_t tile_magic_host(int d) { return cpx::tile_magic(d); }
extern "C" int tile_div_host(int n, int d) { return cpx::tile_div(n, cpx::tile_magic(d)); }  // the kernels' n / d
extern "C" int persistent_grid_host(int cus, int ny, long long tiles, const char* width_env) {
  return cpx::persistent_grid(cus, ny, tiles, width_env);
}
extern "C" int persistent_grid_x_host(int cus, int ny, long long tiles) { return cpx::persistent_grid_x(cus, ny, tiles); }

#ifdef CONV_LAYOUT_HOST_MAIN
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
  {  // every shape of a sweep: images in order, 16-byte aligned, back to back up to `bytes`
    const int chans[] = {1, 8, 16, 24, 32, 48, 64, 128, 256};
    for (int groups = 1; groups <= 4; ++groups)
      for (int ci : chans)
        for (int co : chans)
          for (int stride = 1; stride <= 3; ++stride)
            for (int ksize : {1, 3, 5}) {
              int64_t o[8];
              const int kind = conv_layout_host(ci * groups, co * groups, groups, ksize, stride, o);
              int64_t end = 0;
              for (int i = 2; i < 7; ++i) {
                if (o[i] < 0) continue;
                EXPECT(o[i] % 16 == 0 && o[i] >= end && o[i] < o[7]);
                end = o[i] + 1;
              }
              EXPECT((o[0] == 0) == (o[7] == 0));
              EXPECT(kind >= 0 && kind <= 3 && (ksize == 3 || o[0] == 0));
            }
    int64_t o[8];
    EXPECT(conv_layout_host(128, 256, 2, 3, 3, o) == 3 && o[4] == 0 && o[5] == 589824 && o[7] == 591872);
    EXPECT(conv_layout_host(17, 64, 2, 3, 1, o) == 0 && o[0] == 0);  // channels that do not divide into the groups
    EXPECT(conv_layout_host(16, 64, 0, 3, 1, o) == 0 && o[0] == 0);
  }
  {  // the multipliers divide exactly up to the range's edge
    const int ds[] = {1, 2, 3, 7, 8, 4095};
    for (int d : ds) {
      const unsigned long long m = tile_magic_host(d);
      const unsigned long long ns[] = {0, (unsigned long long)d - 1, (unsigned long long)d, (unsigned long long)d + 1,
                                       1000ull * d - 1, 1000ull * d, (1ull << 22) - 1};
      for (unsigned long long n : ns)
        if (n < (1ull << 22)) EXPECT(((n * m) >> 42) == n / d && (unsigned long long)tile_div_host((int)n, d) == n / d);
    }
    EXPECT(tile_div_host((1 << 22) - 9, 4095) == ((1 << 22) - 9) / 4095 && tile_div_host((1 << 22) - 1, 4095) == ((1 << 22) - 1) / 4095);
  }
  {  // the range errors
    uint64_t o[7];
    EXPECT(tile_fill_host(2048, 2048, 1, 0, 0, o) == -3 && tile_fill_host(1024, 2047, 1, 2, 0, o) == 0 && o[6] == 1024u * 2047u * 2u);
    EXPECT(tile_fill_host(4096, 1, 1, 1, 0, o) == -3 && tile_fill_host(1, 4096, 1, 0, 1, o) == -3 && tile_fill_host(4095, 1, 1, 1, 0, o) == 0);
    EXPECT(tile_fill_host(0, 1, 1, 1, 0, o) == -3 && tile_fill_host(1, 1, 1ll << 40, 0, 0, o) == -3);
    EXPECT(tile_fill_host(1, 1, (1 << 22) - 8, 0, 1, o) == -3 && tile_fill_host(1, 1, (1 << 22) - 9, 0, 1, o) == 0);
  }
  EXPECT(persistent_grid_x_host(256, 2, 1 << 20) == 128 && persistent_grid_x_host(256, 64, 1 << 20) == 8 &&
         persistent_grid_x_host(256, 2, 9) == 16 && persistent_grid_x_host(256, 0, 0) == 0);
  EXPECT(persistent_grid_host(256, 2, 1 << 20, nullptr) == 128 && persistent_grid_host(0, 2, 1 << 20, nullptr) == -1 &&
         persistent_grid_host(256, 2, 1 << 20, "CPX_TEST_NO_SUCH_VARIABLE") == 128);
  return failures ? 1 : 0;
}
#endif
