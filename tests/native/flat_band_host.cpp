// flat_band_host.cpp -- classifier-pipeline_amd/csrc/cpx_flat_band_core.h compiled for the host: the geometry of a flattened
// band as the kernels and flat_pays's capacity test use it, behind a C interface for tests/test_flat_band_host.py, and (with
// -DFLAT_BAND_HOST_MAIN) as a program of its own that sweeps every map the capacity admits, for the sanitizer build.
#include <cstdio>
#include <vector>

#include "cpx_flat_band_core.h"

using namespace cpx;

extern "C" {

int flat_bands_host(int band, int Ho, int Wo) { return flat_bands(band, Ho, Wo); }
int flat_band_max_pixels_host(int band, int Wo) { return flat_band_max_pixels(band, Wo); }
// out: p0, y_first, y_last, PW, PH, npx
void flat_band_host(int ti, int band, int Ho, int Wo, int* out) {
  const FlatBand b = flat_band(ti, band, Ho, Wo);
  out[0] = b.p0; out[1] = b.y_first; out[2] = b.y_last; out[3] = b.PW; out[4] = b.PH; out[5] = b.npx;
}
void flat_item_pixel_host(int ti, int band, int Ho, int Wo, int px, int* iy, int* ix) {
  flat_item_pixel(flat_band(ti, band, Ho, Wo), px, *iy, *ix);
}
int flat_patch_offset_host(int ti, int band, int Ho, int Wo, int p, int ky, int kx) {
  return flat_patch_offset(flat_band(ti, band, Ho, Wo), p, Ho * Wo, Wo, ky, kx);
}

// Every band of an H x W map (stride 1, SAME: Ho = H, Wo = W) against a patch buffer of `cap` pixels.  0: all hold; else
// the first property that failed:
//   1  a band stages more than `cap` pixels, or more than flat_band_max_pixels says any band can
//   2  a (position, tap) offset lies outside the staged pixels -- positions of the band past the map's last included (the
//      kernel forms their addresses; they are clamped)
//   3  the pixel at a (position, tap) offset is not the input pixel (y - 1 + ky, x - 1 + kx) the convolution reads
//   4  in a band with all its positions inside the map: a staged pixel that no position reads lies elsewhere than in the full-width staging's two known surplus
//      runs: the first staged row left of the first position's window, the last staged row right of the last position's
//   5  the bands do not tile the positions
int flat_sweep_host(int H, int W, int band, int cap) {
  const int M = H * W, nb = flat_bands(band, H, W);
  if (flat_band_max_pixels(band, W) > cap) return 1;
  int covered = 0;
  std::vector<char> read;
  for (int ti = 0; ti < nb; ++ti) {
    const FlatBand b = flat_band(ti, band, H, W);
    if (b.p0 != covered) return 5;
    const int plast = (b.p0 + band < M ? b.p0 + band : M) - 1;
    covered = plast + 1;
    if (b.npx > cap || b.npx > flat_band_max_pixels(band, W) || b.npx != b.PH * b.PW || b.npx < 1) return 1;
    read.assign((size_t)b.npx, 0);
    for (int p = b.p0; p < b.p0 + band; ++p) {
      const int pc = p < M ? p : M - 1, y = pc / W, x = pc % W;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const int off = flat_patch_offset(b, p, M, W, ky, kx);
          if (off < 0 || off >= b.npx) return 2;
          if (off != flat_patch_base(b, p, M, W) + flat_tap_offset(b, ky, kx)) return 3;
          int iy, ix;
          flat_item_pixel(b, off, iy, ix);
          if (iy != y - 1 + ky || ix != x - 1 + kx) return 3;
          read[(size_t)off] = 1;
        }
    }
    const int x_first = b.p0 % W, x_last = plast % W;
    if (b.p0 + band > M) continue;  // (a ragged last band may end inside its first row: more of its full rows go unread)
    for (int px = 0; px < b.npx; ++px) {
      if (read[(size_t)px]) continue;
      int iy, ix;
      flat_item_pixel(b, px, iy, ix);
      const bool before = iy == b.y_first - 1 && ix < x_first - 1, after = iy == b.y_last + 1 && ix > x_last + 1;
      if (!before && !after) return 4;
    }
  }
  return covered == M ? 0 : 5;
}

}  // extern "C"

#ifdef FLAT_BAND_HOST_MAIN
int main() {
  int maps = 0;
  for (int W = 1; W <= 64; ++W)
    for (int H = 1; H <= 64; ++H) {
      if (flat_band_max_pixels(128, W) > 256) continue;
      if (const int rc = flat_sweep_host(H, W, 128, 256)) {
        std::fprintf(stderr, "flat_band sweep: %d x %d fails property %d\n", H, W, rc);
        return 1;
      }
      ++maps;
    }
  if (maps == 0) return 1;
  // a map the capacity does not admit is refused, not swept
  if (flat_sweep_host(54, 54, 128, 256) != 1) return 1;
  return 0;
}
#endif
