// cpx_flat_band_core.h -- the geometry of a flattened band, stated once (host + device).  The flattened 3 x 3 stride-1 SAME
// kernels (conv_bf3flat_kernel's capacity test in cpx_cnn_bf3.hip, conv_flat16_kernel in cpx_cnn_flat.hip) give a workgroup
// `band` CONSECUTIVE output positions of a sample in row-major order and stage the input rows these touch at full width with
// one halo row / column on every side.  Here: which rows a band covers, how many pixels it stages, which pixel a staging item
// is, and where the operand of (position, tap) lies among the staged pixels.  Plain C++ without HIP, so that a test compiles
// it on its own (tests/native/flat_band_host.cpp).
#pragma once

namespace cpx {

#if defined(__HIPCC__)
#define CPX_FLAT_HD __host__ __device__ __forceinline__
#else
#define CPX_FLAT_HD inline
#endif

// band `ti` of a map of Ho x Wo = M output positions (W == Wo: stride 1, SAME)
struct FlatBand {
  int p0;               // first position
  int y_first, y_last;  // output rows of its first and last position (the last clamped to the map's last position)
  int PW, PH;           // staged patch: full rows with a halo column each side, rows y_first - 1 .. y_last + 1
  int npx;              // staged pixels = PH * PW
};
CPX_FLAT_HD FlatBand flat_band(int ti, int band, int Ho, int Wo) {
  const int M = Ho * Wo;
  FlatBand b;
  b.p0 = ti * band;
  const int plast = b.p0 + band - 1 < M - 1 ? b.p0 + band - 1 : M - 1;
  b.y_first = b.p0 / Wo;
  b.y_last = plast / Wo;
  b.PW = Wo + 2;
  b.PH = b.y_last - b.y_first + 3;
  b.npx = b.PH * b.PW;
  return b;
}
CPX_FLAT_HD int flat_bands(int band, int Ho, int Wo) { return (Ho * Wo + band - 1) / band; }
// the most pixels any band of `band` positions can stage on rows Wo wide (a band that starts on a row's last position
// spans the most rows): what must fit the kernel's LDS capacity
CPX_FLAT_HD int flat_band_max_pixels(int band, int Wo) {
  const int rows = (band - 1 + Wo - 1) / Wo + 1;
  return (rows + 2) * (Wo + 2);
}
// staged pixel `px` (0 .. npx - 1, row-major in the patch) -> its input row and column; outside [0, H) x [0, W): padding
CPX_FLAT_HD void flat_item_pixel(const FlatBand& b, int px, int& iy, int& ix) {
  const int py = px / b.PW;
  iy = b.y_first - 1 + py;
  ix = px - py * b.PW - 1;
}
// the staged pixel that position p (any p >= b.p0 of the band; positions past the map's last are clamped to it: their
// products are computed and never stored) multiplies with tap (ky, kx): input (y - 1 + ky, x - 1 + kx).  The sum of a
// position's part and a tap's part, which a kernel forms once per lane and once per tap
CPX_FLAT_HD int flat_patch_base(const FlatBand& b, int p, int M, int Wo) {
  const int pc = p < M - 1 ? p : M - 1;
  const int y = pc / Wo, x = pc - y * Wo;
  return (y - b.y_first) * b.PW + x;
}
CPX_FLAT_HD int flat_tap_offset(const FlatBand& b, int ky, int kx) { return ky * b.PW + kx; }
CPX_FLAT_HD int flat_patch_offset(const FlatBand& b, int p, int M, int Wo, int ky, int kx) {
  return flat_patch_base(b, p, M, Wo) + flat_tap_offset(b, ky, kx);
}

}  // namespace cpx
