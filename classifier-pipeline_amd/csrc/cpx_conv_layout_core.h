// cpx_conv_layout_core.h -- what the split-operand convolution launchers know about a layer on the host: which class of
// layer it is, the ONE layout of its weight-image buffer, the tile decomposition the kernels divide by, and the width of a
// persistent grid, and the order in which conv_block32s_kernel's workgroups walk the tiles (host + device: the one function
// the kernel calls).  Plain host C++ without HIP, so that tests compile it on its own (tests/native/conv_layout_host.cpp,
// block_walk_host.cpp);
// cpx_cnn_bf3.hip, cpx_cnn_rw.hip and cpx_cnn_blk.hip are its users in the product.
#pragma once
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

namespace cpx {

// a grouped convolution by shape alone (channels per group); ksize = 0: no shape (groups < 1 or channels not divisible)
struct ConvShape { int groups, cin_g, cout_g, ksize, stride; };
template <class Args>
ConvShape conv_shape_of(const Args& a) {
  if (a.groups < 1 || a.Cin % a.groups || a.Cout % a.groups) return ConvShape{};
  return ConvShape{a.groups, a.Cin / a.groups, a.Cout / a.groups, a.ksize, a.stride};
}

// The classes of layer the split-operand path takes, in the order they are tested (channels per group in -> out):
//   Rw3        3x3 stride 3, 64 -> 128: conv_rw_kernel in fp16x2, the float32 kernel otherwise (wr_resnet.py:27-30, stage 4)
//   Stride2Rw  3x3 stride 2, 32 -> 64: conv_rw_kernel in fp16x2, conv_bf3_kernel<2, 2, 2, 16, 512> otherwise (stage 3)
//   C8         3x3 stride 1, 8 -> 32: the tap-paired form of conv_bf3_kernel, and conv_block32_kernel<true>
//   Wide       3x3 stride 1, 32 or 64 -> 32 or 64: the 16x16x32 form (conv_bf3w_kernel; 64 -> 64 in fp16x2: conv_rw_kernel)
//   Flat       3x3, input channels in sixteens, stride 1 with 128 columns (stage 4: where the map is small the flattened bands --
//              conv_flat16_kernel in fp16x2, conv_bf3flat_kernel otherwise --, the rectangular bands on larger maps) or stride 2 with 64 columns
//   Plain      3x3 stride 1, input channels in sixteens, 32 or 64 columns: three bf16 planes in every math mode
enum class ConvClass { Unsupported, Plain, Flat, Wide, C8, Stride2Rw, Rw3 };

inline ConvClass conv_class(const ConvShape& s) {
  if (s.ksize != 3) return ConvClass::Unsupported;
  if (s.stride == 3 && s.cin_g == 64 && s.cout_g == 128) return ConvClass::Rw3;
  if (s.stride == 2 && s.cin_g == 32 && s.cout_g == 64) return ConvClass::Stride2Rw;
  if (s.stride == 1 && s.cin_g == 8 && s.cout_g == 32) return ConvClass::C8;
  const bool c32_64 = s.cout_g == 32 || s.cout_g == 64;
  if (s.stride == 1 && (s.cin_g == 32 || s.cin_g == 64) && c32_64) return ConvClass::Wide;
  if (s.cin_g < 16 || s.cin_g % 16) return ConvClass::Unsupported;
  if ((s.stride == 1 && s.cout_g == 128) || (s.stride == 2 && s.cout_g == 64)) return ConvClass::Flat;
  return s.stride == 1 && c32_64 ? ConvClass::Plain : ConvClass::Unsupported;
}
// the layers conv_rw_kernel takes in fp16x2 (cpx_cnn_rw.hip): 1 = stride 1, 64 -> 64 (stage 3's convolutions but the strided
// first one), 2 = that strided first one, 3 = stage 4's; 0 = not taken
inline int conv_rw_kind_of(const ConvShape& s) {
  switch (conv_class(s)) {
    case ConvClass::Wide: return s.cin_g == 64 && s.cout_g == 64 ? 1 : 0;
    case ConvClass::Stride2Rw: return 2;
    case ConvClass::Rw3: return 3;
    default: return 0;
  }
}

// A layer's weight-image buffer: the images of the math modes one after the other, byte offsets from its start.
// An image is rows of cout_g 16-byte entries (eight channels of one tap, one plane, one output column):
//   planes3  three bf16 planes  [g][chunk][3][9][2][cout_g] (chunk = 16 channels: 54 rows), Wide [g][chunk of 32][ky][3][kx][4][cout_g]
//            (108 rows), C8 [g][3][5][2][cout_g] (30 rows: two taps per K step)
//   planes2  two bf16 planes (CPX_CNN_MATH_BF16X2), the same order with two planes: 36 / 72 rows per chunk
//   half     two fp16 planes of the scaled weights (CPX_CNN_MATH_FP16X2), as planes2; C8: the tap-quad image of
//            conv_block32_kernel<true>, C8_HALF_ENTRIES entries per group; Rw3: in chunks of 32 (conv_rw_kernel's only image)
//   scales   the per-channel powers of two of `half` and their inverses: 2 x Cout floats, rounded up to 16 bytes
//   rw_half  Stride2Rw only: `half` once more in chunks of 32 channels, the order conv_rw_kernel reads
// An image the class does not have is `absent`, not an offset.
struct WeightImages {
  static constexpr size_t absent = ~(size_t)0;
  static constexpr size_t C8_HALF_ENTRIES = 3 * 2 * 4 * 32;
  ConvClass cls = ConvClass::Unsupported;
  int chunk = 0;  // input channels per chunk of planes3 / planes2 / half: 16 or 32 (0: C8, Unsupported)
  size_t planes3 = absent, planes2 = absent, half = absent, scales = absent, rw_half = absent, bytes = 0;

  static WeightImages of(const ConvShape& s) {
    WeightImages l;
    l.cls = conv_class(s);
    if (l.cls == ConvClass::Unsupported) return l;
    const auto put = [&l](size_t& image, size_t size) { image = l.bytes; l.bytes += size; };
    const size_t row = (size_t)s.cout_g * 16;
    const size_t scales = ((size_t)2 * s.groups * s.cout_g * sizeof(float) + 15) / 16 * 16;
    if (l.cls == ConvClass::C8) {
      put(l.planes3, (size_t)s.groups * 30 * row);
      put(l.half, (size_t)s.groups * C8_HALF_ENTRIES * 16);
      put(l.scales, scales);
      return l;
    }
    l.chunk = l.cls == ConvClass::Wide || l.cls == ConvClass::Rw3 ? 32 : 16;
    // (a chunk of a plane is 9 taps x chunk / 8 rows: either chunking gives the same bytes)
    const auto image = [&](int planes) { return (size_t)s.groups * (s.cin_g / l.chunk) * (9 * l.chunk / 8 * planes) * row; };
    if (l.cls != ConvClass::Rw3) put(l.planes3, image(3));
    if (l.cls == ConvClass::Plain) return l;
    if (l.cls != ConvClass::Rw3) put(l.planes2, image(2));
    put(l.half, image(2));
    put(l.scales, scales);
    if (l.cls == ConvClass::Stride2Rw) put(l.rw_half, image(2));
    return l;
  }
};

// The kernels divide a workgroup's (or a walked tile's) index by tile counts: q = n / d as (n * m) >> 42 with the host-computed
// m = floor(2^42 / d) + 1 -- two scalar multiplies instead of the ~25-instruction reciprocal sequence of a runtime division.
// Exact for n < 2^22, d < 2^12: n (m d - 2^42) <= n d < 2^34 < 2^42, and n m < 2^64.  So a tile count per axis stays below
// TILE_AXIS_LIMIT and the product of all counts below the caller's limit: TILES_PER_LAUNCH where a workgroup has one unit of
// work and divides only its own index (< total); TILES_PERSISTENT where a persistent grid walks the tiles in XCD eighths --
// those kernels form tile indices up to 8 * ceil(total / 8) - 1 <= total + 6 before they compare them with `total`.
constexpr int TILE_AXIS_LIMIT = 4096;
constexpr long long TILES_PER_LAUNCH = 1ll << 22;
constexpr long long TILES_PERSISTENT = (1ll << 22) - 8;
inline unsigned long long tile_magic(int d) { return (1ull << 42) / (unsigned long long)d + 1; }
#if defined(__HIPCC__)
#define CPX_WALK_HD __host__ __device__ __forceinline__
#else
#define CPX_WALK_HD inline
#endif
CPX_WALK_HD int tile_div(int n, unsigned long long m) { return (int)(((unsigned long long)n * m) >> 42); }
// one step of an index decode: the remainder of n by d (m = tile_magic(d)); n becomes the quotient
CPX_WALK_HD int tile_split(int& n, unsigned long long m, int d) {
  const int q = tile_div(n, m), r = n - q * d;
  n = q;
  return r;
}
// A kernel's tile argument: the tile counts along x and y, their product with the samples, and tile_div's multipliers.
// conv_rw_kernel takes it as it is.  BlkTiles (below) and TileDiv (cpx_cnn_bf3.hip) state the same fields themselves, with the
// walk and the column split: the byte offsets of a kernel's arguments are part of its instruction stream, and as structs
// derived from this one theirs move (profiles/cnn_conv_shared_refactor.md).  fill_tiles fills all three
struct Tiles {
  unsigned long long m_tx, m_ty;
  int tiles_x, tiles_y, total;
};

// fills tiles_x / tiles_y / total (= tiles_x tiles_y n) and their multipliers of a kernel's tile argument (schedule_point's
// way); -3: out of tile_div's range
template <class T>
int fill_tiles(T& td, int tiles_x, int tiles_y, long long n, long long limit) {
  if (tiles_x < 1 || tiles_y < 1 || tiles_x >= TILE_AXIS_LIMIT || tiles_y >= TILE_AXIS_LIMIT) return -3;
  const long long total = (long long)tiles_x * tiles_y * n;  // (< 2^24 n: no overflow for any int n)
  if (total >= limit) return -3;
  td.tiles_x = tiles_x, td.m_tx = tile_magic(tiles_x);
  td.tiles_y = tiles_y, td.m_ty = tile_magic(tiles_y);
  td.total = (int)total;
  return 0;
}
// ... and with the columns of a group split among nsplit workgroups per tile (TileDiv): the split is the innermost index
template <class T>
int fill_tiles(T& td, int tiles_x, int tiles_y, long long n, int nsplit, long long limit) {
  if (nsplit < 1 || nsplit >= TILE_AXIS_LIMIT) return -3;
  td.nsplit = nsplit, td.m_nsplit = tile_magic(nsplit);
  return fill_tiles(td, tiles_x, tiles_y, n * nsplit, limit);
}

// A persistent grid's width along x: one workgroup per CU, shared among the ny rows of the grid (groups, or (group, column
// half) pairs); a multiple of eight per row so that blockIdx.x & 7 names the XCD, and no more than the tiles rounded up to eight
inline int persistent_grid_x(int cus, int ny, long long tiles) {
  const int gx = std::max(8, cus / std::max(ny, 1) / 8 * 8);
  return (int)std::min<long long>(gx, (tiles + 7) / 8 * 8);
}
// ... on a device of `cus` compute units (0: no current device; -1).  `width_env`: an environment variable that, where
// set, gives the compute units of the whole grid instead (CPX_BLOCK32_GRID: read at every launch, for the bitwise tests and the timing)
inline int persistent_grid(int cus, int ny, long long tiles, const char* width_env = nullptr) {
  if (cus == 0) return -1;
  const char* e = width_env ? getenv(width_env) : nullptr;
  return e ? persistent_grid_x(atoi(e), 1, tiles) : persistent_grid_x(cus, ny, tiles);
}

// ---- the order in which conv_block32s_kernel's persistent workgroups walk the tiles (cpx_cnn_blk.hip), host + device ----
// Both walks hand out UNITS: every XCD (blockIdx.x & 7) owns a contiguous eighth of the units, its gx / 8 workgroups
// interleave within it, and a workgroup's units ascend.  The unit is
//   WALK_TILES  one tile: a workgroup's consecutive tiles lie gx / 8 apart and are never neighbours;
//   WALK_ROWS   one tile row of one sample, walked from its rightmost tile to its leftmost: every tile but a row's first has
//               its right neighbour as the workgroup's previous tile, which is what the kernel's halo carry needs, and
//               vertically adjacent rows of a sample are in flight in the same XCD at the same time.
enum { WALK_TILES = 0, WALK_ROWS = 1 };
struct BlkTiles {
  unsigned long long m_tx, m_ty;  // Tiles's fields (fill_tiles), at Tiles's offsets
  int tiles_x, tiles_y, total;
  int walk, units;                // WALK_*; units = total (WALK_TILES) or total / tiles_x (WALK_ROWS): set_walk
};
static_assert(sizeof(BlkTiles) == 40 && offsetof(BlkTiles, total) == offsetof(Tiles, total) && offsetof(BlkTiles, walk) == 28 &&
                  offsetof(BlkTiles, units) == 32,
              "the argument layout conv_block32s_kernel was tuned with");
inline void set_walk(BlkTiles& td, int walk) {
  td.walk = walk;
  td.units = walk == WALK_ROWS ? td.total / td.tiles_x : td.total;
}
// tile j (0, 1, ..) of workgroup bx of a grid gx wide (a multiple of eight) -> sample n, tile row ty, tile column tx; false:
// the workgroup has fewer.  No division: a caller stops at the first false, so j stays below total + 3 and a unit index
// below units + 7 -- inside tile_div's range (TILES_PERSISTENT).
CPX_WALK_HD bool walk_tile(const BlkTiles& td, int bx, int gx, int j, int& n, int& ty, int& tx) {
  int col = 0;
  if (td.walk == WALK_ROWS) {
    const int jr = tile_div(j, td.m_tx);
    col = j - jr * td.tiles_x;
    j = jr;
  }
  const int per_xcd = (td.units + 7) >> 3;
  const int t = bx + j * gx;
  if (t >= 8 * per_xcd) return false;
  int unit = (t & 7) * per_xcd + (t >> 3);
  if (unit >= td.units) return false;
  if (td.walk == WALK_ROWS) {
    tx = td.tiles_x - 1 - col;
  } else {
    const int qd = tile_div(unit, td.m_tx);
    tx = unit - qd * td.tiles_x;
    unit = qd;
  }
  n = tile_div(unit, td.m_ty);
  ty = unit - n * td.tiles_y;
  return true;
}
// The largest number of tiles one workgroup walks: XCD 0's eighth is never smaller than another's, and its first workgroup
// gets ceil(eighth / (gx / 8)) units.
inline long long walk_max_tiles(const BlkTiles& td, int walk, int gx) {
  const long long units = walk == WALK_ROWS ? td.total / td.tiles_x : td.total;
  const long long per_xcd = (units + 7) / 8, wgs = gx / 8;
  return (per_xcd + wgs - 1) / wgs * (walk == WALK_ROWS ? td.tiles_x : 1);
}
// The launcher's choice.  A carried tile (every tile of a row run but its first) costs 1 - WALK_CARRY_SAVING of a tile that
// computes its own halo columns; the launch ends with its slowest workgroup, so the row runs are taken when their largest
// per-workgroup cost, in tiles, is below the tile walk's largest count.  The saving is measured (profiles/
// block32_carry_experiments.md: six launches of 1,536 samples, 10 x 10 tiles, nine tiles in ten carried): 54.47 ms on
// interleaved tiles, 51.54 ms on row runs with the carry = 5.4 % of the launch, 6.0 % of a carried tile (the row runs
// without the carry measure 54.87 ms: the walk alone gains nothing, and the 6.0 % is net of what it costs).  At the
// bench's shape (1,559 samples, 128 workgroups per group): 122 rows = 1,220 tiles, 1,098 of them carried, against 1,218;
// a 3-sample batch on the same grid would walk 10 tiles against 3 and stays tile-interleaved.
constexpr double WALK_CARRY_SAVING = 0.06;
inline int choose_walk(const BlkTiles& td, int gx) {
  const double rows = (double)walk_max_tiles(td, WALK_ROWS, gx) / td.tiles_x * (td.tiles_x - WALK_CARRY_SAVING * (td.tiles_x - 1));
  return rows < (double)walk_max_tiles(td, WALK_TILES, gx) ? WALK_ROWS : WALK_TILES;
}

}  // namespace cpx
