// cpx_graph_conv_core.h -- the walk the graph executor's four implicit-GEMM convolutions share (graph_conv_kernel,
// graph_conv_q8_kernel, graph_conv_h2_kernel, graph_conv_i8_kernel), stated once:
//   M = the output pixels of the WHOLE batch, flattened: BM = 128 per workgroup, 32 per wave -- a small map fills its
//       tiles from the next sample instead of wasting them
//   N = the output channels of one group, 32 per MFMA tile, NTN tiles per wave; the group is blockIdx.z
//   K = kh * kw * Cg walked as (tap) x (chunk of KC input channels): a step
// Two threads stage a pixel's chunk, half of it each, and keep that pixel for the whole walk (ConvStager); step s + 1 is
// fetched to registers while the matrix cores work on step s; the epilogue walks a wave's 32 pixels across the samples
// they fall into (the pixel maps of both ends: cpx_graph_core.h).  What a kernel does with a step's patch -- the masked
// loads, the LDS image, the MFMAs -- and with its accumulators is its own: as shared helpers those pieces changed the
// kernels' registers and schedules (profiles/graph_conv_walk_refactor.md).  The host part (ConvGeom, conv_geom,
// conv_tiling, conv_step) compiles without HIP: tests/native/graph_core_host.cpp, held to plain arithmetic by
// tests/test_graph_core_host.py.
#pragma once
#include <type_traits>

#include "cpx_graph_core.h"

namespace cpx {

constexpr int CONV_TILE = 32;   // output channels of an MFMA tile (GRAPH_CONV_CO: every filter image is padded to it)

// ---- the geometry of one launch ----
struct ConvGeom {
  long long P;                  // N * Ho * Wo
  int HoWo, nchunks, ntiles;    // chunks and tiles of ONE group's walk
  int vec;                      // a thread's channels are whole aligned 16-byte pieces in every group
  int cg, cog, G;               // input / output channels of a group, the groups (1: not grouped)
};

// `kc`: the chunk width in channels; `aligned(in, cg)`: the 16-byte test of the view's element type -- group_quads
// (float32) or group_bytes16 (int8), which with cg = C are the whole view's
template <class View, class Aligned>
inline ConvGeom conv_geom(int N, const View& in, const View& out, int kc, int G, Aligned aligned) {
  ConvGeom g;
  g.G = G;
  g.HoWo = out.H * out.W;
  g.P = (long long)N * g.HoWo;
  g.cg = in.C / G;
  g.cog = out.C / G;
  g.nchunks = (g.cg + kc - 1) / kc;
  g.ntiles = (g.cog + CONV_TILE - 1) / CONV_TILE;
  g.vec = aligned(in, g.cg);
  return g;
}
// sixteen channels of an int8 view (pointer and strides in bytes) are one aligned 16-byte piece, in every group: the
// first channel of group g is c_offset + g * Cg
template <class View>
inline bool group_bytes16(const View& v, int cg) {
  return cg % 16 == 0 && v.cstride % 16 == 0 && v.sample_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(v.p) & 15) == 0;
}

// the tiles of a wave and the rows of the grid (blockIdx.y) for `ntiles` tiles: NTN 1, 2 or 4
struct ConvTiling {
  int ntn, rows;
};
CPX_HD inline ConvTiling conv_tiling(int ntiles) {
  return ntiles == 1 ? ConvTiling{1, 1} : ntiles == 2 ? ConvTiling{2, 1} : ConvTiling{4, (ntiles + 3) / 4};
}
// launch(std::integral_constant<int, NTN>(), rows)
template <class Launch>
inline void conv_dispatch_ntn(int ntiles, Launch launch) {
  const ConvTiling t = conv_tiling(ntiles);
  if (t.ntn == 1)
    launch(std::integral_constant<int, 1>(), t.rows);
  else if (t.ntn == 2)
    launch(std::integral_constant<int, 2>(), t.rows);
  else
    launch(std::integral_constant<int, 4>(), t.rows);
}

// ---- K: step s of kh * kw * nchunks -> tap (and its row and column in the window), first channel of the chunk ----
struct ConvStep {
  int tap, c0, ky, kx;
};
CPX_HD inline ConvStep conv_step(int s, int nchunks, int kw, int kc) {
  ConvStep k;
  k.tap = s / nchunks;
  k.c0 = (s - k.tap * nchunks) * kc;
  k.ky = k.tap / kw;
  k.kx = k.tap - k.ky * kw;
  return k;
}

}  // namespace cpx

#ifdef __HIPCC__
#include "cpx_kernels.h"

namespace cpx {

static_assert(CONV_TILE == GRAPH_CONV_CO, "the tiles are the filter images'");

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CT = 256;   // threads of a workgroup
constexpr int BM = 128;   // output pixels of a convolution's workgroup

inline unsigned blocks_for(size_t items) { return (unsigned)((items + CT - 1) / CT); }

__device__ __forceinline__ int pack4(int q0, int q1, int q2, int q3) {
  return (q0 & 255) | ((q1 & 255) << 8) | ((q2 & 255) << 16) | (int)((unsigned)q3 << 24);
}

// The staging role of thread tid: pixel tid / 2 of the workgroup's tile, half tid & 1 of every chunk -- the same pixel
// for the whole K walk, so its window's origin and its sample's base (64-bit over the batch, 32-bit inside a sample; from
// channel `c_first`, the group's first, on) are worked out once.  T: the view's elements, float or int8_t.
template <class T>
struct ConvStager {
  int spx, half;
  ConvPixel px;
  int iy0, ix0;
  const T* in_n;
};
template <class T>
__device__ __forceinline__ ConvStager<T> conv_stager(const GraphOpArgs& a, const ConvGeom& g, const T* in, long long p0, int tid, int c_first) {
  ConvStager<T> st;
  st.spx = tid >> 1, st.half = tid & 1;
  st.px = conv_pixel(p0 + st.spx, g.P, g.HoWo, a.out.W);
  st.iy0 = window_origin(st.px.oy, a.stride_h, a.pad_top), st.ix0 = window_origin(st.px.ox, a.stride_w, a.pad_left);
  st.in_n = in + (size_t)st.px.n * a.in0.sample_stride + c_first;
  return st;
}

// What the stager reads at step s: the first channel of the chunk and of its own half of it (within the group), whether
// the tap lies inside the image (and the pixel inside the batch), and the tap's offset in the sample -- 0 where it is
// masked, so that a masked load reads the sample's first element
struct ConvPatch {
  int tap, c0, c, pix;
  bool inside;
};
template <class T>
__device__ __forceinline__ ConvPatch conv_patch(const GraphOpArgs& a, const ConvStager<T>& st, int s, int nchunks, int kc) {
  const ConvStep k = conv_step(s, nchunks, a.kw, kc);
  const int iy = st.iy0 + k.ky, ix = st.ix0 + k.kx;
  ConvPatch f;
  f.tap = k.tap, f.c0 = k.c0, f.c = k.c0 + (kc / 2) * st.half;
  f.inside = st.px.valid && iy >= 0 && iy < a.in0.H && ix >= 0 && ix < a.in0.W;
  f.pix = f.inside ? (iy * a.in0.W + ix) * a.in0.cstride : 0;
  return f;
}

// Piece `piece` of the `pieces` 16-byte pieces of step s's fragments of every tile of the wave, from a filter image in
// fragment order [step][tile][piece]; a tile beyond the last is not multiplied: load the last
template <int NTN, class V>
__device__ __forceinline__ void prefetch_fragments(const V* img, int s, int ntiles, int tile0, int pieces, int piece, V (&next)[NTN]) {
#pragma unroll
  for (int t = 0; t < NTN; ++t) {
    const int tile = min(tile0 + t, ntiles - 1);
    next[t] = img[((size_t)s * ntiles + tile) * pieces + piece];
  }
}

}  // namespace cpx
#endif
