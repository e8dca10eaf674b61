// cpx_cnn_dev.h -- the device vocabulary of the WR-ResNet split-operand convolutions, each item once: vector types, 32-bit
// addressing, the splits of float32 into bf16 / fp16 planes, the plane products on the matrix pipe.  Included by
// cpx_cnn_bf3.hip, cpx_cnn_rw.hip and cpx_cnn_blk.hip inside their own translation unit (anonymous namespace, everything
// force-inlined: a kernel's instruction stream is what it was with the text written out in place).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace cpx {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
// a native vector, not HIP's uint4 struct: struct copies become memcpy calls that keep a staging array in scratch
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// uniform base + 32-bit unsigned byte offset: the form the compiler turns into `global_load v, v_off, s[base]` (one
// offset register per lane instead of 64-bit address arithmetic per access; everything addressed here stays inside
// one sample or one weight image: < 2^32 bytes)
template <typename T>
__device__ __forceinline__ const T* at_off(const T* base, unsigned bytes) {
  return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + bytes);
}
template <typename T>
__device__ __forceinline__ T* at_off(T* base, unsigned bytes) {
  return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + bytes);
}
// element offset of pixel (y, x) in an NHWC sample: both products stay below 2^24 (y * W + x < 2^17 pixels, x C <= 256
// channels), so the full-rate 24-bit multiply does (a 32-bit v_mul_lo_u32 / v_mad_u64_u32 takes four issue slots)
__device__ __forceinline__ unsigned pix_off(int y, int x, int W, int C) {
  return __umul24(__umul24((unsigned)y, (unsigned)W) + (unsigned)x, (unsigned)C);
}
// ReLU of a float as an integer maximum: one instruction (fmaxf(x, 0) on a value of unknown origin is canonicalised first)
__device__ __forceinline__ float relu_bits(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
// a loop whose index is a compile-time constant in every iteration (register arrays indexed by it stay registers)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

__device__ __forceinline__ unsigned pack2(float a, float b) {
  bf16x2 v = {(__bf16)a, (__bf16)b};  // v_cvt_pk_bf16_f32: round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
// two float32 -> their three bf16 planes (packed pairs)
__device__ __forceinline__ void split_pair(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  p0 = pack2(a, b);
  // (opaque: seeing through the pack, the compiler converts `a` a second time just to shift it -- one vector
  // instruction more per level and pair; the halves of the packed word are what is wanted)
  asm volatile("" : "+v"(p0));
  const float ra = a - bf_lo(p0), rb = b - bf_hi(p0);  // exact
  p1 = pack2(ra, rb);
  asm volatile("" : "+v"(p1));
  const float sa = ra - bf_lo(p1), sb = rb - bf_hi(p1);  // exact
  p2 = pack2(sa, sb);
}

// two float32 -> TWO bf16 planes, each rounded to nearest (v_cvt_pk_bf16_f32): hi + lo carries 16 significand bits,
// |x - hi - lo| <= 2^-16 |x| (CPX_CNN_MATH_BF16X2: three products per K step instead of six)
__device__ __forceinline__ unsigned pack2_rne(float a, float b) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ void split_pair2(float a, float b, unsigned& p0, unsigned& p1) {
  p0 = pack2_rne(a, b);
  const float ra = a - bf_lo(p0), rb = b - bf_hi(p0);  // exact
  p1 = pack2_rne(ra, rb);
}

// CPX_CNN_MATH_FP16X2: two float32 -> two fp16 planes, each rounded to nearest (v_cvt_pk_f16_f32): 11 + 11 significand
// bits and the sign of the remainder, |x - hi - lo| <= 2^-22 |x| while lo is a normal fp16 (|x| >= 2^-3 after the
// caller's scaling) and <= 2^-25 absolute below that (v_mfma_*_f16 keeps subnormal inputs: scratch/fp16_probe.hip)
__device__ __forceinline__ unsigned pack2_h(float a, float b) {
  f16x2 v = {(_Float16)a, (_Float16)b};  // v_cvt_pk_f16_f32: round to nearest even
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void split_pair2_h(float a, float b, unsigned& p0, unsigned& p1) {
  p0 = pack2_h(a, b);
  // lo = fp16(x - hi): the difference is exact in float32, so ONE mixed-precision fused multiply-add per element (x * 1.0 - hi,
  // float32 inside, rounded to nearest fp16 once, into the low / high half of p1) is the same value as convert-back, subtract,
  // convert -- three instructions per pair instead of six
  asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "=v"(p1) : "v"(a), "v"(p0));
  asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(p1) : "v"(b), "v"(p0));
}
// the two-plane split of the chosen kind (H: fp16, else bf16)
template <bool H>
__device__ __forceinline__ void split2(float a, float b, unsigned& p0, unsigned& p1) {
  if (H) split_pair2_h(a, b, p0, p1);
  else split_pair2(a, b, p0, p1);
}
// eight float32 (the channels of one 16-byte entry) -> the entry of each plane.  H: two fp16 planes of v * ws (a power of
// two); else three or two bf16 planes (p2 is written for three only).  The weight images are built from this
// (split_weights*_kernel, once per network)
template <bool H>
__device__ __forceinline__ void split8(const float (&v)[8], float ws, int planes, uint4& p0, uint4& p1, uint4& p2) {
  unsigned q0[4], q1[4], q2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (H) split_pair2_h(v[2 * j] * ws, v[2 * j + 1] * ws, q0[j], q1[j]);
    else if (planes == 3) split_pair(v[2 * j], v[2 * j + 1], q0[j], q1[j], q2[j]);
    else split_pair2(v[2 * j], v[2 * j + 1], q0[j], q1[j]);
  }
  p0 = make_uint4(q0[0], q0[1], q0[2], q0[3]);
  p1 = make_uint4(q1[0], q1[1], q1[2], q1[3]);
  if (!H && planes == 3) p2 = make_uint4(q2[0], q2[1], q2[2], q2[3]);
}

// one plane product on the matrix pipe: 16-byte fragments as they come out of LDS
template <bool H>
__device__ __forceinline__ f32x4 mfma16(u32x4 w, u32x4 x, f32x4 c) {
  if (H) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, x), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), c, 0, 0, 0);
}
template <bool H>
__device__ __forceinline__ f32x16 mfma32(u32x4 x, u32x4 w, f32x16 c) {
  if (H) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, x), __builtin_bit_cast(f16x8, w), c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, x), __builtin_bit_cast(bf16x8, w), c, 0, 0, 0);
}
// the plane products of one K step, x = activation planes, w = weight planes, smallest terms first:
// x1 w1, x0 w2, x2 w0 (three planes only), then x0 w1, x1 w0, x0 w0.  32 x 32 tiles (pixels x columns) and 16 x 16 tiles
// (columns x pixels: the operands' roles are swapped, the order of the terms is the same)
template <int PL, bool H>
__device__ __forceinline__ void plane_products32(const u32x4 (&x)[PL], const u32x4 (&w)[PL], f32x16& acc) {
  if (PL == 3) {
    acc = mfma32<false>(x[1], w[1], acc);
    acc = mfma32<false>(x[0], w[PL - 1], acc);
    acc = mfma32<false>(x[PL - 1], w[0], acc);
  }
  acc = mfma32<H>(x[0], w[1], acc);
  acc = mfma32<H>(x[1], w[0], acc);
  acc = mfma32<H>(x[0], w[0], acc);
}
template <int PL, bool H>
__device__ __forceinline__ void plane_products16(const u32x4 (&x)[PL], const u32x4 (&w)[PL], f32x4& acc) {
  if (PL == 3) {
    acc = mfma16<false>(w[1], x[1], acc);
    acc = mfma16<false>(w[PL - 1], x[0], acc);
    acc = mfma16<false>(w[0], x[PL - 1], acc);
  }
  acc = mfma16<H>(w[1], x[0], acc);
  acc = mfma16<H>(w[0], x[1], acc);
  acc = mfma16<H>(w[0], x[0], acc);
}

constexpr float F16_MAX = 65504.0f;
// producer-side split (ConvArgs::out_planes): four consecutive channels of one pixel, activated and already multiplied by
// the consumer's act_scale, as the consumer stages them: [hi 0..3 | lo 0..3] in the 16 bytes the float32 values would take
__device__ __forceinline__ u32x4 planes_of(f32x4 v) {
  unsigned h0, h1, l0, l1;
  split_pair2_h(v.x, v.y, h0, l0);
  split_pair2_h(v.z, v.w, h1, l1);
  return u32x4{h0, h1, l0, l1};
}
// the running maximum of fp16 bit patterns, two packed halves per instruction: a high plane that came out infinite is a
// value out of fp16's range
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  unsigned r;
  asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float max_abs4(f32x4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
// a clamp to [lo, hi] in one instruction (hi wave-uniform)
__device__ __forceinline__ int med3(int x, int lo, int hi) {
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "s"(hi));
  return r;
}

}  // namespace

}  // namespace cpx
