// cpx_graph_i8_core.h -- the arithmetic of the full-integer operators of the TFLite graph executor (cpx_graph_i8.hip),
// fixed in include/cpx.h ("The full-integer arithmetic"): the TFLite reference integer kernels' fixed-point steps as
// published, each written ONCE here so that the device, a host build (tests/native/graph_i8_host.cpp, held bit for bit to
// the NumPy restatement tests/tflite_eval_i8.py by tests/test_graph_i8_host.py) and the planner agree.  Everything is
// integer but the two ends: QUANTIZE is one float32 division and a roundf, DEQUANTIZE one exact conversion and one
// float32 multiply (the build has -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "cpx.h"

#ifndef CPX_HD
#ifdef __HIPCC__
#define CPX_HD __host__ __device__
#else
#define CPX_HD
#endif
#endif

namespace cpx {

// the int32 header every full-integer operator carries in `shift` (include/cpx.h: CPX_GRAPH_I8_HDR_*)
struct I8Header {
  int32_t v[CPX_GRAPH_I8_HDR_WORDS];
};

// saturating rounding doubling high multiply: round-half-away(a * b / 2^31)
CPX_HD inline int32_t srdhm(int32_t a, int32_t b) {
  if (a == b && a == INT32_MIN) return INT32_MAX;
  const int64_t ab = (int64_t)a * (int64_t)b;
  const int64_t nudge = ab >= 0 ? (int64_t)(1 << 30) : (int64_t)(1 - (1 << 30));
  return (int32_t)((ab + nudge) / ((int64_t)1 << 31));   // C's division: it truncates
}

// rounding (half away from zero) division by 2^e, 0 <= e <= 31
CPX_HD inline int32_t rdivpot(int32_t x, int e) {
  const int32_t mask = (int32_t)(((int64_t)1 << e) - 1);
  const int32_t rem = x & mask;
  const int32_t thr = (mask >> 1) + (x < 0 ? 1 : 0);
  return (x >> e) + (rem > thr ? 1 : 0);
}

// MultiplyByQuantizedMultiplier: x * M * 2^(shift - 31), rounded twice as the reference kernels round.  The planner keeps
// |x| * 2^max(shift, 0) below 2^31; the product is written in unsigned arithmetic so that even a broken promise wraps
// the same way on every build.
CPX_HD inline int32_t mbqm(int32_t x, int32_t M, int shift) {
  const int left = shift > 0 ? shift : 0, right = shift > 0 ? 0 : -shift;
  return rdivpot(srdhm((int32_t)((uint32_t)x << left), M), right);
}

CPX_HD inline int32_t clamp_i8(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// QUANTIZE, float32 -> int8: t = roundf(float32(x / s)) clamped in float to [-128 - z, 127 - z], q = int(t) + z; NaN: z
CPX_HD inline int32_t quantize_f32(float x, float s, int32_t z) {
  const float t = roundf(x / s);
  if (!(t == t)) return z;
  const float lo = (float)(-128 - z), hi = (float)(127 - z);
  return (int32_t)(t < lo ? lo : t > hi ? hi : t) + z;
}

// DEQUANTIZE: float32(s) * float32(q - z)
CPX_HD inline float dequantize_i8(int32_t q, float s, int32_t z) { return s * (float)(q - z); }

// QUANTIZE, int8 -> int8 (also a stand-alone RELU / RELU6): clamp(z_out + MBQM(q - z_in, M0))
CPX_HD inline int32_t requantize_i8(int32_t q, const I8Header& h) {
  return clamp_i8(h.v[CPX_GRAPH_I8_HDR_Z_OUT] + mbqm(q - h.v[CPX_GRAPH_I8_HDR_Z_IN], h.v[CPX_GRAPH_I8_HDR_M0], h.v[CPX_GRAPH_I8_HDR_S0]),
                  h.v[CPX_GRAPH_I8_HDR_LO], h.v[CPX_GRAPH_I8_HDR_HI]);
}

// ADD_I8 (sign 1) / SUB (sign -1)
CPX_HD inline int32_t add_i8(int32_t q1, int32_t q2, int sign, const I8Header& h) {
  const int left = h.v[CPX_GRAPH_I8_HDR_LEFT];
  const int32_t a = mbqm((int32_t)((uint32_t)(q1 - h.v[CPX_GRAPH_I8_HDR_Z_IN]) << left), h.v[CPX_GRAPH_I8_HDR_M0], h.v[CPX_GRAPH_I8_HDR_S0]);
  const int32_t b = mbqm((int32_t)((uint32_t)(q2 - h.v[CPX_GRAPH_I8_HDR_Z_IN1]) << left), h.v[CPX_GRAPH_I8_HDR_M1], h.v[CPX_GRAPH_I8_HDR_S1]);
  const int32_t sum = sign < 0 ? a - b : a + b;
  return clamp_i8(h.v[CPX_GRAPH_I8_HDR_Z_OUT] + mbqm(sum, h.v[CPX_GRAPH_I8_HDR_MO], h.v[CPX_GRAPH_I8_HDR_SO]), h.v[CPX_GRAPH_I8_HDR_LO],
                  h.v[CPX_GRAPH_I8_HDR_HI]);
}

// MUL_I8
CPX_HD inline int32_t mul_i8(int32_t q1, int32_t q2, const I8Header& h) {
  const int32_t p = (q1 - h.v[CPX_GRAPH_I8_HDR_Z_IN]) * (q2 - h.v[CPX_GRAPH_I8_HDR_Z_IN1]);
  return clamp_i8(h.v[CPX_GRAPH_I8_HDR_Z_OUT] + mbqm(p, h.v[CPX_GRAPH_I8_HDR_M0], h.v[CPX_GRAPH_I8_HDR_S0]), h.v[CPX_GRAPH_I8_HDR_LO],
                  h.v[CPX_GRAPH_I8_HDR_HI]);
}

// AVG_POOL_I8's and MEAN_I8's division by the count n >= 1: half away from zero, C's truncating division
CPX_HD inline int32_t round_div(int32_t acc, int32_t n) { return acc > 0 ? (acc + n / 2) / n : (acc - n / 2) / n; }

// MEAN_I8 from the integer sum over the n = H * W pixels; HDR_LEFT carries the bias
CPX_HD inline int32_t mean_i8(int32_t sum, int32_t n, const I8Header& h) {
  const int32_t acc = round_div(mbqm(sum, h.v[CPX_GRAPH_I8_HDR_M0], h.v[CPX_GRAPH_I8_HDR_S0]), n) + h.v[CPX_GRAPH_I8_HDR_LEFT];
  return clamp_i8(acc, h.v[CPX_GRAPH_I8_HDR_LO], h.v[CPX_GRAPH_I8_HDR_HI]);
}

// the filter kinds' finish: acc = sum q * w over the taps with a masked element staged as q = z_in, wsum = sum w
// (DWCONV_I8 sums (q - z_in) * w over the in-bounds taps and passes wsum = 0): clamp(z_out + MBQM(acc - z_in * wsum + bias))
CPX_HD inline int32_t filter_finish_i8(int32_t acc, int32_t wsum, int32_t bias, int32_t M, int shift, const I8Header& h) {
  const int32_t v = (int32_t)((uint32_t)acc - (uint32_t)h.v[CPX_GRAPH_I8_HDR_Z_IN] * (uint32_t)wsum + (uint32_t)bias);
  return clamp_i8(h.v[CPX_GRAPH_I8_HDR_Z_OUT] + mbqm(v, M, shift), h.v[CPX_GRAPH_I8_HDR_LO], h.v[CPX_GRAPH_I8_HDR_HI]);
}

// LUT_I8 and CPX_GRAPH_ACT_LUT: the 256-entry table rides behind the header; a sign-extended byte q reads entry q + 128
CPX_HD inline const int8_t* table_of(const I8Header* h) { return reinterpret_cast<const int8_t*>(h + 1); }
CPX_HD inline int lut_index(int32_t q) { return q + 128; }
CPX_HD inline int32_t lut_i8(const int8_t* table, int32_t q) { return table[lut_index(q)]; }

}  // namespace cpx
