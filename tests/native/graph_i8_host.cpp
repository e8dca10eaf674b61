// graph_i8_host.cpp -- csrc/cpx_graph_i8_core.h compiled for the HOST, for tests/test_graph_i8_host.py: the full-integer
// arithmetic of the graph executor, element by element over arrays.  The product never loads this build.
#include "cpx_graph_i8_core.h"

extern "C" {

void srdhm_host(const int32_t* a, const int32_t* b, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::srdhm(a[i], b[i]);
}

void rdivpot_host(const int32_t* x, const int32_t* e, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::rdivpot(x[i], e[i]);
}

void mbqm_host(const int32_t* x, const int32_t* m, const int32_t* shift, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::mbqm(x[i], m[i], shift[i]);
}

void quantize_f32_host(const float* x, float s, int32_t z, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::quantize_f32(x[i], s, z);
}

void dequantize_i8_host(const int32_t* q, float s, int32_t z, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::dequantize_i8(q[i], s, z);
}

// header: CPX_GRAPH_I8_HDR_WORDS int32 words
void add_i8_host(const int32_t* q1, const int32_t* q2, int sign, const int32_t* header, int n, int32_t* out) {
  cpx::I8Header h;
  for (int k = 0; k < CPX_GRAPH_I8_HDR_WORDS; ++k) h.v[k] = header[k];
  for (int i = 0; i < n; ++i) out[i] = cpx::add_i8(q1[i], q2[i], sign, h);
}

void mul_i8_host(const int32_t* q1, const int32_t* q2, const int32_t* header, int n, int32_t* out) {
  cpx::I8Header h;
  for (int k = 0; k < CPX_GRAPH_I8_HDR_WORDS; ++k) h.v[k] = header[k];
  for (int i = 0; i < n; ++i) out[i] = cpx::mul_i8(q1[i], q2[i], h);
}

void mean_i8_host(const int32_t* sum, int32_t count, const int32_t* header, int n, int32_t* out) {
  cpx::I8Header h;
  for (int k = 0; k < CPX_GRAPH_I8_HDR_WORDS; ++k) h.v[k] = header[k];
  for (int i = 0; i < n; ++i) out[i] = cpx::mean_i8(sum[i], count, h);
}

void round_div_host(const int32_t* acc, const int32_t* cnt, int n, int32_t* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::round_div(acc[i], cnt[i]);
}

}  // extern "C"
