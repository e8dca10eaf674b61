// TEST INFRASTRUCTURE ONLY: host build of the activation of classifier-pipeline_amd/csrc/cpx_graph_core.h
// (tests/test_tflite_se_cpu.py), with -ffp-contract=off as the product: activate() over an array.  The product never
// loads it.
#include "cpx_graph_core.h"

extern "C" void activate_host(const float* v, int act, int n, float* out) {
  for (int i = 0; i < n; ++i) out[i] = cpx::activate(v[i], act);
}
extern "C" int mean_wide_pixels_host() { return cpx::GRAPH_MEAN_WIDE_PIXELS; }
extern "C" int mean_stripes_host() { return cpx::GRAPH_MEAN_STRIPES; }
