// The fp16x2 convolution's RANGE parameters (classifier-pipeline_amd/csrc/cpx_graph_core.h: range_params) compiled for
// the host, so that tests/test_tflite_h2_cpu.py can hold the function the kernel calls to the NumPy restatement.
#include "cpx_graph_core.h"

extern "C" void range_params_host(const float* m, int n, float* up, float* down) {
  for (int i = 0; i < n; ++i) {
    const cpx::RangeParams p = cpx::range_params(m[i]);
    up[i] = p.up;
    down[i] = p.down;
  }
}
