// cpx_api_graph.cpp -- the TFLite graph executor's entry points, float32 and hybrid operators alike (include/cpx.h: cpx_graph_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "cpx_internal.h"

static_assert(sizeof(cpx_graph_tensor) == 32 && sizeof(cpx_graph_op) == 112, "graph layouts are part of the ABI");

// ---- TFLite graph executor (LiteInterpreter.predict, ml_tools/interpreter.py:520-560) ------------------------
struct cpx_graph {
  cpx_handle* h = nullptr;
  std::vector<cpx_graph_op> ops;
  std::vector<cpx_graph_tensor> tensors;
  int input = 0, output = 0;
  size_t arena_floats = 0;  // per sample
};

void graph_free(cpx_graph* g) { delete g; }

extern "C" {

// the window of a convolution or a pool: kernel sides, strides (1 to smax; `bad_stride` names a miss), pads and the
// output size that follows from them.  NULL: it fits.
static const char* graph_check_window(const cpx_graph_op& o, const cpx_graph_tensor& a, const cpx_graph_tensor& y, int smax,
                                      const char* bad_stride) {
  if (o.kh < 1 || o.kw < 1 || o.kh > 7 || o.kw > 7) return "kernel sides are 1 to 7";
  if (o.stride_h < 1 || o.stride_w < 1 || o.stride_h > smax || o.stride_w > smax) return bad_stride;
  if (o.pad_top < 0 || o.pad_left < 0 || o.pad_bottom < 0 || o.pad_right < 0 || o.pad_top >= o.kh || o.pad_bottom >= o.kh ||
      o.pad_left >= o.kw || o.pad_right >= o.kw)
    return "bad padding";
  const int hh = a.H + o.pad_top + o.pad_bottom - o.kh, ww = a.W + o.pad_left + o.pad_right - o.kw;
  if (hh < 0 || ww < 0 || y.H != hh / o.stride_h + 1 || y.W != ww / o.stride_w + 1) return "output size does not follow from kernel, stride and pads";
  return nullptr;
}

// what one operator asks of its tensors; every kernel masks by these sizes, so a graph that passes cannot reach outside
// the views it names (the weights' extents are the caller's: device pointers cannot be measured)
static const char* graph_check_op(const cpx_graph_op& o, const std::vector<cpx_graph_tensor>& t, int input, int output) {
  const int nt = (int)t.size();
  if (o.in0 < 0 || o.in0 >= nt || o.out < 0 || o.out >= nt || o.in1 >= nt) return "tensor id out of range";
  if (o.out == input || o.in0 == output || o.in1 == output) return "the input is written or the output read";
  const cpx_graph_tensor &a = t[o.in0], &y = t[o.out];
  if (o.out_c_offset != y.c_offset || o.out_c_stride != y.c_stride) return "output slice differs from the tensor's";
  if (o.activation != CPX_GRAPH_ACT_NONE && o.activation != CPX_GRAPH_ACT_RELU && o.activation != CPX_GRAPH_ACT_RELU6 &&
      o.activation != CPX_GRAPH_ACT_SWISH && o.activation != CPX_GRAPH_ACT_LOGISTIC && o.activation != CPX_GRAPH_ACT_LUT)
    return "unknown activation";
  if (o.activation == CPX_GRAPH_ACT_LUT && o.kind != CPX_GRAPH_CONV_I8 && o.kind != CPX_GRAPH_CONV_I8_GROUPED && o.kind != CPX_GRAPH_DWCONV_I8)
    return "the activation LUT (a table behind the int32 header) is taken by CONV_I8, CONV_I8_GROUPED and DWCONV_I8 only";
  const bool same_hw = a.H == y.H && a.W == y.W;
  // the element types each kind takes: float32 throughout, unless the kind says otherwise below
  const bool a8 = a.type == CPX_GRAPH_TYPE_INT8, y8 = y.type == CPX_GRAPH_TYPE_INT8;
  const bool b8 = o.in1 >= 0 && t[o.in1].type == CPX_GRAPH_TYPE_INT8;
  bool types_ok = !a8 && !y8 && !b8;
  const bool i8_header = o.kind >= CPX_GRAPH_QUANTIZE && o.kind <= CPX_GRAPH_LUT_I8;
  if (i8_header && (!o.shift || (reinterpret_cast<uintptr_t>(o.shift) & 3))) return "a full-integer operator without its int32 header in `shift`";
  auto is_params = [&](int id) { return id >= 0 && t[id].H == 1 && t[id].W == 1 && t[id].C == 4; };
  switch (o.kind) {
    case CPX_GRAPH_CONV:
    case CPX_GRAPH_CONV_PRE:
    case CPX_GRAPH_CONV_Q8:
    case CPX_GRAPH_CONV_F16X2:
    case CPX_GRAPH_CONV_GROUPED:
    case CPX_GRAPH_CONV_Q8_GROUPED:
    case CPX_GRAPH_DWCONV:
    case CPX_GRAPH_DWCONV_PRE:
    case CPX_GRAPH_DWCONV_Q8:
    case CPX_GRAPH_MAX_POOL:
    case CPX_GRAPH_AVG_POOL: {
      const bool dw = o.kind == CPX_GRAPH_DWCONV || o.kind == CPX_GRAPH_DWCONV_PRE || o.kind == CPX_GRAPH_DWCONV_Q8;
      const bool grouped = o.kind == CPX_GRAPH_CONV_GROUPED || o.kind == CPX_GRAPH_CONV_Q8_GROUPED;
      const bool conv = dw || grouped || o.kind == CPX_GRAPH_CONV || o.kind == CPX_GRAPH_CONV_PRE || o.kind == CPX_GRAPH_CONV_Q8 ||
                        o.kind == CPX_GRAPH_CONV_F16X2;
      if (const char* bad = graph_check_window(o, a, y, grouped ? 3 : conv ? 2 : 7, grouped ? "grouped CONV: strides are 1 to 3" : "bad stride")) return bad;
      if (conv && !o.weights) return "CONV without weights";
      if (!conv && a.C != y.C) return "pool changes the channel count";
      if (dw && a.C != y.C) return "DWCONV changes the channel count (depth multiplier 1 only)";
      if (o.kind == CPX_GRAPH_CONV_PRE) {
        if (o.param != (float)CPX_GRAPH_ACT_RELU && o.param != (float)CPX_GRAPH_ACT_RELU6) return "CONV_PRE: param is the pre-activation, RELU or RELU6";
        if (reinterpret_cast<uintptr_t>(o.weights) & 15) return "CONV_PRE weights are not 16-byte aligned";
      }
      if (o.kind == CPX_GRAPH_DWCONV_PRE && o.param != (float)CPX_GRAPH_ACT_RELU && o.param != (float)CPX_GRAPH_ACT_RELU6)
        return "DWCONV_PRE: param is the pre-activation, RELU or RELU6";
      if ((o.kind == CPX_GRAPH_DWCONV || o.kind == CPX_GRAPH_DWCONV_PRE) && (reinterpret_cast<uintptr_t>(o.weights) & 15))
        return "DWCONV weights are not 16-byte aligned";
      if (o.kind == CPX_GRAPH_DWCONV_Q8 && (reinterpret_cast<uintptr_t>(o.weights) & 3)) return "DWCONV_Q8 weights are not 4-byte aligned";
      if (grouped) {
        if (o.n_map < 2) return "grouped CONV: n_map carries the number of groups, 2 or more";
        if (a.C % o.n_map != 0) return "grouped CONV: the groups do not divide the input channels";
        if (y.C % o.n_map != 0) return "grouped CONV: the groups do not divide the output channels";
        if (o.kind == CPX_GRAPH_CONV_GROUPED && (reinterpret_cast<uintptr_t>(o.weights) & 15)) return "CONV_GROUPED weights are not 16-byte aligned";
        if (o.kind == CPX_GRAPH_CONV_Q8_GROUPED && (reinterpret_cast<uintptr_t>(o.weights) & 15)) return "CONV_Q8_GROUPED weights are not 16-byte aligned";
      }
      if (o.kind == CPX_GRAPH_CONV_F16X2) {
        if (reinterpret_cast<uintptr_t>(o.weights) & 15) return "CONV_F16X2 weights are not 16-byte aligned";
        if (!is_params(o.in1)) return "CONV_F16X2 needs the 1 x 1 x 4 RANGE tensor of its input as in1";
      }
      break;
    }
    case CPX_GRAPH_ADD:
      if (o.in1 < 0) return "ADD needs two inputs";
      if (!same_hw || a.C != y.C || t[o.in1].H != y.H || t[o.in1].W != y.W || t[o.in1].C != y.C) return "ADD of different shapes";
      break;
    case CPX_GRAPH_MUL: {
      if (o.in1 < 0) return "MUL needs two inputs";
      const cpx_graph_tensor& b = t[o.in1];
      if (!same_hw || a.C != y.C || b.C != y.C) return "MUL changes the shape";
      if (!(b.H == y.H && b.W == y.W) && !(b.H == 1 && b.W == 1)) return "MUL: in1 has neither the shape of in0 nor 1 x 1 x C";
      break;
    }
    case CPX_GRAPH_AFFINE:
    case CPX_GRAPH_LOGISTIC:
    case CPX_GRAPH_SOFTMAX:
      if (!same_hw || a.C != y.C) return "element-wise operator changes the shape";
      break;
    case CPX_GRAPH_MEAN:
      if (y.H != 1 || y.W != 1 || a.C != y.C) return "MEAN gives 1 x 1 x C";
      break;
    case CPX_GRAPH_FC:
    case CPX_GRAPH_FC_Q8:
      if (a.H != 1 || a.W != 1 || y.H != 1 || y.W != 1 || !o.weights) return "FULLY_CONNECTED takes and gives 1 x 1 x C";
      break;
    case CPX_GRAPH_QUANT_PARAMS:
      if (!is_params(o.out)) return "QUANT_PARAMS writes a 1 x 1 x 4 tensor";
      if (o.param != 0.0f && o.param != 1.0f) return "QUANT_PARAMS: param is 0 (asymmetric) or 1 (symmetric)";
      break;
    case CPX_GRAPH_RANGE:
      if (!is_params(o.out)) return "RANGE writes a 1 x 1 x 4 tensor";
      break;
    case CPX_GRAPH_PAD:
      if (o.pad_top < 0 || o.pad_left < 0 || o.pad_bottom < 0 || o.pad_right < 0 || a.C != y.C ||
          y.H != a.H + o.pad_top + o.pad_bottom || y.W != a.W + o.pad_left + o.pad_right)
        return "PAD sizes do not add up";
      break;
    case CPX_GRAPH_SLICE: {
      // pad_top / pad_left are signed (negative: a crop); the kernel masks every read by the input's size
      if (o.kh != 1 || o.kw != 1) return "SLICE: kh = kw = 1";
      if (o.stride_h < 1 || o.stride_w < 1 || o.stride_h > 7 || o.stride_w > 7) return "bad stride";
      if (o.activation != CPX_GRAPH_ACT_NONE && o.activation != CPX_GRAPH_ACT_RELU && o.activation != CPX_GRAPH_ACT_RELU6)
        return "SLICE: the activation is NONE, RELU or RELU6";
      const int hh = a.H + o.pad_top + o.pad_bottom - 1, ww = a.W + o.pad_left + o.pad_right - 1;
      if (hh < 0 || ww < 0 || y.H != hh / o.stride_h + 1 || y.W != ww / o.stride_w + 1) return "SLICE: output size does not follow from stride and pads";
      if (a.C != y.C) return "SLICE changes the channel count";
      if (o.param != 0.0f && o.param != 1.0f) return "SLICE: param is 0 (a copy) or 1 (-0.0 becomes +0.0)";
      if (a8 || y8) {
        if (!a8 || !y8 || o.in1 >= 0) return "SLICE: input and output are of one type";
        if (o.activation != CPX_GRAPH_ACT_NONE || o.param != 0.0f) return "SLICE on int8 tensors copies bytes: no activation, param 0";
        if (!o.shift || (reinterpret_cast<uintptr_t>(o.shift) & 3)) return "SLICE on int8 tensors needs the int32 header (the zero point) in `shift`";
        types_ok = true;
      }
      break;
    }
    case CPX_GRAPH_QUANTIZE:
      if (!same_hw || a.C != y.C || o.in1 >= 0) return "QUANTIZE keeps the shape and has one input";
      if (!y8) return "QUANTIZE writes an int8 tensor";
      if (!a8 && !(o.param > 0.0f)) return "QUANTIZE: param is the output's scale, above 0";
      types_ok = true;
      break;
    case CPX_GRAPH_DEQUANTIZE:
      if (!same_hw || a.C != y.C || o.in1 >= 0) return "DEQUANTIZE keeps the shape and has one input";
      if (!a8 || y8) return "DEQUANTIZE reads an int8 tensor and writes a float32 one";
      if (!(o.param > 0.0f)) return "DEQUANTIZE: param is the input's scale, above 0";
      types_ok = true;
      break;
    case CPX_GRAPH_CONV_I8:
    case CPX_GRAPH_CONV_I8_GROUPED:
    case CPX_GRAPH_DWCONV_I8:
    case CPX_GRAPH_MAX_POOL_I8:
    case CPX_GRAPH_AVG_POOL_I8: {
      const bool dw = o.kind == CPX_GRAPH_DWCONV_I8, grouped = o.kind == CPX_GRAPH_CONV_I8_GROUPED;
      const bool conv = dw || grouped || o.kind == CPX_GRAPH_CONV_I8;
      if (const char* bad = graph_check_window(o, a, y, grouped ? 3 : conv ? 2 : 7, "bad stride")) return bad;
      if ((!conv || dw) && a.C != y.C) return "the operator keeps the channel count";
      if (conv && (!o.weights || !o.scale)) return "a full-integer filter operator without weights or its int32 M / shift / bias in `scale`";
      if (conv && ((reinterpret_cast<uintptr_t>(o.weights) & 15) || (reinterpret_cast<uintptr_t>(o.scale) & 3))) return "a full-integer filter operator's weights are not 16-byte aligned";
      if (grouped && (o.n_map < 2 || a.C % o.n_map != 0 || y.C % o.n_map != 0)) return "grouped CONV: n_map carries the number of groups, which divide the input and output channels";
      if (!a8 || !y8 || o.in1 >= 0) return "the operator takes one int8 tensor and writes one";
      types_ok = true;
      break;
    }
    case CPX_GRAPH_FC_I8:
      if (a.H != 1 || a.W != 1 || y.H != 1 || y.W != 1 || !o.weights || !o.scale) return "FULLY_CONNECTED takes and gives 1 x 1 x C";
      if ((reinterpret_cast<uintptr_t>(o.weights) & 3) || (reinterpret_cast<uintptr_t>(o.scale) & 3)) return "FC_I8 weights are not 4-byte aligned";
      if (!a8 || !y8 || o.in1 >= 0) return "the operator takes one int8 tensor and writes one";
      types_ok = true;
      break;
    case CPX_GRAPH_ADD_I8:
    case CPX_GRAPH_MUL_I8:
      if (!same_hw || a.C != y.C) return "element-wise operator changes the shape";
      if (o.in1 >= 0) {   // the shape of in0, or for MUL_I8 the 1 x 1 x C gate
        const cpx_graph_tensor& b = t[o.in1];
        const bool same = b.H == y.H && b.W == y.W, gate = o.kind == CPX_GRAPH_MUL_I8 && b.H == 1 && b.W == 1;
        if (b.C != y.C || (!same && !gate)) return "ADD_I8 / MUL_I8 of different shapes (MUL_I8: in1 has the shape of in0 or is 1 x 1 x C)";
      }
      if (o.in1 < 0 && !o.weights) return "ADD_I8 / MUL_I8 needs a second tensor or the constant in `weights`";
      if (o.kind == CPX_GRAPH_ADD_I8 && o.param != 1.0f && o.param != -1.0f) return "ADD_I8: param is 1 (ADD) or -1 (SUB)";
      if (!a8 || !y8 || (o.in1 >= 0 && !b8)) return "the operator takes int8 tensors and writes one";
      types_ok = true;
      break;
    case CPX_GRAPH_LUT_I8:
      if (!same_hw || a.C != y.C || o.in1 >= 0) return "LUT_I8 keeps the shape and has one input";
      if (!a8 || !y8) return "the operator takes one int8 tensor and writes one";
      types_ok = true;
      break;
    case CPX_GRAPH_MEAN_I8:
      if (y.H != 1 || y.W != 1 || a.C != y.C || o.in1 >= 0) return "MEAN gives 1 x 1 x C";
      if (!a8 || !y8) return "the operator takes one int8 tensor and writes one";
      types_ok = true;
      break;
    case CPX_GRAPH_INPUT:
      if (!o.shift || !(o.param > 0.0f)) return "INPUT needs a shift and a positive param";
      /* fall through */
    case CPX_GRAPH_CHANNEL_MAP:
      if (!same_hw || o.n_map != y.C || o.n_map < 1 || o.n_map > 4) return "channel map of 1 to 4 output channels";
      for (int c = 0; c < o.n_map; ++c)
        if (o.channel_map[c] < 0 || o.channel_map[c] >= a.C) return "channel map index out of range";
      break;
    default:
      return "unknown operator kind";
  }
  // what a hybrid operator needs beyond its float32 twin (the caller's message names the operator's kind)
  if (o.kind == CPX_GRAPH_CONV_Q8 || o.kind == CPX_GRAPH_FC_Q8 || o.kind == CPX_GRAPH_DWCONV_Q8 || o.kind == CPX_GRAPH_CONV_Q8_GROUPED) {
    if (!is_params(o.in1)) return "a hybrid operator needs a 1 x 1 x 4 parameter tensor as in1";
    if (!o.scale || !o.shift) return "a hybrid operator without scale or shift";
  }
  if (!types_ok) return "a tensor's element type is not what the operator's kind takes";
  return nullptr;
}

int cpx_graph_create(cpx_handle* h, const cpx_graph_op* ops, int n_ops, const cpx_graph_tensor* tensors, int n_tensors,
                     int input_tensor, int output_tensor, cpx_graph** out) {
  if (!h) return CPX_ERR_INVALID;
  if (!ops || !tensors || !out || n_ops < 1 || n_tensors < 2 || input_tensor < 0 || input_tensor >= n_tensors ||
      output_tensor < 0 || output_tensor >= n_tensors || input_tensor == output_tensor)
    return fail(h, CPX_ERR_INVALID, "cpx_graph_create: bad argument");
  *out = nullptr;
  cpx_graph* g = new (std::nothrow) cpx_graph();
  if (!g) return fail(h, CPX_ERR_NOMEM, "cpx_graph_create: out of memory");
  g->h = h;
  g->ops.assign(ops, ops + n_ops);
  g->tensors.assign(tensors, tensors + n_tensors);
  g->input = input_tensor;
  g->output = output_tensor;
  for (int i = 0; i < n_tensors; ++i) {
    const cpx_graph_tensor& t = g->tensors[i];
    const bool ext = i == input_tensor || i == output_tensor;
    // a sample is indexed in 32 bits
    if (t.H < 1 || t.W < 1 || t.C < 1 || t.c_offset < 0 || t.c_stride < t.c_offset + t.C ||
        (double)t.H * t.W * t.c_stride >= 2147483648.0 || (!ext && t.arena_offset < 0) ||
        (i == input_tensor && (t.c_offset != 0 || t.c_stride != t.C)) ||
        (t.type != CPX_GRAPH_TYPE_FLOAT32 && t.type != CPX_GRAPH_TYPE_INT8) || (ext && t.type != CPX_GRAPH_TYPE_FLOAT32)) {
      delete g;
      return fail(h, CPX_ERR_INVALID, "cpx_graph_create: bad tensor");
    }
    // (an int8 tensor's extent: its bytes rounded up to floats)
    const size_t elems = (size_t)t.H * t.W * t.c_stride;
    if (!ext) g->arena_floats = std::max(g->arena_floats, (size_t)t.arena_offset + (t.type == CPX_GRAPH_TYPE_INT8 ? (elems + 3) / 4 : elems));
  }
  for (int i = 0; i < n_ops; ++i) {
    if (const char* why = graph_check_op(g->ops[i], g->tensors, input_tensor, output_tensor)) {
      delete g;
      h->err = "cpx_graph_create: operator " + std::to_string(i) + " (kind " + std::to_string(ops[i].kind) + "): " + why;
      return CPX_ERR_INVALID;
    }
  }
  h->graphs.push_back(g);
  *out = g;
  return CPX_OK;
}

void cpx_graph_destroy(cpx_graph* g) {
  if (!g) return;
  cpx_handle* h = g->h;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  h->graphs.erase(std::remove(h->graphs.begin(), h->graphs.end(), g), h->graphs.end());
  graph_free(g);
}

int cpx_graph_arena_bytes(const cpx_graph* g, int N, size_t* bytes) {
  if (!g || !bytes || N < 0) return CPX_ERR_INVALID;
  *bytes = g->arena_floats * (size_t)N * sizeof(float);
  return CPX_OK;
}

int cpx_graph_arena_allocated(const cpx_handle* h, size_t* bytes) {
  if (!h || !bytes) return CPX_ERR_INVALID;
  *bytes = h->graph_arena.bytes;
  return CPX_OK;
}

int cpx_graph_forward(cpx_graph* g, const float* in_dev, int N, float* out_dev) {
  if (!g) return CPX_ERR_INVALID;
  cpx_handle* h = g->h;
  if (!in_dev || !out_dev || N < 1) return fail(h, CPX_ERR_INVALID, "cpx_graph_forward: bad argument");
  CPX_ENTER(h);
  if (int rc = h->graph_arena.grow(h, g->arena_floats * (size_t)N * sizeof(float), "cpx_graph_forward: arena hipMalloc"))
    return rc;
  auto view = [&](int id) {
    const cpx_graph_tensor& t = g->tensors[id];
    cpx::GraphView v{};
    v.H = t.H;
    v.W = t.W;
    v.C = t.C;
    v.cstride = t.c_stride;
    v.sample_stride = (size_t)t.H * t.W * t.c_stride;
    if (id == g->input)
      v.p = const_cast<float*>(in_dev);
    else if (id == g->output)
      v.p = out_dev + t.c_offset;
    else if (t.type == CPX_GRAPH_TYPE_INT8)   // bytes: the pointer and the sample stride count elements of one byte
      v.p = reinterpret_cast<float*>(reinterpret_cast<char*>(h->graph_arena.as<float>() + (size_t)t.arena_offset * N) + t.c_offset);
    else
      v.p = h->graph_arena.as<float>() + (size_t)t.arena_offset * N + t.c_offset;
    return v;
  };
  for (const cpx_graph_op& o : g->ops) {
    cpx::GraphOpArgs a{};
    a.kind = o.kind;
    a.N = N;
    a.in0 = view(o.in0);
    if (o.in1 >= 0) a.in1 = view(o.in1);
    a.out = view(o.out);
    a.kh = o.kh;
    a.kw = o.kw;
    a.stride_h = o.stride_h;
    a.stride_w = o.stride_w;
    a.pad_top = o.pad_top;
    a.pad_left = o.pad_left;
    a.act = o.activation;
    a.n_map = o.n_map;
    for (int c = 0; c < 4; ++c) a.map[c] = o.channel_map[c];
    a.param = o.param;
    a.weights = o.weights;
    a.scale = o.scale;
    a.shift = o.shift;
    a.in0_int8 = g->tensors[o.in0].type == CPX_GRAPH_TYPE_INT8;
    cpx::launch_graph_op(a, h->stream);
  }
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

}  // extern "C"
