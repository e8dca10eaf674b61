// cpx_api_cnn.cpp -- the WR-ResNet's entry points (include/cpx.h): one convolution (cpx_conv2d), the head, the launch timing,
// and the whole-network forward: a per-block plan (plan_block) and its executor (run_block).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <utility>
#include <vector>

#include "cpx_internal.h"

static_assert(sizeof(cpx_wrresnet_block) == 56 && sizeof(cpx_wrresnet_params) == 1560,
              "cpx_wrresnet_params layout is part of the ABI");

struct cpx_cnn {
  cpx_handle* h = nullptr;
  cpx_wrresnet_params p{};
  std::vector<std::pair<const float*, void*>> split;  // bf16 plane images of the 3x3 stride-1 weights
  // CPX_CNN_MATH_FP16X2: the power of two each 3x3 convolution's activated input is multiplied by before the fp16 split
  // ([stage][block][a / b]; 1 until cpx_cnn_set_activation_bounds says more)
  float act_scale[3][CPX_WRRESNET_MAX_BLOCKS][2];
  // CPX_CNN_MATH_FP16X2, the fused 1x1 shortcut of a stage's first block as fp16x2 products: the bound of the block's input
  // (cpx_cnn_set_residual_bounds; 0 = none given), the power of two the host chose for it (0 = this layer keeps the float32
  // side product) and the fp16 plane image of the shortcut's weights built for that scale and the layer's act_scale
  float res_bound[3] = {0.0f, 0.0f, 0.0f};
  float sc_xscale[3] = {0.0f, 0.0f, 0.0f};
  void* sc_img[3] = {nullptr, nullptr, nullptr};
  double sc_wmax[3] = {-1.0, -1.0, -1.0};  // max |shortcut weight| w_scale[c] of the stage: read back once (< 0 = not yet)
  cpx_cnn() {
    for (auto& st : act_scale)
      for (auto& b : st) b[0] = b[1] = 1.0f;
  }
  const void* split_of(const float* w) const {
    for (const auto& e : split)
      if (e.first == w) return e.second;
    return nullptr;
  }
};

void cnn_free(cpx_cnn* c) {
  for (auto& e : c->split) hipFree(e.second);
  for (void* img : c->sc_img)
    if (img) hipFree(img);
  delete c;
}

// a 1x1 shortcut convolution folded into the convolution that would have read its output as the residual
struct conv_fuse {
  const float* in = nullptr;  // [N, H, W, cin]
  const float* w = nullptr;
  const float* bias = nullptr;
  int H = 0, W = 0, cin = 0, stride = 1;
  const void* planes = nullptr;  // fp16 plane image of w for the operand scale xscale (ConvArgs::sc_planes), or none
  float xscale = 0.0f;
};

// the modes that run the split-operand kernels (16-bit planes on the bf16 / fp16 matrix pipe)
static bool split_math(const cpx_handle* h) { return h->cnn_math != CPX_CNN_MATH_F32; }
// CPX_CNN_MATH_FP16X2: what a network's forward knows about the layer and a bare cpx_conv2d does not
struct conv_half {
  float act_scale = 1.0f;   // power of two the activated input is multiplied by before the fp16 split
  bool keep_flag = false;   // the overflow word belongs to the forward in flight (cleared once, at its start)
  int word = 0;             // which overflow word: 0 = a bare convolution's, 2 + b = block b of the forward in flight
  // producer-side split between a block's two convolutions (cpx_cnn_forward decides; ConvArgs::out_planes / in_planes)
  bool out_planes = false;  // store the output as the next layer's fp16 planes, scaled by out_act_scale
  float out_act_scale = 1.0f;
  bool in_planes = false;   // the input is in that form
  // the fp16 work of this layer was done by a fused block launch (conv_block32_kernel): only the guarded three-plane
  // rerun is launched, and no timing record is taken (the block launch has its own)
  bool rerun_only = false;
};
// the handle's overflow words: [0] the last bare convolution's / whether the last forward raised any, [1] forwards that did,
// [2 + b] block b of the forward in flight.  One word per BLOCK, not per forward: an activation out of fp16's range sends
// the rest of ITS block (the two convolutions hand fp16 planes to each other) to the bf16x3 kernels; the next block is
// back on the fp16 ones
constexpr int OVF_WORDS = 2 + 3 * CPX_WRRESNET_MAX_BLOCKS;
static int ensure_ovf_word(cpx_handle* h) {
  if (h->cnn_ovf.p) return CPX_OK;
  if (int rc = h->cnn_ovf.grow(h, OVF_WORDS * sizeof(int), "cpx_conv2d: overflow word allocation failed")) return rc;
  CPX_HIP(h, hipMemsetAsync(h->cnn_ovf.p, 0, OVF_WORDS * sizeof(int), h->stream));
  return CPX_OK;
}
// One convolution's geometry from its shape: TensorFlow SAME (out = ceil(in / stride), surplus padding goes to the bottom /
// right) or VALID (the caller has refused an input smaller than the kernel).  This shape-only form is what the kernels'
// predicates are asked with (conv_bf3_supported and its kin read nothing else); a layer that has no map yet passes N = H = W = 0
static cpx::ConvArgs conv_shape(int N, int H, int W, int Cin, int Cout, int groups, int ksize, int stride, int pad_same) {
  cpx::ConvArgs a{};
  a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.groups = groups; a.ksize = ksize; a.stride = stride;
  if (pad_same) {
    a.Ho = (H + stride - 1) / stride;
    a.Wo = (W + stride - 1) / stride;
    a.pad_top = std::max((a.Ho - 1) * stride + ksize - H, 0) / 2;
    a.pad_left = std::max((a.Wo - 1) * stride + ksize - W, 0) / 2;
  } else {
    a.Ho = (H - ksize) / stride + 1;
    a.Wo = (W - ksize) / stride + 1;
  }
  return a;
}
// ... and the whole launch: the descriptor's pointers, and the 1x1 shortcut folded into it
static cpx::ConvArgs conv_describe(const cpx_conv_desc& d, const conv_fuse* fuse = nullptr) {
  cpx::ConvArgs a = conv_shape(d.N, d.H, d.W, d.Cin, d.Cout, d.groups, d.ksize, d.stride, d.pad_same);
  a.relu = d.relu;
  a.in = d.in_dev; a.out = d.out_dev; a.weights = d.weights_dev;
  a.in_scale = d.in_scale_dev; a.in_shift = d.in_shift_dev;
  a.out_scale = d.out_scale_dev; a.out_shift = d.out_shift_dev; a.residual = d.residual_dev;
  if (fuse) {
    a.sc_in = fuse->in; a.sc_w = fuse->w; a.sc_bias = fuse->bias;
    a.sc_H = fuse->H; a.sc_W = fuse->W; a.sc_cin = fuse->cin; a.sc_stride = fuse->stride;
    a.sc_planes = fuse->planes; a.sc_xscale = fuse->xscale;
  }
  return a;
}

// The two events of one conv_timing record.  Timing on: both are created and the first recorded here; commit() records the
// second and hands the pair to the handle.  Dropped uncommitted (an early return, a launch that was not taken) they are destroyed.
class ConvTimer {
 public:
  ConvTimer(cpx_handle* h, bool on) : h_(h) {
    if (!on) return;
    ok_ = hipEventCreate(&ev_.e0) == hipSuccess && hipEventCreate(&ev_.e1) == hipSuccess &&
          hipEventRecord(ev_.e0, h->stream) == hipSuccess;
  }
  ~ConvTimer() {
    if (ev_.e0) hipEventDestroy(ev_.e0);
    if (ev_.e1) hipEventDestroy(ev_.e1);
  }
  ConvTimer(const ConvTimer&) = delete;
  ConvTimer& operator=(const ConvTimer&) = delete;
  bool ok() const { return ok_; }
  int commit(int key, double flops) {
    if (!ev_.e0) return CPX_OK;
    CPX_HIP(h_, hipEventRecord(ev_.e1, h_->stream));
    ev_.key = key;
    ev_.flops = flops;
    h_->conv_events.push_back(ev_);
    ev_ = {};
    return CPX_OK;
  }

 private:
  cpx_handle* h_;
  cpx_handle::ConvEv ev_{};
  bool ok_ = true;
};

// how one convolution is launched
enum class ConvRoute {
  Float32,    // the float32 kernel
  Split,      // the split-operand kernel on bf16 planes (three, or two in bf16x2)
  Fp16Pair,   // fp16x2: the fp16 launch, then the same layer on three bf16 planes guarded by the overflow word
  RerunOnly,  // a fused block launch did the fp16 work: the guarded launch alone (whichever kernel has the layer), untimed
};

// split_weights: the bf16 plane image of d->weights_dev if the caller (a cpx_cnn) keeps one, else NULL
static int conv_run(cpx_handle* h, const cpx_conv_desc* d, const void* split_weights, const conv_fuse* fuse = nullptr,
                    const conv_half* hf = nullptr) {
  // ---- validate and describe
  if (!h) return CPX_ERR_INVALID;
  if (!d || !d->in_dev || !d->out_dev || !d->weights_dev) return fail(h, CPX_ERR_INVALID, "cpx_conv2d: null argument");
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->groups < 1 || d->Cin % d->groups || d->Cout % d->groups ||
      d->ksize < 1 || d->stride < 1 || (d->in_scale_dev == nullptr) != (d->in_shift_dev == nullptr))
    return fail(h, CPX_ERR_INVALID, "cpx_conv2d: bad descriptor");
  CPX_ENTER(h);
  if (!d->pad_same && (d->H < d->ksize || d->W < d->ksize)) return fail(h, CPX_ERR_INVALID, "cpx_conv2d: input smaller than kernel");
  cpx::ConvArgs a = conv_describe(*d, fuse);
  const bool split = split_math(h) && cpx::conv_bf3_supported(a);
  if (fuse && (!split || a.out_scale || a.residual))
    return fail(h, CPX_ERR_INVALID, "conv_run: shortcut fusion needs the split-operand kernel, no output scale, no residual");
  if (split) a.planes = h->cnn_math == CPX_CNN_MATH_BF16X2 ? 2 : 3;
  // ---- choose the route
  const conv_half bare;  // (a bare cpx_conv2d: scale 1, overflow word 0)
  const conv_half& k = hf ? *hf : bare;
  // fp16x2: the two-plane layers run on fp16 planes, with the three-plane kernel launched behind as the guarded
  // rerun (it returns at once unless a scaled activation left fp16's range); every other layer as bf16x3
  // (an output that aliases the residual or the input -- an in-place add -- must not be written twice: the guarded
  // rerun would read what the fp16 pass has already stored.  Such a call runs bf16x3 directly.)
  const bool fp16 = split && h->cnn_math == CPX_CNN_MATH_FP16X2;
  const bool aliased = a.out == a.residual || a.out == a.in;
  const bool half = fp16 && cpx::conv_bf3_two_planes(a) && !aliased;
  const bool planes_out = fp16 && k.out_planes;  // (the three-plane kernel can store the next layer's fp16 planes too)
  const ConvRoute route = k.rerun_only ? ConvRoute::RerunOnly  // (any layer: the 8-channel one of a fused first block, conv1_1 behind it)
                          : !split ? ConvRoute::Float32
                          : (half || planes_out) ? ConvRoute::Fp16Pair
                                                 : ConvRoute::Split;
  ConvTimer timer(h, h->conv_timing && route != ConvRoute::RerunOnly);
  if (!timer.ok()) return fail(h, CPX_ERR_HIP, "cpx_conv2d: event creation failed");
  // ---- prepare what the route needs: the overflow word, the weight image
  int* word = nullptr;
  if (route == ConvRoute::Fp16Pair || route == ConvRoute::RerunOnly) {
    if (int rc = ensure_ovf_word(h)) return rc;
    if (!k.keep_flag) CPX_HIP(h, hipMemsetAsync(h->cnn_ovf.p, 0, sizeof(int), h->stream));
    word = h->cnn_ovf.as<int>() + k.word;
  }
  if (split && !split_weights) {
    if (int rc = h->bf3_scratch.grow(h, cpx::conv_bf3_weight_bytes(a), "cpx_conv2d: weight scratch allocation failed"))
      return rc;
    cpx::launch_split_weights(a, h->bf3_scratch.p, h->stream);
    split_weights = h->bf3_scratch.p;
  }
  // ---- launch
  int rc = 0;
  if (route == ConvRoute::Fp16Pair) {
    cpx::ConvArgs first = a;
    if (half) {
      first.planes = 2;
      first.half = 1;
      first.act_scale = k.act_scale;
      first.act_unscale = 1.0f / first.act_scale;  // (a power of two: exact)
      first.in_planes = k.in_planes;
      first.flat16 = h->flat16;
    }
    first.ovf = word;
    if (planes_out) {
      first.out_planes = 1;
      first.out_act_scale = k.out_act_scale;
    }
    rc = cpx::launch_conv_bf3(first, split_weights, h->stream);
  }
  a.guard = word;  // (Fp16Pair, RerunOnly: this launch returns at once while the word is clear)
  if (split) {
    if (rc == 0) rc = cpx::launch_conv_bf3(a, split_weights, h->stream);
    if (rc == -3) {  // more tiles than the split-operand kernel's tile decomposition indexes: float32 path
      // the float32 kernel has no fused shortcut: dropping it silently would lose the block's shortcut branch
      if (fuse) return fail(h, CPX_ERR_UNSUPPORTED, "conv_run: batch too large for the fused-shortcut kernel (split the call)");
      rc = cpx::launch_conv(a, h->stream);
    }
  } else {
    rc = cpx::launch_conv(a, h->stream);
  }
  if (int trc = timer.commit((a.Cin / a.groups) * 10000 + (a.Cout / a.groups) * 10 + a.stride + (a.ksize == 1 ? 5 : 0),
                             2.0 * a.N * a.Ho * a.Wo * a.Cout * (double)(a.Cin / a.groups) * a.ksize * a.ksize))
    return trc;
  if (rc == -2) return fail(h, CPX_ERR_UNSUPPORTED, "cpx_conv2d: no kernel for this (channels per group, stride, kernel size)");
  if (rc != 0) return fail(h, CPX_ERR_HIP, "cpx_conv2d: kernel configuration failed");
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

// the 3x3 stride-1 convolution of f channels runs on the split-operand kernel (which can absorb a 1x1 shortcut)
static bool conv_can_fuse(const cpx_handle* h, int f, int groups) {
  return split_math(h) && cpx::conv_bf3_supported(conv_shape(0, 0, 0, f, f, groups, 3, 1, 1));
}

// ---- whole-network forward: decide per block (plan_block), then launch (run_block) -----------------------------------
// what a residual block's two 3x3 convolutions run as
enum class BlockForm {
  OneLaunch,   // fp16x2: the fused block kernel (conv_block32_kernel: `mid` stays in LDS); the convolutions follow as guarded reruns
  PlanesPair,  // fp16x2: two launches, `mid` travels as the second one's scaled fp16 planes (same bytes as float32)
  Separate,    // two launches, `mid` in float32
};
enum class Shortcut {
  Identity,         // the block's input is the residual
  FusedIntoSecond,  // a stage's first block: the 1x1 shortcut inside the second convolution's kernel
  OwnLaunch,        // ... or a launch of its own, its output the residual
};
// where the network's first convolution runs: said by the plan of the first block, which reads it
enum class Conv1 {
  NotHere,      // (every later block)
  InFront,      // a launch of its own in front of the block
  InsideBlock,  // the block kernel computes it while it stages its patch (conv_block32_kernel<true, true>); its own launch is
                // the guarded head of that block's rerun, which is all that reads the tensor
};
// how far a plan may fuse: lowered, block by block, where the launcher declines what was planned (downgrade)
enum class Fusion { None, Block, BlockAndConv1 };

struct BlockPlan {
  int k, st, d;                          // block k = d of stage st
  int stride, H, W, Ho, Wo, c_in, f;     // both convolutions are 3x3 SAME: c_in -> f at `stride`, f -> f at 1
  int word;                              // its overflow word
  BlockForm form;
  Shortcut shortcut;
  bool shortcut_fp16;                    // FusedIntoSecond: its products on the fp16 matrix pipe (the network has the scaled image)
  Conv1 conv1;
};

// what the launches of one forward share
struct Forward {
  cpx_cnn* cnn;
  cpx_handle* h;
  const float* in;
  int N, H, W;
  float *act[2], *mid, *sc;  // block k reads act[k & 1] and writes act[(k + 1) & 1]
};

static cpx_conv_desc layer_desc(const Forward& fw, const float* in, float* out, const float* w, int H, int W, int cin, int cout,
                                int ksize, int stride, int same, int relu) {
  cpx_conv_desc d{};
  d.N = fw.N; d.H = H; d.W = W; d.Cin = cin; d.Cout = cout; d.groups = fw.cnn->p.groups; d.ksize = ksize; d.stride = stride;
  d.pad_same = same; d.relu = relu;
  d.in_dev = in; d.out_dev = out; d.weights_dev = w;
  return d;
}

// a block's layers as cpx_conv2d would take them: first convolution, 1x1 shortcut (as a launch, and as the second convolution
// folds it in), second convolution
struct BlockLayers {
  cpx_conv_desc a, sc, b;
  conv_fuse fuse;
};
static BlockLayers block_layers(const Forward& fw, const BlockPlan& bp) {
  const cpx_wrresnet_params& p = fw.cnn->p;
  const cpx_wrresnet_block& b = p.block[bp.st][bp.d];
  const float* cur = fw.act[bp.k & 1];
  BlockLayers l{};
  l.a = layer_desc(fw, cur, fw.mid, b.wa, bp.H, bp.W, bp.c_in, bp.f, 3, bp.stride, 1, 1);
  l.a.in_scale_dev = b.in_scale; l.a.in_shift_dev = b.in_shift; l.a.out_scale_dev = b.a_scale; l.a.out_shift_dev = b.a_shift;
  l.sc = layer_desc(fw, cur, fw.sc, p.shortcut_w[bp.st], bp.H, bp.W, bp.c_in, bp.f, 1, bp.stride, 0, 0);
  l.sc.out_shift_dev = p.shortcut_b[bp.st];
  l.fuse.in = cur; l.fuse.w = p.shortcut_w[bp.st]; l.fuse.bias = p.shortcut_b[bp.st];
  l.fuse.H = bp.H; l.fuse.W = bp.W; l.fuse.cin = bp.c_in; l.fuse.stride = bp.stride;
  if (bp.shortcut_fp16) {
    l.fuse.planes = fw.cnn->sc_img[bp.st];
    l.fuse.xscale = fw.cnn->sc_xscale[bp.st];
  }
  l.b = layer_desc(fw, fw.mid, fw.act[(bp.k + 1) & 1], b.wb, bp.Ho, bp.Wo, bp.f, bp.f, 3, 1, 1, 1);
  l.b.out_shift_dev = b.bb;
  l.b.residual_dev = bp.shortcut == Shortcut::Identity ? cur : bp.shortcut == Shortcut::OwnLaunch ? fw.sc : nullptr;
  return l;
}
// ... and its two convolutions as the fused block kernel takes them (launch_conv_block32)
static void block32_args(const Forward& fw, const BlockPlan& bp, cpx::ConvArgs* ca, cpx::ConvArgs* cb) {
  const BlockLayers l = block_layers(fw, bp);
  *ca = conv_describe(l.a);
  *cb = conv_describe(l.b, bp.shortcut == Shortcut::FusedIntoSecond ? &l.fuse : nullptr);
  cpx::ConvArgs* both[2] = {ca, cb};
  for (int i = 0; i < 2; ++i) {
    both[i]->planes = 2;
    both[i]->half = 1;
    both[i]->ovf = fw.h->cnn_ovf.as<int>() + bp.word;
    both[i]->act_scale = fw.cnn->act_scale[bp.st][bp.d][i];
    both[i]->act_unscale = 1.0f / both[i]->act_scale;
  }
  if (bp.conv1 == Conv1::InsideBlock) {
    ca->c1_in = fw.in; ca->c1_w = fw.cnn->p.conv1_w; ca->c1_b = fw.cnn->p.conv1_b;
  }
}

// The launches of block k, whose input is an H x W map, under the handle's math mode and switches.  Reads nothing an
// earlier block decided, enqueues nothing.  (Whether the launcher takes a OneLaunch block is its own to say at launch
// time -- its tile counts: downgrade.)
static BlockPlan plan_block(const Forward& fw, int k, int H, int W, Fusion most) {
  const cpx_handle* h = fw.h;
  const cpx_cnn* cnn = fw.cnn;
  const cpx_wrresnet_params& p = cnn->p;
  const int g = p.groups;
  BlockPlan bp{};
  bp.k = k; bp.st = k / p.blocks_per_stage; bp.d = k % p.blocks_per_stage;
  const cpx_wrresnet_block& b = p.block[bp.st][bp.d];
  bp.stride = bp.d == 0 ? bp.st + 1 : 1;  // wr_block(stride = stage index), wr_resnet.py:27-30
  bp.c_in = p.filters[bp.d == 0 ? bp.st : bp.st + 1];
  bp.f = p.filters[bp.st + 1];
  const cpx::ConvArgs first = conv_shape(fw.N, H, W, bp.c_in, bp.f, g, 3, bp.stride, 1);
  const cpx::ConvArgs second = conv_shape(fw.N, first.Ho, first.Wo, bp.f, bp.f, g, 3, 1, 1);
  bp.H = H; bp.W = W; bp.Ho = first.Ho; bp.Wo = first.Wo;
  bp.word = 2 + k;
  const bool fp16 = h->cnn_math == CPX_CNN_MATH_FP16X2, whole_groups = bp.c_in % g == 0 && bp.f % g == 0;
  // the 1x1 shortcut of a stage's first block: folded into the block's second convolution when that one runs on the
  // split-operand kernel (saves writing and re-reading the shortcut tensor), a launch of its own otherwise
  // (the kernels' fused shortcut walks K in fours -- conv_bf3w_kernel -- or in twos: a block input with 2, 6, 10 ...
  // channels per group keeps the shortcut as a launch of its own rather than depending on which kernel takes the layer)
  bp.shortcut = bp.d != 0 ? Shortcut::Identity
                : (h->fuse_shortcut && conv_can_fuse(h, bp.f, g) && (bp.c_in / g) % 4 == 0) ? Shortcut::FusedIntoSecond
                                                                                          : Shortcut::OwnLaunch;
  // fp16x2: the fused shortcut's products run on fp16 planes where a residual bound was given and the host found scales
  // for this layer (update_shortcut_images); CPX_CNN_SHORTCUT_FP16=0, or no bound: the float32 side product
  bp.shortcut_fp16 = bp.shortcut == Shortcut::FusedIntoSecond && fp16 && h->shortcut_fp16 && cnn->sc_xscale[bp.st] > 0.0f &&
                     cnn->sc_img[bp.st] != nullptr;
  // fp16x2: a block whose two convolutions are stride-1 with 32 channels per group (stage 2 past its first block) is ONE
  // launch; the stage's first block too (8 input channels per group; its 1x1 shortcut inside the second convolution) ...
  const bool first8 = bp.d == 0 && bp.stride == 1 && bp.c_in / g == 8 && h->block_fusion >= 2 && h->fuse_shortcut;
  bool one_launch = most != Fusion::None && fp16 && h->block_fusion && bp.stride == 1 &&
                    ((bp.d != 0 && bp.c_in == bp.f) || first8) && b.in_scale && cnn->split_of(b.wa) && cnn->split_of(b.wb) &&
                    whole_groups;
  if (one_launch) {
    cpx::ConvArgs ca, cb;
    block32_args(fw, bp, &ca, &cb);
    one_launch = cpx::conv_block32_supported(ca, cb);
  }
  // ... and that one with conv1_1 inside, where the network's first convolution is the shape the kernel restates
  const bool c1_inside = one_launch && most == Fusion::BlockAndConv1 && k == 0 && first8 && h->fuse_conv1 && g == 2 &&
                         p.in_channels == 2 && p.filters[0] == 16;
  bp.conv1 = k != 0 ? Conv1::NotHere : c1_inside ? Conv1::InsideBlock : Conv1::InFront;
  // fp16x2, two launches: where the first convolution's kernel can store fp16 planes and the second one's can stage them,
  // `mid` travels as the second convolution's scaled planes and its staging is a copy
  const bool planes = fp16 && whole_groups && cpx::conv_bf3_can_store_planes(first) && cpx::conv_bf3_two_planes(second) &&
                      cpx::conv_bf3_can_load_planes(second);
  bp.form = one_launch ? BlockForm::OneLaunch : planes ? BlockForm::PlanesPair : BlockForm::Separate;
  return bp;
}

static int run_layer(const Forward& fw, const cpx_conv_desc& d, const conv_half& hf, const conv_fuse* fuse = nullptr) {
  return conv_run(fw.h, &d, fw.cnn->split_of(d.weights_dev), fuse, &hf);
}
// what every layer of the forward says of the overflow words: they are the forward's (cleared once, at its start)
static conv_half forward_half(int word, bool rerun_only) {
  conv_half hf;
  hf.keep_flag = true;
  hf.word = word;
  hf.rerun_only = rerun_only;
  return hf;
}

static int run_conv1(const Forward& fw, const conv_half& hf) {
  const cpx_wrresnet_params& p = fw.cnn->p;
  cpx_conv_desc d = layer_desc(fw, fw.in, fw.act[0], p.conv1_w, fw.H, fw.W, p.in_channels, p.filters[0], 3, 1, 1, 0);
  d.out_shift_dev = p.conv1_b;
  return run_layer(fw, d, hf);
}

// PlanesPair (planes), Separate, and the rerun of OneLaunch (rerun_only: guarded, behind the block launch that did the fp16
// work; it hands float32 over): first convolution, the 1x1 shortcut where it is a launch of its own, second convolution
static int run_layers(const Forward& fw, const BlockPlan& bp, bool planes, bool rerun_only) {
  const BlockLayers l = block_layers(fw, bp);
  const float* act_scale = fw.cnn->act_scale[bp.st][bp.d];
  const conv_half hf = forward_half(bp.word, rerun_only);
  conv_half ha = hf, hb = hf;
  ha.act_scale = act_scale[0];
  ha.out_planes = planes;
  ha.out_act_scale = act_scale[1];
  hb.act_scale = act_scale[1];
  hb.in_planes = planes;
  if (int rc = run_layer(fw, l.a, ha)) return rc;
  if (bp.shortcut == Shortcut::OwnLaunch)
    if (int rc = run_layer(fw, l.sc, hf)) return rc;
  return run_layer(fw, l.b, hb, bp.shortcut == Shortcut::FusedIntoSecond ? &l.fuse : nullptr);
}

// OneLaunch: the block kernel, then the guarded rerun -- conv1_1 at its head when the kernel computed it.
// *declined: the launcher's code when it does not take the block (nothing was launched then)
static int run_one_launch(const Forward& fw, const BlockPlan& bp, int* declined) {
  cpx_handle* h = fw.h;
  const cpx_wrresnet_params& p = fw.cnn->p;
  const cpx_wrresnet_block& b = p.block[bp.st][bp.d];
  const int g = p.groups;
  cpx::ConvArgs ca, cb;
  block32_args(fw, bp, &ca, &cb);
  ConvTimer timer(h, h->conv_timing);
  if (!timer.ok()) return fail(h, CPX_ERR_HIP, "cpx_cnn_forward: event creation failed");
  *declined = cpx::launch_conv_block32(ca, cb, fw.cnn->split_of(b.wa), fw.cnn->split_of(b.wb), h->stream);
  if (*declined) return CPX_OK;
  // ("stride 4": a fused block; both convolutions' products -- and conv1_1's when it is computed inside --, the shortcut's not counted)
  double flops = 2.0 * fw.N * bp.H * bp.W * bp.f * ((double)(bp.c_in / g) + (double)(bp.f / g)) * 9;
  if (bp.conv1 == Conv1::InsideBlock) flops += 2.0 * fw.N * bp.H * bp.W * bp.c_in * (double)(p.in_channels / g) * 9;
  if (int rc = timer.commit((bp.c_in / g) * 10000 + 32 * 10 + 4, flops)) return rc;
  if (bp.conv1 == Conv1::InsideBlock)
    if (int rc = run_conv1(fw, forward_half(bp.word, true))) return rc;
  return run_layers(fw, bp, false, true);
}

// The one place a plan changes after it was made: the launcher declined a OneLaunch block (launch_conv_block32: -2 = not
// a form it has, -3 = more tiles or pixels than it indexes).  With conv1_1 inside, whatever the code: conv1_1 as a launch
// of its own, then the block once more without it.  Otherwise, on -2 / -3: the convolutions as launches of their own; any
// other code is an error.
static int downgrade(const Forward& fw, BlockPlan* bp, int declined) {
  if (bp->conv1 == Conv1::InsideBlock) {
    *bp = plan_block(fw, bp->k, bp->H, bp->W, Fusion::Block);
    return run_conv1(fw, forward_half(0, false));
  }
  if (declined != -2 && declined != -3) return fail(fw.h, CPX_ERR_HIP, "cpx_cnn_forward: block kernel configuration failed");
  *bp = plan_block(fw, bp->k, bp->H, bp->W, Fusion::None);
  return CPX_OK;
}

static int run_block(const Forward& fw, BlockPlan bp) {
  if (bp.conv1 == Conv1::InFront)
    if (int rc = run_conv1(fw, forward_half(0, false))) return rc;
  while (bp.form == BlockForm::OneLaunch) {
    int declined = 0;
    if (int rc = run_one_launch(fw, bp, &declined)) return rc;
    if (!declined) return CPX_OK;
    if (int rc = downgrade(fw, &bp, declined)) return rc;
  }
  return run_layers(fw, bp, bp.form == BlockForm::PlanesPair, false);
}

// The fused shortcuts on the fp16 pipe, decided per layer on the host whenever a bound changes (cpx_cnn_set_residual_bounds,
// cpx_cnn_set_activation_bounds): for each stage whose first block's second convolution can take the shortcut as fp16x2
// products (conv_shortcut_planes_layer) and whose input has a bound, the largest scaled shortcut weight is read back, a power
// of two for the operand is chosen (cpx_cnn_shortcut_scale) and the weights' fp16 plane image is built for it.  A layer
// without a bound, or for which no power of two fits, keeps sc_xscale = 0: the float32 side product.
static int update_shortcut_images(cpx_cnn* cnn) {
  cpx_handle* h = cnn->h;
  const cpx_wrresnet_params& p = cnn->p;
  CPX_ENTER(h);
  for (int st = 0; st < 3; ++st) {
    cnn->sc_xscale[st] = 0.0f;
    const int g = p.groups, c_in = p.filters[st], f = p.filters[st + 1];
    if (!(cnn->res_bound[st] > 0.0f) || c_in % g || f % g) continue;
    cpx::ConvArgs second = conv_shape(0, 0, 0, f, f, g, 3, 1, 1);
    second.weights = p.block[st][0].wb;
    const void* wimg = cnn->split_of(second.weights);
    if (!wimg || !cpx::conv_shortcut_planes_layer(second, c_in / g)) continue;
    const int cin_g = c_in / g, cout_g = f / g;
    const float* w_scale_dev = cpx::conv_bf3_weight_scales(second, wimg);
    if (cnn->sc_wmax[st] < 0.0) {  // the weights are constant for the life of the network: one read-back per stage
      std::vector<float> ws((size_t)f), w((size_t)g * cin_g * cout_g);
      CPX_HIP(h, hipStreamSynchronize(h->stream));  // (the scales were written on the stream when the network was created)
      CPX_HIP(h, hipMemcpy(ws.data(), w_scale_dev, ws.size() * sizeof(float), hipMemcpyDeviceToHost));
      CPX_HIP(h, hipMemcpy(w.data(), p.shortcut_w[st], w.size() * sizeof(float), hipMemcpyDeviceToHost));
      double m = 0.0;
      for (int gi = 0; gi < g; ++gi)
        for (int k = 0; k < cin_g; ++k)
          for (int c = 0; c < cout_g; ++c)
            m = std::max(m, std::fabs((double)w[((size_t)gi * cin_g + k) * cout_g + c]) * ws[gi * cout_g + c]);
      cnn->sc_wmax[st] = m;
    }
    const float act_scale = cnn->act_scale[st][0][1];
    const double wmax = cnn->sc_wmax[st] * act_scale;  // the largest shortcut weight as the accumulators are scaled
    float sx = 0.0f;
    if (!cpx_cnn_shortcut_scale(cnn->res_bound[st], (float)wmax, &sx)) continue;
    if (!cnn->sc_img[st] && hipMalloc(&cnn->sc_img[st], cpx::conv_shortcut_image_bytes(g, cin_g, cout_g)) != hipSuccess) {
      (void)hipGetLastError();
      cnn->sc_img[st] = nullptr;
      return fail(h, CPX_ERR_NOMEM, "cpx_cnn_set_residual_bounds: shortcut image allocation failed");
    }
    cpx::launch_split_shortcut(p.shortcut_w[st], cnn->sc_img[st], g, cin_g, cout_g, w_scale_dev, act_scale / sx, h->stream);
    CPX_HIP(h, hipGetLastError());
    cnn->sc_xscale[st] = sx;
  }
  return CPX_OK;
}

// cpx_cnn_forward and cpx_cnn_forward_taps: the same launches; with taps != nullptr each residual block's final output is
// also copied to taps[stage * blocks_per_stage + d] and, when ovf_out != nullptr, the blocks' overflow words to ovf_out
static int cnn_forward(cpx_cnn* cnn, const float* in_dev, int N, int H, int W, float* logits_dev, float* probs_dev,
                       float* const* taps, int* ovf_out) {
  cpx_handle* h = cnn->h;
  CPX_ENTER(h);
  const cpx_wrresnet_params& p = cnn->p;
  if (h->cnn_math == CPX_CNN_MATH_FP16X2) {  // the blocks' overflow words start clear
    const int rco = ensure_ovf_word(h);
    if (rco != CPX_OK) return rco;
    CPX_HIP(h, hipMemsetAsync(h->cnn_ovf.as<int>() + 2, 0, (OVF_WORDS - 2) * sizeof(int), h->stream));
  }
  // largest activation: conv1 output (and the stage-2 tensors at stride 1)
  size_t biggest = 0;
  {
    int hh = H, ww = W;
    biggest = (size_t)N * hh * ww * p.filters[0];
    for (int st = 0; st < 3; ++st) {
      const int s = st + 1;
      hh = (hh + s - 1) / s;
      ww = (ww + s - 1) / s;
      biggest = std::max(biggest, (size_t)N * hh * ww * p.filters[st + 1]);
    }
  }
  biggest = align_up(biggest, 64);
  if (int rc = h->cnn_arena.grow(h, 4 * biggest * sizeof(float), "cpx_cnn_forward: activation hipMalloc")) return rc;
  float* const arena = h->cnn_arena.as<float>();
  const Forward fw{cnn, h, in_dev, N, H, W, {arena, arena + biggest}, arena + 2 * biggest, arena + 3 * biggest};
  // decide ...
  const int n_blocks = 3 * p.blocks_per_stage;
  BlockPlan plan[3 * CPX_WRRESNET_MAX_BLOCKS];
  int hh = H, ww = W;
  for (int k = 0; k < n_blocks; ++k) {
    plan[k] = plan_block(fw, k, hh, ww, Fusion::BlockAndConv1);
    hh = plan[k].Ho;
    ww = plan[k].Wo;
  }
  // ... then launch
  for (int k = 0; k < n_blocks; ++k) {
    if (int brc = run_block(fw, plan[k])) return brc;
    if (taps)  // (behind the block's guarded rerun launches: what the next block reads)
      CPX_HIP(h, hipMemcpyAsync(taps[k], fw.act[(k + 1) & 1], (size_t)N * plan[k].Ho * plan[k].Wo * plan[k].f * sizeof(float),
                                hipMemcpyDeviceToDevice, h->stream));
  }
  const float* cur = fw.act[n_blocks & 1];
  const int c_in = plan[n_blocks - 1].f;
  cpx_head_desc hd{};
  hd.N = N; hd.HW = hh * ww; hd.C = c_in; hd.L = p.n_labels;
  hd.n_hidden = p.n_hidden;
  hd.activation = p.activation;
  for (int k = 0; k < p.n_hidden; ++k) {
    hd.hidden_sizes[k] = p.hidden_sizes[k];
    hd.hidden_w_dev[k] = p.hidden_w[k];
    hd.hidden_b_dev[k] = p.hidden_b[k];
  }
  hd.in_dev = cur; hd.bn_scale_dev = p.final_scale; hd.bn_shift_dev = p.final_shift;
  hd.dense_w_dev = p.dense_w; hd.dense_b_dev = p.dense_b; hd.logits_dev = logits_dev; hd.probs_dev = probs_dev;
  int rc = cpx_cnn_head_ex(h, &hd);
  if (rc == CPX_OK && h->cnn_math == CPX_CNN_MATH_FP16X2)
    cpx::launch_count_overflow(h->cnn_ovf.as<int>(), 3 * p.blocks_per_stage, h->stream);
  if (rc == CPX_OK && ovf_out) {
    const size_t bytes = (size_t)3 * p.blocks_per_stage * sizeof(int);
    if (h->cnn_math == CPX_CNN_MATH_FP16X2)
      CPX_HIP(h, hipMemcpyAsync(ovf_out, h->cnn_ovf.as<int>() + 2, bytes, hipMemcpyDeviceToDevice, h->stream));
    else  // (no fp16 launch: no block was rerun)
      CPX_HIP(h, hipMemsetAsync(ovf_out, 0, bytes, h->stream));
  }
  if (rc == CPX_OK && h->cnn_math == CPX_CNN_MATH_FP16X2 && std::getenv("CPX_CNN_DEBUG_OVF")) {
    // diagnostic (synchronises): which blocks of this forward left fp16's range
    int words[OVF_WORDS];
    if (hipStreamSynchronize(h->stream) == hipSuccess &&
        hipMemcpy(words, h->cnn_ovf.p, sizeof(words), hipMemcpyDeviceToHost) == hipSuccess && words[0]) {
      std::fprintf(stderr, "cpx_cnn_forward: N = %d, fp16 overflow in blocks", N);
      for (int k = 0; k < 3 * p.blocks_per_stage; ++k)
        if (words[2 + k]) std::fprintf(stderr, " %d.%d", k / p.blocks_per_stage + 2, k % p.blocks_per_stage);
      std::fprintf(stderr, "\n");
    }
  }
  return rc;
}

extern "C" {

int cpx_conv2d(cpx_handle* h, const cpx_conv_desc* d) { return conv_run(h, d, nullptr); }

int cpx_set_cnn_math(cpx_handle* h, int mode) {
  if (!h) return CPX_ERR_INVALID;
  if (mode != CPX_CNN_MATH_F32 && mode != CPX_CNN_MATH_BF16X3 && mode != CPX_CNN_MATH_BF16X2 && mode != CPX_CNN_MATH_FP16X2)
    return fail(h, CPX_ERR_INVALID, "cpx_set_cnn_math: unknown mode");
  h->cnn_math = mode;
  return CPX_OK;
}
int cpx_get_cnn_math(const cpx_handle* h) { return h ? h->cnn_math : CPX_ERR_INVALID; }

int cpx_cnn_overflow_forwards(cpx_handle* h, int* count, int reset) {
  if (!h) return CPX_ERR_INVALID;
  if (!count) return fail(h, CPX_ERR_INVALID, "cpx_cnn_overflow_forwards: null argument");
  CPX_ENTER(h);
  *count = 0;
  if (!h->cnn_ovf.p) return CPX_OK;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  CPX_HIP(h, hipMemcpy(count, h->cnn_ovf.as<int>() + 1, sizeof(int), hipMemcpyDeviceToHost));
  if (reset) CPX_HIP(h, hipMemset(h->cnn_ovf.as<int>() + 1, 0, sizeof(int)));
  return CPX_OK;
}

int cpx_cnn_last_overflow(cpx_handle* h, int* overflowed) {
  if (!h) return CPX_ERR_INVALID;
  if (!overflowed) return fail(h, CPX_ERR_INVALID, "cpx_cnn_last_overflow: null argument");
  CPX_ENTER(h);
  *overflowed = 0;
  if (!h->cnn_ovf.p) return CPX_OK;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  CPX_HIP(h, hipMemcpy(overflowed, h->cnn_ovf.p, sizeof(int), hipMemcpyDeviceToHost));
  return CPX_OK;
}

int cpx_cnn_head_ex(cpx_handle* h, const cpx_head_desc* d) {
  if (!h) return CPX_ERR_INVALID;
  if (!d || !d->in_dev || !d->bn_scale_dev || !d->bn_shift_dev || !d->dense_w_dev || !d->dense_b_dev || !d->logits_dev ||
      d->N < 1 || d->HW < 1 || d->C < 1 || d->L < 1 || d->C > 8192 || d->L > 8192 || d->n_hidden < 0 ||
      d->n_hidden > CPX_HEAD_MAX_HIDDEN || (d->activation != CPX_HEAD_SIGMOID && d->activation != CPX_HEAD_SOFTMAX))
    return fail(h, CPX_ERR_INVALID, "cpx_cnn_head: bad argument");
  CPX_ENTER(h);
  cpx::HeadArgs a{};
  a.N = d->N; a.HW = d->HW; a.C = d->C; a.L = d->L;
  a.n_hidden = d->n_hidden;
  a.activation = d->activation;
  for (int k = 0; k < d->n_hidden; ++k) {
    if (!d->hidden_w_dev[k] || !d->hidden_b_dev[k] || d->hidden_sizes[k] < 1 || d->hidden_sizes[k] > 2048)
      return fail(h, CPX_ERR_INVALID, "cpx_cnn_head: bad hidden layer");
    a.hidden_sizes[k] = d->hidden_sizes[k];
    a.hidden_w[k] = d->hidden_w_dev[k];
    a.hidden_b[k] = d->hidden_b_dev[k];
  }
  a.in = d->in_dev; a.bn_scale = d->bn_scale_dev; a.bn_shift = d->bn_shift_dev;
  a.dense_w = d->dense_w_dev; a.dense_b = d->dense_b_dev; a.logits = d->logits_dev; a.probs = d->probs_dev;
  cpx::launch_head(a, h->stream);
  CPX_HIP(h, hipGetLastError());
  return CPX_OK;
}

int cpx_cnn_head(cpx_handle* h, const float* in_dev, int N, int HW, int C, const float* bn_scale_dev,
                 const float* bn_shift_dev, const float* dense_w_dev, const float* dense_b_dev, int L,
                 float* logits_dev, float* probs_dev) {
  if (!h) return CPX_ERR_INVALID;
  cpx_head_desc d{};
  d.N = N; d.HW = HW; d.C = C; d.L = L;
  d.n_hidden = 0;
  d.activation = CPX_HEAD_SIGMOID;
  d.in_dev = in_dev; d.bn_scale_dev = bn_scale_dev; d.bn_shift_dev = bn_shift_dev;
  d.dense_w_dev = dense_w_dev; d.dense_b_dev = dense_b_dev; d.logits_dev = logits_dev; d.probs_dev = probs_dev;
  return cpx_cnn_head_ex(h, &d);
}

int cpx_conv_timing_enable(cpx_handle* h, int enable) {
  if (!h) return CPX_ERR_INVALID;
  for (auto& e : h->conv_events) {
    hipEventDestroy(e.e0);
    hipEventDestroy(e.e1);
  }
  h->conv_events.clear();
  h->conv_timing = enable != 0;
  return CPX_OK;
}

int cpx_conv_timing_report(cpx_handle* h, cpx_conv_timing* out, int cap, int* n_out) {
  if (!h || !out || !n_out || cap < 1) return CPX_ERR_INVALID;
  CPX_HIP(h, hipStreamSynchronize(h->stream));
  int n = 0;
  for (auto& e : h->conv_events) {
    float ms = 0.f;
    CPX_HIP(h, hipEventElapsedTime(&ms, e.e0, e.e1));
    int i = 0;
    for (; i < n; ++i)
      if (out[i].key == e.key) break;
    if (i == n) {
      if (n == cap) return fail(h, CPX_ERR_OVERFLOW, "cpx_conv_timing_report: more kernel variants than capacity");
      out[n].key = e.key;
      out[n].launches = 0;
      out[n].total_ms = 0.0;
      out[n].flops = 0.0;
      n += 1;
    }
    out[i].launches += 1;
    out[i].total_ms += ms;
    out[i].flops += e.flops;
  }
  *n_out = n;
  return CPX_OK;
}

int cpx_cnn_create(cpx_handle* h, const cpx_wrresnet_params* params, cpx_cnn** out) {
  if (!h) return CPX_ERR_INVALID;
  if (!params || !out) return fail(h, CPX_ERR_INVALID, "cpx_cnn_create: null argument");
  *out = nullptr;
  const cpx_wrresnet_params& p = *params;
  if (p.n_labels < 1 || p.blocks_per_stage < 1 || p.blocks_per_stage > CPX_WRRESNET_MAX_BLOCKS || p.groups < 1 ||
      p.in_channels < 1 || !p.conv1_w || !p.final_scale || !p.final_shift || !p.dense_w || !p.dense_b ||
      p.n_hidden < 0 || p.n_hidden > CPX_HEAD_MAX_HIDDEN ||
      (p.activation != CPX_HEAD_SIGMOID && p.activation != CPX_HEAD_SOFTMAX))
    return fail(h, CPX_ERR_INVALID, "cpx_cnn_create: bad network description");
  for (int k = 0; k < p.n_hidden; ++k)
    if (!p.hidden_w[k] || !p.hidden_b[k] || p.hidden_sizes[k] < 1 || p.hidden_sizes[k] > 2048)
      return fail(h, CPX_ERR_INVALID, "cpx_cnn_create: bad hidden dense layer");
  for (int st = 0; st < 3; ++st) {
    if (!p.shortcut_w[st]) return fail(h, CPX_ERR_INVALID, "cpx_cnn_create: missing shortcut weights");
    for (int d = 0; d < p.blocks_per_stage; ++d) {
      const cpx_wrresnet_block& b = p.block[st][d];
      if (!b.in_scale || !b.in_shift || !b.wa || !b.wb)
        return fail(h, CPX_ERR_INVALID, "cpx_cnn_create: missing block parameters");
    }
  }
  cpx_cnn* c = new (std::nothrow) cpx_cnn();
  if (!c) return fail(h, CPX_ERR_NOMEM, "cpx_cnn_create: out of memory");
  c->h = h;
  c->p = p;
  h->cnns.push_back(c);
  // the weights are constant for the life of the network: split them once (the images are used when the handle's
  // math mode is bf16x3 at forward time)
  CPX_ENTER(h);
  int c_in = p.filters[0];
  for (int st = 0; st < 3; ++st) {
    const int f = p.filters[st + 1];
    for (int d = 0; d < p.blocks_per_stage; ++d) {
      const cpx_wrresnet_block& b = p.block[st][d];
      const float* ws[2] = {b.wa, b.wb};
      for (int k = 0; k < 2; ++k) {
        // (no map yet: the image is a property of the layer alone)
        cpx::ConvArgs a = conv_shape(0, 0, 0, k == 0 ? c_in : f, f, p.groups, 3, (k == 0 && d == 0) ? st + 1 : 1, 1);
        a.weights = ws[k];
        if (a.Cin % a.groups || a.Cout % a.groups || !cpx::conv_bf3_supported(a) || c->split_of(ws[k])) continue;
        void* img = nullptr;
        if (hipMalloc(&img, cpx::conv_bf3_weight_bytes(a)) != hipSuccess) {
          (void)hipGetLastError();
          cpx_cnn_destroy(c);
          return fail(h, CPX_ERR_NOMEM, "cpx_cnn_create: weight image allocation failed");
        }
        c->split.emplace_back(ws[k], img);
        cpx::launch_split_weights(a, img, h->stream);
      }
      c_in = f;
    }
  }
  CPX_HIP(h, hipGetLastError());
  *out = c;
  return CPX_OK;
}

void cpx_cnn_destroy(cpx_cnn* cnn) {
  if (!cnn) return;
  cpx_handle* h = cnn->h;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  h->cnns.erase(std::remove(h->cnns.begin(), h->cnns.end(), cnn), h->cnns.end());
  cnn_free(cnn);
}

int cpx_cnn_set_activation_bounds(cpx_cnn* cnn, const float* bounds, int n) {
  if (!cnn) return CPX_ERR_INVALID;
  cpx_handle* h = cnn->h;
  const cpx_wrresnet_params& p = cnn->p;
  if (!bounds || n != 3 * p.blocks_per_stage * 2)
    return fail(h, CPX_ERR_INVALID, "cpx_cnn_set_activation_bounds: expected 3 * blocks_per_stage * 2 bounds");
  for (int st = 0; st < 3; ++st)
    for (int d = 0; d < p.blocks_per_stage; ++d)
      for (int k = 0; k < 2; ++k) {
        const float b = bounds[(st * p.blocks_per_stage + d) * 2 + k];
        // the largest power of two that keeps bound * scale at or below 2^12, between 1 and 2^14; no usable bound: 1.
        // (2^12, not 2^15: sixteen times the bound still fits fp16 -- a bound from BatchNorm statistics is a guess, and
        // headroom is cheap: the low plane of every activation above 2^-3 / scale keeps all its bits either way)
        int e = 0;
        if (b > 0.0f && std::isfinite(b)) {
          int eb = 0;
          (void)std::frexp(b, &eb);  // b = f 2^eb, f in [0.5, 1): b <= 2^eb
          e = std::min(std::max(12 - eb, 0), 14);
        }
        cnn->act_scale[st][d][k] = std::ldexp(1.0f, e);
      }
  return update_shortcut_images(cnn);  // (the shortcut images carry act_scale: nothing to do while no residual bound is set)
}

int cpx_cnn_shortcut_scale(float bound, float wmax, float* sx) {
  if (!sx) return 0;
  *sx = 0.0f;
  if (!(bound > 0.0f) || !(wmax > 0.0f) || !std::isfinite(bound) || !std::isfinite(wmax)) return 0;
  int eb = 0, ew = 0;
  (void)std::frexp(bound, &eb);  // bound <= 2^eb
  (void)std::frexp(wmax, &ew);   // 2^(ew - 1) <= wmax < 2^ew
  // sx = 2^e.  Inside fp16: bound sx <= 2^15 and wmax / sx < 2^15.  Low planes (they resolve 2^-24 absolute): bound sx > 2^3 --
  // a bound of 64 standard deviations then has its typical operand above 2^-3 --, and wmax / sx >= 2^-1: weights down to a
  // quarter of the largest stay above 2^-3
  const int e_lo = std::max(4 - eb, ew - 15), e_hi = std::min(15 - eb, ew);
  if (e_lo > e_hi) return 0;
  // the bound at 2^12 where the window allows: sixteen-fold headroom, as for the activations
  const int e = std::min(std::max(12 - eb, e_lo), e_hi);
  if (e < -60 || e > 60) return 0;
  *sx = std::ldexp(1.0f, e);
  return 1;
}

int cpx_cnn_set_residual_bounds(cpx_cnn* cnn, const float* bounds, int n) {
  if (!cnn) return CPX_ERR_INVALID;
  cpx_handle* h = cnn->h;
  if (!bounds || n != 3) return fail(h, CPX_ERR_INVALID, "cpx_cnn_set_residual_bounds: expected 3 bounds, one per stage");
  for (int st = 0; st < 3; ++st)
    if (!(bounds[st] >= 0.0f) || !std::isfinite(bounds[st]))
      return fail(h, CPX_ERR_INVALID, "cpx_cnn_set_residual_bounds: a bound is negative or not finite");
  for (int st = 0; st < 3; ++st) cnn->res_bound[st] = bounds[st];
  return update_shortcut_images(cnn);
}

int cpx_cnn_forward(cpx_cnn* cnn, const float* in_dev, int N, int H, int W, float* logits_dev, float* probs_dev) {
  if (!cnn) return CPX_ERR_INVALID;
  if (!in_dev || !logits_dev || N < 1 || H < 1 || W < 1)
    return fail(cnn->h, CPX_ERR_INVALID, "cpx_cnn_forward: bad argument");
  return cnn_forward(cnn, in_dev, N, H, W, logits_dev, probs_dev, nullptr, nullptr);
}

int cpx_cnn_forward_taps(cpx_cnn* cnn, const float* in_dev, int N, int H, int W, float* logits_dev, float* probs_dev,
                         float* const* block_out_dev, int n_blocks, int* block_overflow_dev) {
  if (!cnn) return CPX_ERR_INVALID;
  cpx_handle* h = cnn->h;
  if (!in_dev || !logits_dev || N < 1 || H < 1 || W < 1 || !block_out_dev)
    return fail(h, CPX_ERR_INVALID, "cpx_cnn_forward_taps: bad argument");
  if (n_blocks != 3 * cnn->p.blocks_per_stage)
    return fail(h, CPX_ERR_INVALID, "cpx_cnn_forward_taps: expected n_blocks = 3 * blocks_per_stage");
  for (int k = 0; k < n_blocks; ++k)
    if (!block_out_dev[k]) return fail(h, CPX_ERR_INVALID, "cpx_cnn_forward_taps: null block output");
  return cnn_forward(cnn, in_dev, N, H, W, logits_dev, probs_dev, block_out_dev, block_overflow_dev);
}

}  // extern "C"
