// cpx_schedule_core.h -- the host-side schedule of the per-frame launches: which frames of a batch are processed,
// their FFC flags, the order the clips are handed out in, and the ONE flat layout the device reads them in.  Plain
// host C++ without HIP, so that tests compile it on its own (tests/native/schedule_host.cpp); cpx_api.cpp is its
// only user in the product.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "cpx.h"

namespace cpx {

struct Schedule {
  std::vector<int> clip_first, proc_off, proc_idx, proc_ffc, order;
  int total = 0, max_proc = 0;
};

enum class SchedError { Ok, EmptyClip, TooLong };

// which frames are processed (background frames only initialise, cliptrackextractor.py:167-168)
// and their FFC flags (cptvmotiondetector.py:211-223 with int milliseconds)
inline SchedError schedule_build(const int32_t* clip_offsets, const cpx_frame_meta* meta, int B, int max_frames,
                                 Schedule* sc) {
  sc->total = clip_offsets[B];
  sc->clip_first.resize(B);
  sc->proc_off.assign(B + 1, 0);
  sc->proc_idx.reserve(sc->total);
  sc->proc_ffc.reserve(sc->total);
  for (int b = 0; b < B; ++b) {
    const int f0 = clip_offsets[b], f1 = clip_offsets[b + 1];
    if (f1 <= f0) return SchedError::EmptyClip;
    sc->clip_first[b] = f0;
    for (int f = f0; f < f1; ++f) {
      if (meta[f].background_frame) continue;
      sc->proc_idx.push_back(f);
      int ffc = 0;
      if (meta[f].has_times) ffc = (meta[f].time_on_ms - meta[f].last_ffc_ms) < 9 ? 1 : 0;
      sc->proc_ffc.push_back(ffc);
    }
    sc->proc_off[b + 1] = (int)sc->proc_idx.size();
    const int np = sc->proc_off[b + 1] - sc->proc_off[b];
    if (np > max_frames) return SchedError::TooLong;
    sc->max_proc = std::max(sc->max_proc, np);
  }
  // longest clips first: one workgroup walks a whole clip, and the dispatcher hands out workgroups in index order
  sc->order.resize(B);
  for (int b = 0; b < B; ++b) sc->order[b] = b;
  std::stable_sort(sc->order.begin(), sc->order.end(), [&](int x, int y) {
    return sc->proc_off[x + 1] - sc->proc_off[x] > sc->proc_off[y + 1] - sc->proc_off[y];
  });
  return SchedError::Ok;
}

// the schedule as one int array: clip_first[B] | proc_off[B+1] | proc_idx[n] | proc_ffc[n] | order[B], n = max(nproc, 1)
// (a batch of background frames only still gives every array an address of its own).  Offsets in ints.
struct SchedLayout {
  size_t clip_first, proc_off, proc_idx, proc_ffc, order, ints;
  static SchedLayout of(int B, int nproc) {
    const size_t n = (size_t)std::max(nproc, 1);
    SchedLayout l{};
    l.clip_first = 0;
    l.proc_off = l.clip_first + (size_t)B;
    l.proc_idx = l.proc_off + (size_t)B + 1;
    l.proc_ffc = l.proc_idx + n;
    l.order = l.proc_ffc + n;
    l.ints = l.order + (size_t)B;
    return l;
  }
};

inline std::vector<int> schedule_flatten(const Schedule& sc, int B) {
  const SchedLayout l = SchedLayout::of(B, (int)sc.proc_idx.size());
  std::vector<int> flat(l.ints, 0);
  std::copy(sc.clip_first.begin(), sc.clip_first.end(), flat.begin() + l.clip_first);
  std::copy(sc.proc_off.begin(), sc.proc_off.end(), flat.begin() + l.proc_off);
  std::copy(sc.proc_idx.begin(), sc.proc_idx.end(), flat.begin() + l.proc_idx);
  std::copy(sc.proc_ffc.begin(), sc.proc_ffc.end(), flat.begin() + l.proc_ffc);
  std::copy(sc.order.begin(), sc.order.end(), flat.begin() + l.order);
  return flat;
}

// points a kernel argument struct at the flat array at `base` (TrackArgs also has `order`: its caller sets that)
template <class Args>
void schedule_point(Args& a, const int* base, const SchedLayout& l) {
  a.clip_first = base + l.clip_first;
  a.proc_off = base + l.proc_off;
  a.proc_idx = base + l.proc_idx;
  a.proc_ffc = base + l.proc_ffc;
}

// processed frames among a clip's first n_prev: the step a resumed stream continues at
inline int processed_before(const cpx_frame_meta* meta, int n_prev) {
  int t = 0;
  for (int f = 0; f < n_prev; ++f) t += meta[f].background_frame ? 0 : 1;
  return t;
}

}  // namespace cpx
