// TEST INFRASTRUCTURE ONLY: host build of classifier-pipeline_amd/csrc/cpx_schedule_core.h (tests/test_schedule_host.py).
// As a shared object it hands the flat schedule and its layout to NumPy; with -DSCHEDULE_HOST_MAIN it is a program
// of its own that walks the same cases, for a sanitizer build.  The product never loads either.
#include <stdio.h>

#include <vector>

#include "cpx_schedule_core.h"

// Builds and flattens.  Returns the SchedError (0 ok, 1 empty clip, 2 too long), or -1 when `flat` is too small.
// layout: clip_first, proc_off, proc_idx, proc_ffc, order, ints.  total_max: Schedule::total, Schedule::max_proc.
extern "C" int schedule_host(const int32_t* clip_offsets, const cpx_frame_meta* meta, int B, int max_frames, int* flat,
                             int flat_cap, int64_t* layout, int* total_max) {
  cpx::Schedule sc;
  const cpx::SchedError e = cpx::schedule_build(clip_offsets, meta, B, max_frames, &sc);
  if (e != cpx::SchedError::Ok) return (int)e;
  const std::vector<int> f = cpx::schedule_flatten(sc, B);
  const cpx::SchedLayout l = cpx::SchedLayout::of(B, (int)sc.proc_idx.size());
  if (f.size() != l.ints || (size_t)flat_cap < l.ints) return -1;
  for (size_t i = 0; i < f.size(); ++i) flat[i] = f[i];
  const size_t offs[6] = {l.clip_first, l.proc_off, l.proc_idx, l.proc_ffc, l.order, l.ints};
  for (int i = 0; i < 6; ++i) layout[i] = (int64_t)offs[i];
  total_max[0] = sc.total;
  total_max[1] = sc.max_proc;
  return 0;
}

extern "C" int processed_before_host(const cpx_frame_meta* meta, int n_prev) { return cpx::processed_before(meta, n_prev); }

#ifdef SCHEDULE_HOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                 \
    }                                                             \
  } while (0)

cpx_frame_meta frame(int background, int has_times = 0, int64_t on = 0, int64_t ffc = 0) {
  cpx_frame_meta m{};
  m.time_on_ms = on;
  m.last_ffc_ms = ffc;
  m.background_frame = background;
  m.has_times = has_times;
  return m;
}

struct Built {
  int rc;
  std::vector<int> flat;
  int64_t lay[6];
  int tm[2];
};

Built run(const std::vector<int32_t>& offs, const std::vector<cpx_frame_meta>& meta, int max_frames) {
  Built b{};
  const int B = (int)offs.size() - 1;
  b.flat.assign(3 * (size_t)B + 3 + 2 * meta.size(), -7);
  b.rc = schedule_host(offs.data(), meta.data(), B, max_frames, b.flat.data(), (int)b.flat.size(), b.lay, b.tm);
  return b;
}

}  // namespace

int main() {
  {  // no processed frames: the two padding ints
    const Built b = run({0, 3}, {frame(1), frame(1), frame(1)}, 10);
    EXPECT(b.rc == 0 && b.lay[5] == 1 + 2 + 2 + 1 && b.tm[0] == 3 && b.tm[1] == 0);
    EXPECT(b.flat[b.lay[2]] == 0 && b.flat[b.lay[3]] == 0 && b.flat[b.lay[4]] == 0);
  }
  {  // FFC boundary
    const Built b = run({0, 4}, {frame(0, 1, 1008, 1000), frame(0, 1, 1009, 1000), frame(0, 0, 1001, 1000), frame(0, 1, 5, 1000)}, 10);
    EXPECT(b.rc == 0);
    const int* ffc = b.flat.data() + b.lay[3];
    EXPECT(ffc[0] == 1 && ffc[1] == 0 && ffc[2] == 0 && ffc[3] == 1);
  }
  {  // order: longest first, ties by index
    const int len[5] = {3, 7, 3, 7, 1};
    std::vector<int32_t> offs{0};
    std::vector<cpx_frame_meta> meta;
    for (int n : len) {
      meta.push_back(frame(1));
      for (int i = 0; i < n; ++i) meta.push_back(frame(0));
      offs.push_back((int32_t)meta.size());
    }
    const Built b = run(offs, meta, 7);
    const int want[5] = {1, 3, 0, 2, 4};
    EXPECT(b.rc == 0 && b.tm[1] == 7);
    for (int i = 0; i < 5; ++i) EXPECT(b.flat[b.lay[4] + i] == want[i]);
    EXPECT(b.flat[b.lay[0] + 1] == 4 && b.flat[b.lay[1] + 5] == 21 && b.flat[b.lay[2]] == 1);
  }
  {  // max_frames counts processed frames only
    std::vector<cpx_frame_meta> meta{frame(1), frame(1)};
    for (int i = 0; i < 6; ++i) meta.push_back(frame(0));
    EXPECT(run({0, 8}, meta, 6).rc == 0);
    meta.push_back(frame(0));
    EXPECT(run({0, 9}, meta, 6).rc == (int)cpx::SchedError::TooLong);
  }
  {  // an empty clip in the middle
    const std::vector<cpx_frame_meta> meta(4, frame(0));
    EXPECT(run({0, 2, 2, 4}, meta, 10).rc == (int)cpx::SchedError::EmptyClip);
  }
  {  // processed_before
    const std::vector<cpx_frame_meta> meta{frame(1), frame(1), frame(0), frame(0), frame(1), frame(0)};
    const int want[7] = {0, 0, 0, 1, 2, 2, 3};
    for (int n = 0; n <= 6; ++n) EXPECT(processed_before_host(meta.data(), n) == want[n]);
    EXPECT(processed_before_host(meta.data(), -1) == 0);
  }
  return failures ? 1 : 0;
}
#endif
