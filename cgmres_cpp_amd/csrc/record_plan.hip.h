// The launch cut of a recorded closed loop (cgmres_hip_closed_loop_device_rec): one decision, one place, no kernel code.
//
// Tick k of a call is recorded iff (k + 1) % stride == 0, and a record is taken BETWEEN launches, so every recorded tick
// has to be the last tick of a launch.  The rule: each stride window is cut exactly as a fresh call of `stride` ticks is
// cut (fuse, ..., fuse, remainder), and the tail behind the last record as a fresh call of the remaining ticks.  A
// recorded loop is then, launch for launch, the loop of a caller who calls cgmres_hip_closed_loop_device_ex once per
// window, and a stride that is a multiple of `fuse` adds no launch.  stride 0: nothing is recorded, one window.
// `fuse` is the mapping's ticks per launch: CGMRES_HIP_TICKS_PER_LAUNCH for the wg contexts, 1 for the lane context.
#pragma once
#include <cstdint>

namespace cgm {

struct RecordCut {
  int n_ticks, stride, fuse;
  int i = 0;  // first tick of the next launch
  constexpr RecordCut(int n_ticks_, int stride_, int fuse_) : n_ticks(n_ticks_), stride(stride_), fuse(fuse_) {}
  constexpr int n_rec() const { return stride > 0 ? n_ticks / stride : 0; }
  constexpr bool done() const { return i >= n_ticks; }
  // Ticks of the next launch; *rec: it ends a stride window, whose record (number i / stride - 1 afterwards) is due.
  constexpr int next(bool* rec) {
    const bool in_window = stride > 0 && i / stride < n_ticks / stride;
    const int end = in_window ? (i / stride + 1) * stride : n_ticks;
    const int n = end - i < fuse ? end - i : fuse;
    i += n;
    *rec = in_window && i == end;
    return n;
  }
};

// cgmres_hip_record_plan: *n_rec records, *n_launches launches, their sizes in launch_ticks[0 .. cap) (null: not wanted).
// false for n_ticks < 0, stride < 1 or a cap smaller than the number of launches.
inline bool record_plan(int n_ticks, int stride, int fuse, int32_t* n_rec, int32_t* launch_ticks, int cap, int32_t* n_launches) {
  if (n_ticks < 0 || stride < 1 || fuse < 1) return false;
  RecordCut cut(n_ticks, stride, fuse);
  int n = 0;
  while (!cut.done()) {
    bool rec = false;
    const int ticks = cut.next(&rec);
    if (launch_ticks) {
      if (n >= cap) return false;
      launch_ticks[n] = ticks;
    }
    ++n;
  }
  if (n_rec) *n_rec = cut.n_rec();
  if (n_launches) *n_launches = n;
  return true;
}

}  // namespace cgm
