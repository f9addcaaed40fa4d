// Which ready jobs of a pipeline share one SIMT LF launch (kernels.h LaunchLfSimtGroup), and how many LF streams a process with Q hardware queues uses.
// Host only, no HIP: tests/lf_group_plan.cc checks both functions against the rules written here.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace jxlhip {

constexpr int kLfGroupMax = 8;      // parts of one launch (the table travels as kernel arguments)

// What two jobs must agree in to share a launch.  eligible: a plain VarDCT batch with a SIMT plan that does not take the wide one-wavefront-per-stream launch and has
// no LF groups with trees of their own; kernel: the LfDecodeSimtKernel instantiation (weighted predictor / general / lean, and the candidate lanes per stream).
struct LfGroupKey {
  int eligible = 0;
  int kernel = 0;
  uint32_t lanes_per_wave = 0;
  int lf_flags = 0;
  bool operator==(const LfGroupKey& o) const { return eligible == o.eligible && kernel == o.kernel && lanes_per_wave == o.lanes_per_wave && lf_flags == o.lf_flags; }
};

// The ready jobs in ticket order -> the sizes of the groups, in that order (their sum is n).  A group is a run of adjacent eligible jobs with equal keys, of at most
// min(cap, kLfGroupMax) jobs (cap < 1 counts as 1); an ineligible job is a group of one.  Order is kept inside a group and between groups: job i never overtakes job i - 1.
inline std::vector<int> PlanLfGroups(const LfGroupKey* keys, int n, int cap) {
  std::vector<int> groups;
  cap = cap < 1 ? 1 : cap > kLfGroupMax ? kLfGroupMax : cap;
  for (int i = 0; i < n;) {
    int m = 1;
    if (keys[i].eligible) while (i + m < n && m < cap && keys[i + m] == keys[i]) m++;
    groups.push_back(m);
    i += m;
  }
  return groups;
}

// LF streams a pipeline uses: min(lf_streams, kLfStreamsCap, max(3, Q - 2 - hf_streams)).  Streams that share a hardware queue serialise, so beside the main stream,
// the copy stream and the HF streams only Q - 2 - hf_streams queues are left for LF launches.  Never fewer than three streams (measured at 4 queues: three are 1-3 % ahead
// of two — a launch runs on two of them while the next group collects), never more than kLfStreamsCap (measured at 16 queues: with grouped launches 6 streams give
// 29.6 Gpixel/s, 10 give 27.8, 11 give 25.8-26.8: more launches side by side only crowd the pixel kernels), never more than asked for.  hw_queues: the text of
// GPU_MAX_HW_QUEUES as the process has it; nullptr, empty, not a positive number: 4, the runtime's default.
constexpr int kLfStreamsCap = 6;
inline int LfStreamsForQueues(int lf_streams, int hf_streams, const char* hw_queues) {
  long q = 4;
  if (hw_queues && *hw_queues) {
    char* end = nullptr;
    const long v = strtol(hw_queues, &end, 10);
    if (end && *end == 0 && v > 0 && v <= 1024) q = v;
  }
  const long room = q - 2 - hf_streams;
  const long want = room > kLfStreamsCap ? kLfStreamsCap : room > 3 ? room : 3;
  return (int)(lf_streams < want ? (lf_streams < 1 ? 1 : lf_streams) : want);
}

}  // namespace jxlhip
