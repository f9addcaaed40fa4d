// PlanLfGroups and LfStreamsForQueues (jpegxl-rs_amd/csrc/lf_group_plan.h) against their rules, on hand-made key sequences.  Stand-alone, host only;
// tests/test_lf_group_plan.py builds it with -fsanitize=address,undefined and runs it.
#include "lf_group_plan.h"
#include <cstdio>
#include <string>

using namespace jxlhip;

static int mismatches = 0;

static LfGroupKey Key(int eligible, int kernel = 16, uint32_t lanes_per_wave = 8, int lf_flags = 0) {
  LfGroupKey k;
  k.eligible = eligible; k.kernel = kernel; k.lanes_per_wave = lanes_per_wave; k.lf_flags = lf_flags;
  return k;
}
static std::string Show(const std::vector<int>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); i++) s += (i ? " " : "") + std::to_string(v[i]);
  return s + "]";
}
static void Expect(const char* what, const std::vector<LfGroupKey>& keys, int cap, const std::vector<int>& want) {
  const std::vector<int> got = PlanLfGroups(keys.data(), (int)keys.size(), cap);
  // the rules, whatever the expected sizes say: the sizes cover the list in order, no group exceeds the cap or kLfGroupMax, groups larger than one are uniform and eligible
  size_t at = 0;
  bool ok = got == want;
  const int limit = cap < 1 ? 1 : cap > kLfGroupMax ? kLfGroupMax : cap;
  for (int m : got) {
    if (m < 1 || m > limit || at + (size_t)m > keys.size()) { ok = false; break; }
    for (int i = 0; i < m && m > 1; i++) if (!keys[at + (size_t)i].eligible || !(keys[at + (size_t)i] == keys[at])) ok = false;
    at += (size_t)m;
  }
  if (at != keys.size()) ok = false;
  if (!ok) { mismatches++; printf("MISMATCH %s: cap %d -> %s, expected %s\n", what, cap, Show(got).c_str(), Show(want).c_str()); }
}
static void ExpectStreams(const char* q, int lf_streams, int hf_streams, int want) {
  const int got = LfStreamsForQueues(lf_streams, hf_streams, q);
  if (got != want) { mismatches++; printf("MISMATCH streams: Q \"%s\", lf_streams %d, hf_streams %d -> %d, expected %d\n", q ? q : "(unset)", lf_streams, hf_streams, got, want); }
}

int main() {
  const LfGroupKey lean = Key(1), wp = Key(1, 4), other_lanes = Key(1, 16, 16), other_flags = Key(1, 16, 8, 1), no = Key(0), no2 = Key(0, 4);
  Expect("empty", {}, 4, {});
  Expect("one", {lean}, 4, {1});
  Expect("cap respected", {lean, lean, lean, lean, lean, lean}, 4, {4, 2});
  Expect("cap 2", {lean, lean, lean, lean, lean}, 2, {2, 2, 1});
  Expect("cap 1: off", {lean, lean, lean}, 1, {1, 1, 1});
  Expect("cap 0 counts as 1", {lean, lean}, 0, {1, 1});
  Expect("cap -3 counts as 1", {lean, lean}, -3, {1, 1});
  Expect("full table", std::vector<LfGroupKey>(8, lean), 8, {8});
  Expect("nine", std::vector<LfGroupKey>(9, lean), 8, {8, 1});
  Expect("cap clamped to kLfGroupMax", std::vector<LfGroupKey>(20, lean), 100, {8, 8, 4});
  Expect("mixed kernels split", {lean, wp, lean}, 4, {1, 1, 1});
  Expect("mixed kernels, runs", {lean, lean, wp, wp, wp, lean}, 4, {2, 3, 1});
  Expect("lanes per wavefront split", {lean, other_lanes, other_lanes}, 4, {1, 2});
  Expect("flags split", {lean, other_flags, lean, lean}, 4, {1, 1, 2});
  Expect("ineligible alone", {no, no, no}, 4, {1, 1, 1});
  Expect("ineligible between", {lean, lean, no, lean, lean, lean}, 4, {2, 1, 3});
  Expect("ineligible with equal fields stays alone", {no2, no2, wp, wp}, 4, {1, 1, 2});
  Expect("ineligible first and last", {no, lean, lean, no}, 8, {1, 2, 1});
  // order: group k covers the keys right behind group k - 1 (checked by Expect for every case above); a key that matches a job two places back does not jump the queue
  Expect("no reordering", {lean, wp, lean, wp}, 8, {1, 1, 1, 1});

  // streams: min(lf_streams, kLfStreamsCap, max(3, Q - 2 - hf_streams)), Q = 4 when GPU_MAX_HW_QUEUES is unset or no positive number
  static_assert(kLfStreamsCap == 6, "the expectations below are written for a cap of six");
  ExpectStreams(nullptr, 11, 2, 3);
  ExpectStreams("", 11, 2, 3);
  ExpectStreams("0", 11, 2, 3);
  ExpectStreams("1", 11, 2, 3);
  ExpectStreams("4", 11, 2, 3);
  ExpectStreams("8", 11, 2, 4);
  ExpectStreams("9", 11, 2, 5);
  ExpectStreams("10", 11, 2, 6);
  ExpectStreams("16", 11, 2, 6);     // the cap
  ExpectStreams("16", 32, 2, 6);
  ExpectStreams("32", 11, 2, 6);
  ExpectStreams("32", 32, 2, 6);
  ExpectStreams("garbage", 11, 2, 3);
  ExpectStreams("16x", 11, 2, 3);
  ExpectStreams("-8", 11, 2, 3);
  ExpectStreams("16", 1, 2, 1);      // never more than asked for
  ExpectStreams("4", 1, 2, 1);
  ExpectStreams("4", 2, 2, 2);
  ExpectStreams("16", 4, 2, 4);
  ExpectStreams("16", 11, 12, 3);    // never fewer than three when three were asked for
  ExpectStreams("8", 3, 1, 3);
  ExpectStreams("8", 11, 1, 5);
  printf("%d mismatches\n", mismatches);
  return mismatches ? 1 : 0;
}
