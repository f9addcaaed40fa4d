// The part table of jpegxl-rs_amd/csrc/decode_parts.h against the table written out: which stages part 0 .. 12 runs, in which flavour, and the two derived bits;
// and the nine timing marks against their indices.  Host only.
#include <cstdio>

#include "decode_parts.h"

using namespace jxlhip;

int main() {
  // part: LF, LF post, HF, IDCT, pixels, libjpeg-exact flavour, split, LF head start
  static const int kExpected[13][8] = {
      {1, 1, 1, 1, 1, 0, 0, 0},   // 0  whole decode
      {1, 1, 0, 0, 0, 0, 1, 1},   // 1
      {0, 0, 1, 1, 1, 0, 1, 0},   // 2
      {0, 0, 1, 0, 0, 0, 1, 0},   // 3
      {0, 0, 0, 1, 1, 0, 1, 0},   // 4
      {1, 0, 0, 0, 0, 0, 1, 1},   // 5
      {0, 1, 0, 0, 0, 0, 1, 0},   // 6
      {0, 0, 0, 1, 0, 0, 1, 0},   // 7
      {0, 0, 0, 0, 1, 0, 1, 0},   // 8
      {0, 0, 0, 1, 0, 1, 1, 0},   // 9  libjpeg-exact IDCT
      {0, 0, 0, 0, 1, 1, 1, 0},   // 10 libjpeg-exact pixels
      {0, 1, 0, 0, 0, 1, 1, 0},   // 11 libjpeg-exact LF post: the mark only
      {0, 0, 1, 0, 0, 1, 1, 0},   // 12 libjpeg-exact HF: by group list
  };
  int bad = 0;
  static_assert(kNumParts == 13 && kNumPublicParts == 9, "part codes");
  for (int part = 0; part < 13; part++) {
    const PartPlan p = PlanOf(part);
    const int got[8] = {p.has(kStageLf), p.has(kStageLfPost), p.has(kStageHf), p.has(kStageIdct), p.has(kStagePixels), p.jpeg, p.split, p.lf_head_start};
    for (int k = 0; k < 8; k++)
      if (got[k] != kExpected[part][k]) { printf("part %d column %d: %d, expected %d\n", part, k, got[k], kExpected[part][k]); bad++; }
    if (p.stages & ~31u) { printf("part %d: unknown stage bits %u\n", part, p.stages); bad++; }
  }
  if (PlanOf(-1).stages || PlanOf(13).stages) { printf("a code outside 0 .. 12 runs stages\n"); bad++; }
  // the names keep the public codes
  const int names[13] = {kPartWhole, kPartFront, kPartRest, kPartHf, kPartAfterHf, kPartLf, kPartLfPost, kPartIdct, kPartPixels, kPartJpegIdct, kPartJpegPixels, kPartJpegLfPost, kPartJpegHf};
  for (int part = 0; part < 13; part++) if (names[part] != part) { printf("name of part %d has the value %d\n", part, names[part]); bad++; }
  // a stage in a flavour -> its part
  const struct { Stage s; bool jpeg; int part; } picks[] = {{kStageLf, false, 5}, {kStageLf, true, 5}, {kStageLfPost, false, 6}, {kStageLfPost, true, 11}, {kStageHf, false, 3}, {kStageHf, true, 12},
                                                           {kStageIdct, false, 7}, {kStageIdct, true, 9}, {kStagePixels, false, 8}, {kStagePixels, true, 10}};
  for (auto& k : picks) if (PartOf(k.s, k.jpeg) != k.part) { printf("PartOf(%u, %d) = %d, expected %d\n", (unsigned)k.s, (int)k.jpeg, (int)PartOf(k.s, k.jpeg), k.part); bad++; }
  const int marks[9] = {kMarkLfStart, kMarkLfEnd, kMarkLfPostEnd, kMarkHfEnd, kMarkIdctEnd, kMarkFiltersEnd, kMarkOutputEnd, kMarkHfStart, kMarkIdctStart};
  for (int m = 0; m < 9; m++) if (marks[m] != m) { printf("mark %d has the value %d\n", m, marks[m]); bad++; }
  if (kNumMarks != 9) { printf("kNumMarks = %d\n", (int)kNumMarks); bad++; }
  printf("%d mismatches\n", bad);
  return bad ? 1 : 0;
}
