// The parts a decode can be enqueued in (Batch::RunPart, JxlHipBatchDecodePart), the stages a part consists of and the timing marks the stages record.
// Host only, no HIP: this table is the one place that says what a part does (tests/decode_parts_table.cc compares it with the table written out).
#pragma once

namespace jxlhip {

// the stages of a decode, in the order they run; a part is a set of them
enum Stage : unsigned {
  kStageLf = 1,        // Modular global streams, LF decode, varblock placement
  kStageLfPost = 2,    // LF frames, dequantised LF, LLF, EPF sigma
  kStageHf = 4,        // coefficient clear, HF decode (with VarDCT frames in the batch: the Modular sub-streams and tail too)
  kStageIdct = 8,      // the last stage that touches the coefficient planes
  kStagePixels = 16,   // filters, colour, write, frame tail, resizes
};
// the timing marks of a timed decode (StageTimes, Batch::DebugTimeline): indices into one row of events.  The HF stage and the IDCT of a split decode may sit on other
// streams than the stage before them: they record a start of their own
enum Mark : int { kMarkLfStart, kMarkLfEnd, kMarkLfPostEnd, kMarkHfEnd, kMarkIdctEnd, kMarkFiltersEnd, kMarkOutputEnd, kMarkHfStart, kMarkIdctStart, kNumMarks };
// The integer codes are public for 0 .. 8 (include/jxl_hip.h); the libjpeg-exact flavours (after PlanJpegPixels / EnqueueJpegPixelTable) are internal.
enum DecodePart : int {
  kPartWhole = 0,          // every stage, timed as one decode
  kPartFront = 1,          // LF decode + LF post-processing
  kPartRest = 2,           // HF decode, IDCT, pixels
  kPartHf = 3,
  kPartAfterHf = 4,        // IDCT, pixels
  kPartLf = 5,             // what the HF stage waits for
  kPartLfPost = 6,         // what the IDCT and the filters wait for
  kPartIdct = 7,
  kPartPixels = 8,
  kPartJpegIdct = 9,       // libjpeg-exact: the integer IDCT over the HF planes (EnqueueJpegIdct)
  kPartJpegPixels = 10,    // libjpeg-exact: chroma upsampling, colour, write (EnqueueJpegColorOut), resizes
  kPartJpegLfPost = 11,    // libjpeg-exact: the tail reads nothing LF post-processing writes — records the mark, launches nothing
  kPartJpegHf = 12,        // libjpeg-exact: frames decoded by region (jpeg_region) decode the groups of their lists only
  kNumParts = 13,
  kNumPublicParts = 9,
};

struct PartPlan {
  unsigned stages;        // Stage bits
  bool jpeg;              // the libjpeg-exact flavour of those stages
  bool split;             // one piece of a decode that a caller enqueues in pieces: records its own start marks, reads the placement flags back behind the LF stage
  bool lf_head_start;     // the LF stage on its own: a pipelined caller, the HF stage of another batch is about to start
  constexpr bool has(Stage s) const { return (stages & s) != 0; }
};
constexpr PartPlan PlanOf(int part) {
  constexpr unsigned kStages[kNumParts] = {
      kStageLf | kStageLfPost | kStageHf | kStageIdct | kStagePixels, kStageLf | kStageLfPost, kStageHf | kStageIdct | kStagePixels, kStageHf, kStageIdct | kStagePixels,
      kStageLf, kStageLfPost, kStageIdct, kStagePixels, kStageIdct, kStagePixels, kStageLfPost, kStageHf};
  const unsigned stages = part >= 0 && part < kNumParts ? kStages[part] : 0;
  const bool split = part != kPartWhole;
  return PartPlan{stages, part >= kPartJpegIdct && part < kNumParts, split, split && (stages & kStageLf) != 0};
}
// the part that is one stage in one flavour: callers that decide by the kind of a job pick a flavour (there is one LF stage for both)
constexpr DecodePart PartOf(Stage stage, bool jpeg) {
  for (int part = 1; part < kNumParts; part++)
    if (PlanOf(part).stages == stage && PlanOf(part).jpeg == (jpeg && stage != kStageLf)) return (DecodePart)part;
  return kNumParts;
}

}  // namespace jxlhip
