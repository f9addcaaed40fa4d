// jxl-hip: lossless batch encoder (prefix-coded Modular codestreams) — what the device kernels (encode_lossless.hip) and the host half (encode_lossless.cc) share:
// the fixed MA tree's constants, the token alphabet and the device tables.  The host file compiles with a plain C++ compiler too (sanitizer build), so streams are void*.
#pragma once
#include <cstddef>
#include <cstdint>

namespace jxlhip {

constexpr uint32_t kEncGroupDim = 256;              // group_size_shift = 1
constexpr uint32_t kEncMaxChannels = 4;
// The fixed tree: a split on the channel, then a balanced tree over these cut-offs of property 9 (W + N - NW); every leaf predicts with the clamped gradient (5).
constexpr int kEncNumCuts = 11;
#define JXL_ENC_CUTS {-1023, -255, -63, -15, -3, 0, 3, 15, 63, 255, 1023}   /* (a macro: device code cannot read a host array) */
constexpr uint32_t kEncLeaves = kEncNumCuts + 1;    // per channel
constexpr uint32_t kEncNumCtx = kEncMaxChannels * kEncLeaves;
// Hybrid-uint configuration (split_exponent 4, msb 2, lsb 0).  The largest residual is that of a 16-bit chroma channel after the RCT: |v - guess| <= 2 * 65535, packed
// 262140 < 2^18, whose token is 16 + (17 - 4) * 4 + 3 = 71.
constexpr uint32_t kEncAlphabet = 72;
constexpr uint32_t kEncHistSize = kEncNumCtx * kEncAlphabet;
constexpr uint32_t kEncMaxCodeBits = 15;            // prefix code length limit of the format

constexpr uint32_t kEncFlagRange = 1;               // a sample above 2^bits - 1
constexpr uint32_t kEncFlagPack = 2;                // the pack pass met a store outside its section (the two passes disagree: cannot happen)

struct EncImageDev {
  const uint8_t* src;                // interleaved samples, u8 or little-endian u16
  uint64_t pitch;                    // bytes per row
  uint32_t xsize, ysize, nch, bytes_per_sample, max_value, rct;
};
// One section that carries samples: the whole image (GlobalModular of a single-group frame) or one group (PassGroup).  lead_bits bits come before its tokens: the
// group header of a PassGroup (lead_value), or the last bits of the host-written LfGlobal prefix, which the host ORs in (value 0).
struct EncSectionDev { uint32_t image, x0, y0, w, h, lead_bits, lead_value, row_base; };

struct EncPlan {
  const EncImageDev* images;
  const EncSectionDev* sections;
  uint32_t num_images, num_sections;
  const uint8_t* leaf_ctx;           // [4 channel counts][4 channels][kEncLeaves]: bucket of property 9 -> context (the leaf's number in the tree's BFS order)
  uint32_t* hist;                    // [num_images][kEncNumCtx][kEncAlphabet]
  uint32_t* flags;                   // [num_images]
  const uint32_t* codes;             // [num_images][kEncNumCtx][kEncAlphabet]: bit-reversed code | length << 16
  uint32_t* row_off;                 // per (section, channel, row): bits of the section's tokens before that row
  uint32_t* sec_bytes;               // [num_sections]
  uint64_t* sec_off;                 // [num_sections + 1]: byte offset of every section in the compact buffer; the last entry is the total
  uint32_t* out;                     // the compact buffer (zeroed), out_words 32-bit words
  uint64_t out_words;
};

// Launchers (encode_lossless.hip); stream is a hipStream_t.
void EncLaunchTokenise(const EncPlan& p, void* stream);      // histograms + range flags
void EncLaunchCount(const EncPlan& p, void* stream);         // row_off, sec_bytes, sec_off
void EncLaunchPack(const EncPlan& p, void* stream);          // the bits

}  // namespace jxlhip
