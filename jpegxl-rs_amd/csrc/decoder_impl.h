// What the host translation units of the batch decoder share beyond decoder.h (decoder.cc, frame_tail.cc).
#pragma once
#include "decoder.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>

namespace jxlhip {

#define HIP_CHECK(expr)                                                                                    \
  do {                                                                                                     \
    hipError_t e_ = (expr);                                                                                \
    if (e_ != hipSuccess) throw ParseError(std::string("HIP error: ") + hipGetErrorString(e_) + " in " #expr, false); \
  } while (0)

inline size_t Align(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// appends to the buffer the constant arena is assembled in; returns the offset
struct Arena {
  HostStage& buf;
  explicit Arena(HostStage& b) : buf(b) {}
  size_t Put(const void* src, size_t n, size_t align = 256) {
    const size_t off = Align(buf.size(), align), end = off + std::max<size_t>(n, 4);
    buf.Resize(end);                                   // (the gap before `off` and a short tail are zeroed)
    if (n) memcpy(buf.data() + off, src, n);
    return off;
  }
};

void FillColor(const ImageHeader& ih, bool do_ycbcr, FrameDev& f);
void FillColourConversion(const ImageHeader& ih, const OutputSpec& o, ColorArgs* ca);      // ColorKernel's conversion of an image that is not XYB to o.color
OutputDesc FillOutput(const ImageEntry& e, uint8_t* work, uint8_t* big, bool resize_target = false);
// ... and requested extra-channel plane k (OutputSpec::planes) in the caller's destination: one planar slot with the plane's own type, byte order, row pitch, scale / bias
OutputDesc FillPlaneOutput(const ImageEntry& e, size_t k, uint8_t* work, bool resize_target = false);
void DebugSync(const char* what, void* stream);     // under JXL_HIP_DEBUG_SYNC: names the stage on stderr and waits for it

}  // namespace jxlhip
