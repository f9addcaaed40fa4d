// jxl-hip: kernels of the frame "tail" that images with more than one frame or with image features take (gfx950):
// integer Modular planes -> float, patches, splines, upsampling, noise, colour transform, blending onto the canvas and the
// write stage — libjxl's render_pipeline stages stage_{patches,splines,upsampling,noise,xyb,from_linear,ycbcr,blending,write}.cc,
// reached by the reference through JxlDecoderProcessInput (jpegxl-rs/src/decode.rs:238).  Explicit arguments, one launch per
// stage and frame, planned by the host (decoder.cc PlanPostOps): these stages are plain streaming passes over the planes
// (HBM-bound, 8..24 B/px each), only frames that need them pay for them — single-frame images without features keep the
// fused tile kernels of kernels.hip.  Arithmetic and operation order are those of oracle/image_features.h; upsampling, colour
// transform, transfer function and the write are pixel_ops.h's, shared with those kernels.
#include "kernels.h"
#include "pixel_ops.h"
#include "host_parse.h"
#include <hip/hip_runtime.h>
#include <math.h>

namespace jxlhip {

namespace {

__device__ __forceinline__ float Clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }

// base/fast_math-inl.h
__device__ __forceinline__ float FastErffD(float x) {
  const float absx = fabsf(x);
  float d = fmaf(absx, 7.77394369e-02f, 2.05260015e-04f);
  d = fmaf(d, absx, 2.32120216e-01f);
  d = fmaf(d, absx, 2.77820801e-01f);
  d = fmaf(d, absx, 1.0f);
  const float d2 = d * d;
  const float inv = 1.0f / d2;
  const float r = fmaf(-inv, inv, 1.0f);
  return x <= 0.0f ? -r : r;
}

// ---- integer Modular planes -> float planes (dec_modular.cc ModularImageToDecodedRect) ---------------------------------
__global__ void IntToFloatKernel(const int32_t* __restrict__ src, uint32_t src_stride, float* __restrict__ dst, uint32_t dst_stride, uint32_t w, uint32_t h, float factor,
                                 uint32_t float_bits, uint32_t float_exp_bits) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const int32_t v = src[(size_t)y * src_stride + x];
  dst[(size_t)y * dst_stride + x] = float_bits ? IntToFloatSample(v, float_bits, float_exp_bits) : (float)v * factor;
}
// XYB Modular frames code Y, X, B - Y; factors = the LF dequantisation factors (DequantMatrices::DCQuants)
__global__ void XybModToFloatKernel(const int32_t* __restrict__ cy, const int32_t* __restrict__ cx, const int32_t* __restrict__ cb, uint32_t src_stride,
                                    float* dx, float* dy, float* db, uint32_t dst_stride, uint32_t w, uint32_t h, float fx, float fy, float fb) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t si = (size_t)y * src_stride + x, di = (size_t)y * dst_stride + x;
  const int32_t vy = cy[si];
  dx[di] = (float)cx[si] * fx;
  dy[di] = (float)vy * fy;
  db[di] = (float)(cb[si] + vy) * fb;
}

// ---- patches (stage_patches.cc; blending.cc PerformBlending) ---------------------------------------------------------------
__device__ __forceinline__ float PatchBlendSample(uint32_t mode, bool clamp, bool premultiplied, float frame, float patch, float frame_a, float patch_a) {
  switch (mode) {
    case 0: return frame;
    case 1: return patch;
    case 2: return frame + patch;
    case 3: return frame * (clamp ? Clamp01(patch) : patch);
    case 4: case 5: {
      const bool above = mode == 4;
      const float fg = above ? patch : frame, bg = above ? frame : patch;
      float fa = above ? patch_a : frame_a; const float ba = above ? frame_a : patch_a;
      if (clamp) fa = Clamp01(fa);
      if (premultiplied) return fg + bg * (1.0f - fa);
      const float new_a = 1.0f - (1.0f - fa) * (1.0f - ba);
      const float rnew_a = new_a > 0 ? 1.0f / new_a : 0.0f;
      return (fg * fa + bg * ba * (1.0f - fa)) * rnew_a;
    }
    case 6: { const float a = clamp ? Clamp01(patch_a) : patch_a; return frame + patch * a; }
    default: { const float a = clamp ? Clamp01(frame_a) : frame_a; return patch + frame * a; }
  }
}
__device__ __forceinline__ float PatchBlendAlpha(uint32_t mode, bool clamp, float frame_a, float patch_a) {
  switch (mode) {
    case 4: case 5: {
      float fa = mode == 4 ? patch_a : frame_a; const float ba = mode == 4 ? frame_a : patch_a;
      if (clamp) fa = Clamp01(fa);
      return 1.0f - (1.0f - fa) * (1.0f - ba);
    }
    case 6: return frame_a;
    default: return patch_a;
  }
}

// One workgroup per 32x32 tile of the frame; the tile's list names, in dictionary order, the patch placements that touch it, so
// every pixel sees its patches in the order libjxl applies them (float additions do not commute).  An extra channel's new value goes
// to its `tmp` plane first and comes back once every channel and the colour of the pixel have read the values from before the patch:
// the alpha a blending refers to may be any channel, also one that the same patch changes.
__global__ __launch_bounds__(256) void PatchKernel(PatchFrameArgs a, const EcChanDev* __restrict__ table, const PatchEntryDev* __restrict__ entries,
                                                   const PatchEcDev* __restrict__ pec, const uint32_t* __restrict__ tile_start,
                                                   const uint32_t* __restrict__ tile_list, uint32_t tiles_x) {
  const uint32_t tile = blockIdx.x;
  const uint32_t begin = tile_start[tile], end = tile_start[tile + 1];
  if (begin == end) return;
  const uint32_t tx = tile % tiles_x, ty = tile / tiles_x;
  for (uint32_t t = threadIdx.x; t < 1024; t += blockDim.x) {
    const int x = (int)(tx * 32 + (t & 31)), y = (int)(ty * 32 + (t >> 5));
    if (x >= (int)a.w || y >= (int)a.h) continue;
    const size_t fo = (size_t)y * a.stride + x, eo = (size_t)y * a.ec_stride + x;
    for (uint32_t k = begin; k < end; k++) {
      const uint32_t ei = tile_list[k];
      const PatchEntryDev& e = entries[ei];
      const PatchEcDev* __restrict__ pe = pec + (size_t)ei * a.num_extra;
      const int ix = x - e.x, iy = y - e.y;
      if (ix < 0 || iy < 0 || ix >= (int)e.xs || iy >= (int)e.ys) continue;
      const size_t so = (size_t)iy * e.src_stride + ix, seo = (size_t)iy * e.esrc_stride + ix;
      const uint32_t m0 = e.mode & 0xFF, a0 = (e.mode >> 8) & 0xFF; const bool c0 = (e.mode >> 16) & 1;
      float fa = 1.0f, pa = 1.0f; bool premul = false;
      if (m0 >= 4) { fa = table[a0].plane[eo]; pa = pe[a0].src[seo]; premul = table[a0].premul != 0; }
      for (uint32_t c = 0; c < a.num_extra; c++) {
        const uint32_t m = pe[c].mode & 0xFF, ac = (pe[c].mode >> 8) & 0xFF; const bool cl = (pe[c].mode >> 16) & 1;
        const float fv = table[c].plane[eo], pv = pe[c].src[seo];
        float efa = 1.0f, epa = 1.0f;
        if (m >= 4) { efa = table[ac].plane[eo]; epa = pe[ac].src[seo]; }
        float o;
        if (m >= 4 && ac == c) o = PatchBlendAlpha(m, cl, efa, epa);
        else o = PatchBlendSample(m, cl, m >= 4 ? table[ac].premul != 0 : false, fv, pv, efa, epa);
        table[c].tmp[eo] = o;
      }
      for (int c = 0; c < 3; c++) a.p[c][fo] = PatchBlendSample(m0, c0, premul, a.p[c][fo], e.src[c][so], fa, pa);
      for (uint32_t c = 0; c < a.num_extra; c++) table[c].plane[eo] = table[c].tmp[eo];
    }
  }
}

// ---- splines (stage_splines.cc; splines.cc DrawSegment) --------------------------------------------------------------------
// One thread per pixel; the row's segment list is walked in order (ascending segment index, as Splines::Apply does), the
// contributions are added one by one — same order of float additions per pixel as the scalar reference.
__global__ __launch_bounds__(256) void SplineKernel(float* p0, float* p1, float* p2, uint32_t stride, uint32_t w, uint32_t h, const SplineSegmentDev* __restrict__ segs,
                                                    const uint32_t* __restrict__ row_start, const uint32_t* __restrict__ indices) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const uint32_t begin = row_start[y], end = row_start[y + 1];
  if (begin == end) return;
  const size_t o = (size_t)y * stride + x;
  float v0 = p0[o], v1 = p1[o], v2 = p2[o];
  bool touched = false;
  for (uint32_t i = begin; i < end; i++) {
    const SplineSegmentDev s = segs[indices[i]];
    // column range of the segment: [llround(cx - maxdist), llround(cx + maxdist)]
    const long long x0 = llroundf(s.center_x - s.maximum_distance), x1 = llroundf(s.center_x + s.maximum_distance) + 1;
    if ((long long)x < x0 || (long long)x >= x1) continue;
    const float dx = (float)x - s.center_x, dy = (float)y - s.center_y;
    const float sqd = fmaf(dx, dx, dy * dy);
    const float distance = sqrtf(sqd);
    const float f = FastErffD(fmaf(distance, 0.5f, 0.353553391f) * s.inv_sigma) - FastErffD(fmaf(distance, 0.5f, -0.353553391f) * s.inv_sigma);
    const float local_intensity = s.sigma_over_4_times_intensity * (f * f);
    v0 = fmaf(s.color[0], local_intensity, v0);
    v1 = fmaf(s.color[1], local_intensity, v1);
    v2 = fmaf(s.color[2], local_intensity, v2);
    touched = true;
  }
  if (touched) { p0[o] = v0; p1[o] = v1; p2[o] = v2; }
}

// ---- upsampling of one plane (stage_upsampling.cc: UpsampleSample) -------------------------------------------------------------
__global__ void UpsamplePlaneKernel(const float* __restrict__ src, uint32_t src_stride, int w, int h, float* __restrict__ dst, uint32_t dst_stride, int ow, int oh,
                                    int up, const float* __restrict__ weights) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y * blockDim.y + threadIdx.y;
  if (ox >= ow || oy >= oh) return;
  dst[(size_t)oy * dst_stride + ox] = UpsampleSample([&](int x, int y) { return src[(size_t)y * src_stride + x]; }, w, h, ox, oy, up, weights);
}
// ---- the same two steps for every extra channel of a frame: channel on blockIdx.z (the table entry is wave-uniform)
__global__ void EcIntToFloatKernel(EcFrameArgs a) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  const EcChanDev& c = a.table[blockIdx.z];
  const size_t o = (size_t)y * a.w + x;
  const int32_t v = c.src_int[o];
  c.plane[o] = c.float_bits ? IntToFloatSample(v, c.float_bits, c.float_exp_bits) : (float)v * c.factor;
}
__global__ void EcUpsampleKernel(EcFrameArgs a) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y * blockDim.y + threadIdx.y;
  if (ox >= (int)a.ow || oy >= (int)a.oh) return;
  const EcChanDev& c = a.table[blockIdx.z];
  c.up[(size_t)oy * a.ow + ox] = UpsampleSample([&](int x, int y) { return c.plane[(size_t)y * a.w + x]; }, (int)a.w, (int)a.h, ox, oy, (int)a.up, a.up_weights);
}

// ---- noise (dec_noise.cc Random3Planes, stage_noise.cc) --------------------------------------------------------------------
__device__ __forceinline__ uint64_t SplitMix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// One workgroup per 256x256 group (upsampled coordinates), one lane per Xorshift128+ generator (8 independent ones, base/random.h):
// lane i produces floats 2i and 2i+1 of every 16-float batch; a row of xs samples takes ceil(xs / 16) batches, three planes in turn.
__global__ __launch_bounds__(64) void NoiseRandomKernel(float* n0, float* n1, float* n2, uint32_t stride, uint32_t w, uint32_t h, uint32_t group_dim,
                                                        uint32_t visible_frame_index, uint32_t nonvisible_frame_index) {
  const uint32_t i = threadIdx.x;
  if (i >= 8) return;
  const uint32_t gx0 = blockIdx.x * group_dim, gy0 = blockIdx.y * group_dim;
  if (gx0 >= w || gy0 >= h) return;
  uint64_t s0 = SplitMix64((((uint64_t)visible_frame_index << 32) + nonvisible_frame_index) + 0x9E3779B97F4A7C15ull);
  uint64_t s1 = SplitMix64((((uint64_t)gx0 << 32) + gy0) + 0x9E3779B97F4A7C15ull);
  for (uint32_t k = 0; k < i; k++) { s0 = SplitMix64(s0); s1 = SplitMix64(s1); }
  const uint32_t xs = min(group_dim, w - gx0), ys = min(group_dim, h - gy0);
  float* planes[3] = {n0, n1, n2};
  for (int c = 0; c < 3; c++) {
    for (uint32_t y = 0; y < ys; y++) {
      float* row = planes[c] + (size_t)(gy0 + y) * stride + gx0;
      for (uint32_t x = 0; x < xs; x += 16) {
        uint64_t a = s0; const uint64_t b = s1;
        const uint64_t bits = a + b;
        s0 = b;
        a ^= a << 23;
        a ^= b ^ (a >> 18) ^ (b >> 5);
        s1 = a;
        const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
        if (x + 2 * i < xs) row[x + 2 * i] = __uint_as_float((lo >> 9) | 0x3F800000u);
        if (x + 2 * i + 1 < xs) row[x + 2 * i + 1] = __uint_as_float((hi >> 9) | 0x3F800000u);
      }
    }
  }
}
__device__ __forceinline__ float NoiseStrength(const float* lut, float vx) {
  const float kScale = 6.0f;
  const float scaled = fmaxf(0.0f, vx * kScale);
  float floor_x = floorf(scaled), frac = scaled - floor_x;
  if (scaled >= kScale + 1) { floor_x = kScale; frac = 1.0f; }
  const int i = (int)floor_x;
  const float low = lut[i], hi = lut[i + 1];
  const float v = fmaf(hi - low, frac, low);
  return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}
__global__ void NoiseAddKernel(NoiseArgs a) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  const int w = (int)a.w, h = (int)a.h;
  if (x >= w || y >= h) return;
  float conv[3];
  int xs[5], ys[5];
  for (int i = 0; i < 5; i++) { xs[i] = MirrorD(x + i - 2, w); ys[i] = MirrorD(y + i - 2, h); }
  for (int c = 0; c < 3; c++) {
    const float* n = a.noise[c];
    auto px = [&](int r, int dx) { return n[(size_t)ys[r] * a.noise_stride + xs[dx + 2]]; };
    const float p00 = px(2, 0);
    float others = 0.0f;
    for (int i = -2; i <= 2; i++) { others += px(0, i); others += px(1, i); others += px(3, i); others += px(4, i); }
    others += px(2, -2); others += px(2, -1); others += px(2, 1); others += px(2, 2);
    conv[c] = fmaf(others, 0.16f, p00 * -3.84f);
  }
  const float kNorm = 0.22f, kRGCorr = 0.9921875f, kRGNCorr = 0.0078125f;
  const size_t o = (size_t)y * a.stride + x;
  const float vx = a.p[0][o], vy = a.p[1][o];
  const float in_g = vy - vx, in_r = vy + vx;
  const float sg = NoiseStrength(a.lut, in_g * 0.5f), sr = NoiseStrength(a.lut, in_r * 0.5f);
  const float ar = conv[0] * kNorm, ag = conv[1] * kNorm, ac = conv[2] * kNorm;
  const float red = sr * fmaf(kRGNCorr, ar, kRGCorr * ac);
  const float green = sg * fmaf(kRGNCorr, ag, kRGCorr * ac);
  const float rg = red + green;
  a.p[0][o] = fmaf(a.ytox, rg, red - green) + vx;
  a.p[1][o] = vy + rg;
  a.p[2][o] = fmaf(a.ytob, rg, a.p[2][o]);
}

// ---- colour transform to the output space (stage_xyb.cc, stage_from_linear.cc, stage_ycbcr.cc: XybToLinear, TransferFromLinear, YcbcrToRgb)
__global__ void ColorKernel(ColorArgs a) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  const size_t si = (size_t)y * a.src_stride + x, di = (size_t)y * a.dst_stride + x;
  const float X = a.src[0][si], Y = a.src[1][si], B = a.src[2][si];
  float r, g, b;
  if (a.mode == 0) {          // XYB -> linear -> transfer function
    XybToLinear(a, X, Y, B, r, g, b);
    const float3 t = TransferFromLinear(a, a.tf_kind, r, g, b); r = t.x; g = t.y; b = t.z;
  } else if (a.mode == 1) YcbcrToRgb(X, Y, B, r, g, b);   // (planes Cb, Y, Cr)
  else if (a.mode == 3) {     // transfer function only: the planes hold linear light (a spot-colour stage came in between)
    r = X; g = Y; b = B;
    const float3 t = TransferFromLinear(a, a.tf_kind, r, g, b); r = t.x; g = t.y; b = t.z;
  } else { r = X; g = Y; b = B; }
  // an image that is not XYB on its way to a requested encoding (ColorArgs::convert, modes 1 and 2): its transfer function undone, the matrix between the two sets of
  // primaries, the target's transfer function.  Every switch is on a kernel argument: scalar branches.
  if (a.convert && (a.mode == 1 || a.mode == 2)) {
    const float3 l = TransferToLinear(a.src_par, a.src_tf, r, g, b);
    r = l.x; g = l.y; b = l.z;
    if (!a.conv_identity) {
      r = fmaf(a.conv[2], l.z, fmaf(a.conv[1], l.y, a.conv[0] * l.x));
      g = fmaf(a.conv[5], l.z, fmaf(a.conv[4], l.y, a.conv[3] * l.x));
      b = fmaf(a.conv[8], l.z, fmaf(a.conv[7], l.y, a.conv[6] * l.x));
    }
    const float3 t = TransferFromLinear(a, a.tf_kind, r, g, b); r = t.x; g = t.y; b = t.z;
  }
  a.dst[0][di] = r; a.dst[1][di] = g; a.dst[2][di] = b;
}

// ---- chroma upsampling of subsampled YCbCr frames (stage_chroma_upsampling.cc: SubsampledSample), one thread per output sample
struct ChromaUpArgs { const float* src; float* dst; uint32_t src_stride, dst_stride, hs, vs, out_w, out_h; };
__global__ void ChromaUpsampleKernel(ChromaUpArgs a) {
  const uint32_t X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X >= a.out_w || Y >= a.out_h) return;
  a.dst[(size_t)Y * a.dst_stride + X] = SubsampledSample(a.src, a.src_stride, a.hs, a.vs, a.out_w, a.out_h, X, Y);
}

// ---- blending of a frame onto the image canvas (stage_blending.cc; blending.cc) ----------------------------------------------
__device__ __forceinline__ float FrameBlendSampleD(uint32_t mode, bool clamp, bool premultiplied, float bg, float fg, float bga, float fga) {
  switch (mode) {
    case 0: return fg;
    case 1: return bg + fg;
    case 2: {
      const float fa = clamp ? Clamp01(fga) : fga;
      if (premultiplied) return fg + bg * (1.0f - fa);
      const float new_a = 1.0f - (1.0f - fa) * (1.0f - bga);
      const float rnew_a = new_a > 0 ? 1.0f / new_a : 0.0f;
      return (fg * fa + bg * bga * (1.0f - fa)) * rnew_a;
    }
    case 3: { const float fa = clamp ? Clamp01(fga) : fga; return bg + fg * fa; }
    default: return bg * (clamp ? Clamp01(fg) : fg);
  }
}
// the alpha channel's own update under modes 2 (blend) / 3 (alpha-weighted add: the background's alpha stays)
__device__ __forceinline__ float FrameBlendAlphaD(uint32_t mode, bool clamp, float bga, float fga) {
  const float fa = clamp ? Clamp01(fga) : fga;
  return mode == 2 ? 1.0f - (1.0f - fa) * (1.0f - bga) : bga;
}
// Colour: the foreground alpha is read through the channel table (null without extra channels: such a frame has no alpha to blend against).
__global__ void BlendColorKernel(BlendArgs a, const EcChanDev* __restrict__ table) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X >= (int)a.img_w || Y >= (int)a.img_h) return;
  const size_t co = (size_t)Y * a.canvas_stride + X, bo = (size_t)Y * a.bg_stride + X;
  const int fx = X - a.x0, fy = Y - a.y0;
  const bool inside = fx >= 0 && fy >= 0 && fx < (int)a.fw && fy < (int)a.fh;
  if (!inside) {
    for (int c = 0; c < 3; c++) a.canvas[c][co] = a.bg[0] ? a.bg[c][bo] : 0.0f;
    return;
  }
  const size_t fo = (size_t)fy * a.fg_stride + fx;
  const uint32_t mode = a.mode & 0xFF, ach = (a.mode >> 8) & 0xFF; const bool clamp = (a.mode >> 16) & 1;
  float fga = 1.0f, bga = 1.0f; bool premul = false;
  if (mode == 2 || mode == 3) {
    const EcChanDev& al = table[ach];
    fga = al.fg[(size_t)fy * al.fg_stride + fx];
    bga = a.bg_alpha ? a.bg_alpha[(size_t)Y * a.bg_alpha_stride + X] : 0.0f;
    premul = al.premul != 0;
  }
  for (int c = 0; c < 3; c++) {
    const float b = a.bg[0] ? a.bg[c][bo] : 0.0f;
    a.canvas[c][co] = FrameBlendSampleD(mode, clamp, premul, b, a.fg[c][fo], bga, fga);
  }
}
// Extra channels: channel on blockIdx.z.  Every read is of a foreground plane or of a plane of the source (the canvas as an earlier frame left it),
// every write goes to this frame's own canvas plane of the channel: no slice reads what another one writes.
__global__ void BlendEcKernel(BlendArgs a, const EcChanDev* __restrict__ table) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y * blockDim.y + threadIdx.y;
  if (X >= (int)a.img_w || Y >= (int)a.img_h) return;
  const uint32_t e = blockIdx.z;
  const EcChanDev& c = table[e];
  const size_t bo = (size_t)Y * c.bg_stride + X;
  const float b = c.bg ? c.bg[bo] : 0.0f;
  float* out = c.canvas + (size_t)Y * c.canvas_stride + X;
  const int fx = X - a.x0, fy = Y - a.y0;
  if (!(fx >= 0 && fy >= 0 && fx < (int)a.fw && fy < (int)a.fh)) { *out = b; return; }
  const uint32_t m = c.mode & 0xFF, ac = (c.mode >> 8) & 0xFF; const bool cl = (c.mode >> 16) & 1;
  const float fv = c.fg[(size_t)fy * c.fg_stride + fx];
  float o;
  if (m == 2 || m == 3) {
    const EcChanDev& al = table[ac];
    const float efga = al.fg[(size_t)fy * al.fg_stride + fx];
    const float ebga = c.bg_alpha ? c.bg_alpha[bo] : 0.0f;
    if (ac == e) o = FrameBlendAlphaD(m, cl, ebga, efga);
    else o = FrameBlendSampleD(m, cl, al.premul != 0, b, fv, ebga, efga);
  } else o = FrameBlendSampleD(m, cl, false, b, fv, 1.0f, 1.0f);
  *out = o;
}
// ---- spot colours (stage_spot.cc): one thread per pixel walks the channels in header order (each mix reads what the one before it wrote)
__global__ void SpotKernel(float* p0, float* p1, float* p2, uint32_t stride, const EcChanDev* __restrict__ table, uint32_t num_extra, uint32_t use_canvas,
                           uint32_t w, uint32_t h) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t o = (size_t)y * stride + x;
  float v[3] = {p0[o], p1[o], p2[o]};
  for (uint32_t e = 0; e < num_extra; e++) {
    const EcChanDev& c = table[e];
    if (c.type != 2) continue;
    const float s = use_canvas ? c.canvas[(size_t)y * c.canvas_stride + x] : c.fg[(size_t)y * c.fg_stride + x];
    const float mix = c.spot[3] * s;
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = mix * c.spot[k] + (1.0f - mix) * v[k];
  }
  p0[o] = v[0]; p1[o] = v[1]; p2[o] = v[2];
}

// ---- write stage (stage_write.cc): float planes in the output colour space -> caller layout (StorePixel) ---------------------
__global__ void WriteKernel(WriteArgs a) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  const int w = (int)a.img_w, h = (int)a.img_h;
  if (x >= w || y >= h) return;
  const size_t o = (size_t)y * a.stride + x;
  float r = a.p[0][o], g = a.p[1][o], b = a.p[2][o];
  float al = 1.0f;
  if (a.alpha) {
    al = a.alpha[(size_t)y * a.alpha_stride + x];
    if (a.unpremul) {   // alpha.cc UnpremultiplyAlpha: colour / max(alpha, 2^-26)
      const float m = 1.0f / fmaxf(1.0f / (float)(1u << 26), al);
      r *= m; g *= m; b *= m;
    }
  }
  StorePixel(a.od, w, h, x, y, r, g, b, al);
}

// ---- extra-channel planes beside the colour output (OutputSpec::planes): a float plane of the finished image -> one plane of the caller's layout ---------------
// A streaming pass like EcIntToFloatKernel: lanes along x, rows on blockIdx.y (a block walks rows blockIdx.y, blockIdx.y + gridDim.y, ...: the grid's y extent is
// limited, an image's height is not), the requested plane on blockIdx.z — its table entry is the same for every lane of the block (scalar loads) and the same channel
// may stand in several entries.  Every lane stays inside w x h of its source; OutPixelPtr maps that rectangle onto the oriented one the host sized the destination
// for.  No LDS.  The conversion is pixel_ops.h's, as for every other sample the decoder stores.
__global__ __launch_bounds__(256) void EcPlanesOutKernel(EcPlanesOutArgs a) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= a.w) return;
  const EcPlaneOutDev& e = a.table[blockIdx.z];
  const uint32_t bps = e.od.out_type == 0 ? 1 : e.od.out_type == 2 ? 4 : 2;
  for (uint32_t y = blockIdx.y; y < a.h; y += gridDim.y) {
    const float v = e.src[(size_t)y * e.src_stride + x];
    StoreSample(e.od, OutPixelPtr(e.od, (int)a.w, (int)a.h, (int)x, (int)y, bps), SlotValue(e.od, 0, v));
  }
}

__global__ void CopyPlaneKernel(const float* __restrict__ src, uint32_t src_stride, float* __restrict__ dst, uint32_t dst_stride, uint32_t w, uint32_t h) {
  const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  dst[(size_t)y * dst_stride + x] = src[(size_t)y * src_stride + x];
}

// ---- resized output (OutputSpec::resize_w / resize_h) --------------------------------------------------------------------------------------
// Separable antialiased filter (triangle or cubic: the weights are the host's, ResizeAxis) over the f32 picture the write stage left (decoder.cc FillOutput): the horizontal pass (kVertical = false) turns the rows of the
// resampled rectangle into rows of out_w pixels in `tmp`, the vertical pass turns those into the out_w x out_h target and stores it through SlotValue / StoreSample /
// OutPixelPtr — type, byte order, bit depth, row alignment, planes and scale / bias as for every other output.  The host built each axis' taps (ResizeAxis: first sample,
// normalised f32 weights); a thread owns one pixel, all NC slots, and walks its taps — as many as the ratio asks for — with one fmaf per tap, the first tap a plain product
// (a copy at ratio 1 stays bit-exact).  A wavefront is 64 neighbouring pixels of one row: horizontally their tap windows adjoin or overlap, so the wave reads one
// contiguous stretch of the row and every later tap finds its line in the vector L1; vertically the lanes read 64 neighbouring pixels of the same row of `tmp` per tap and
// lo / first / weight are wave-uniform.  No LDS, nothing that grows with the ratio but the trip count.
// One launch serves a group of images of NC slots: blockIdx.z picks the image's entry of the device table (Batch::Prepare wrote it), read once per block into scalar
// registers — the entry is the same for every lane and nothing is stored before it has been read; the grid spans the group's largest extents and a block outside its own
// image's returns at once.  mirror: the finished target pixel ox is stored at column out_w - 1 - ox (a flip of the result: sources, taps and sums are untouched).
template <int NC, bool kVertical> __global__ __launch_bounds__(256) void ResizeKernel(const ResizeArgs* __restrict__ table) {
  const ResizeArgs a = table[blockIdx.z];
  const uint32_t ox = blockIdx.x * 64 + threadIdx.x;
  if (ox >= a.out_w) return;
  float acc[NC];
  if (!kVertical) {
    const uint32_t lo = a.ax.lo[ox], t0 = a.ax.first[ox], nt = a.ax.first[ox + 1] - t0;
    const float* __restrict__ wt = a.ax.weight + t0;
    for (uint32_t y = blockIdx.y * 4 + threadIdx.y; y < a.in_h; y += gridDim.y * 4) {
      const float* __restrict__ in = a.src + (size_t)(a.y0 + y) * a.src_stride + (size_t)(a.x0 + lo) * NC;
      const float w0 = wt[0];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = w0 * in[c];
      for (uint32_t j = 1; j < nt; j++) {
        const float w = wt[j];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = fmaf(w, in[(size_t)j * NC + c], acc[c]);
      }
      float* __restrict__ out = a.tmp + ((size_t)y * a.out_w + ox) * NC;
#pragma unroll
      for (int c = 0; c < NC; c++) out[c] = acc[c];
    }
  } else {
    const uint32_t oy = blockIdx.y * 4 + threadIdx.y;
    if (oy >= a.out_h) return;
    const uint32_t lo = a.ay.lo[oy], t0 = a.ay.first[oy], nt = a.ay.first[oy + 1] - t0;
    const float* __restrict__ wt = a.ay.weight + t0;
    const size_t pitch = (size_t)a.out_w * NC;
    const float* __restrict__ in = a.tmp + (size_t)lo * pitch + (size_t)ox * NC;
    const float w0 = wt[0];
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = w0 * in[c];
    for (uint32_t j = 1; j < nt; j++) {
      const float w = wt[j];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = fmaf(w, in[(size_t)j * pitch + c], acc[c]);
    }
    const uint32_t bps = a.od.out_type == 0 ? 1 : a.od.out_type == 2 ? 4 : 2;
    uint8_t* const p = OutPixelPtr(a.od, (int)a.out_w, (int)a.out_h, (int)(a.mirror ? a.out_w - 1 - ox : ox), (int)oy, bps);
    const size_t step = a.od.planar ? (size_t)a.od.plane_stride : (size_t)bps;
#pragma unroll
    for (int c = 0; c < NC; c++) StoreSample(a.od, p + c * step, SlotValue(a.od, c, acc[c]));
  }
}

// ---- integer resample of libjpeg-exact outputs (OutputSpec::resize_u8; the rule: include/jxl_hip.h, JxlHipBatchSetOutputJpegResampled) -----------------------------------
// Pillow's 8-bit resize over the u8 picture the libjpeg-exact write stage left (decoder.cc FillOutput: interleaved u8, every slot of the output): the same two passes, the
// same table entry, grid and grouping as ResizeKernel — entries with ResizeArgs::u8 set, whose src / tmp are bytes and whose weights are the host's int32 kk
// (ResizeAxisInt) — in int32: a sample is clamp((2^21 + sum p x kk) >> 22, 0, 255), arithmetic shift, once behind the horizontal pass (u8 `tmp`) and once behind the
// vertical one.  The finished k goes out as the libjpeg-exact write stage stores a sample: (float)k x (1 / 255) through SlotValue / StoreSample, which gives k for u8 and
// 257 k for u16.  A lane reads its taps byte by byte: 64 neighbouring pixels' windows adjoin or overlap, so a wave's taps fall into a few lines of the vector L1, as in
// ResizeKernel; the sum of |kk| x 255 stays below 2^31 for both filters (the normalised weights' absolute sum is below 2: the centre's own sample is always in the range, so the positive lobe
// outweighs the cubic's negative ones by far more than three to one).
__device__ __forceinline__ int32_t ResizeU8Round(int32_t acc) { return min(max((acc + (1 << 21)) >> 22, 0), 255); }
template <int NC, bool kVertical> __global__ __launch_bounds__(256) void ResizeU8Kernel(const ResizeArgs* __restrict__ table) {
  const ResizeArgs a = table[blockIdx.z];
  const uint32_t ox = blockIdx.x * 64 + threadIdx.x;
  if (ox >= a.out_w) return;
  const uint8_t* __restrict__ const tmp_in = (const uint8_t*)a.tmp;
  int32_t acc[NC];
  if (!kVertical) {
    const uint32_t lo = a.ax.lo[ox], t0 = a.ax.first[ox], nt = a.ax.first[ox + 1] - t0;
    const int32_t* __restrict__ wt = (const int32_t*)a.ax.weight + t0;
    uint8_t* __restrict__ const tmp_out = (uint8_t*)a.tmp;
    for (uint32_t y = blockIdx.y * 4 + threadIdx.y; y < a.in_h; y += gridDim.y * 4) {
      const uint8_t* __restrict__ in = (const uint8_t*)a.src + (size_t)(a.y0 + y) * a.src_stride + (size_t)(a.x0 + lo) * NC;
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = 0;
      for (uint32_t j = 0; j < nt; j++) {
        const int32_t w = wt[j];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] += (int32_t)in[(size_t)j * NC + c] * w;
      }
      uint8_t* __restrict__ out = tmp_out + ((size_t)y * a.out_w + ox) * NC;
#pragma unroll
      for (int c = 0; c < NC; c++) out[c] = (uint8_t)ResizeU8Round(acc[c]);
    }
  } else {
    const uint32_t oy = blockIdx.y * 4 + threadIdx.y;
    if (oy >= a.out_h) return;
    const uint32_t lo = a.ay.lo[oy], t0 = a.ay.first[oy], nt = a.ay.first[oy + 1] - t0;
    const int32_t* __restrict__ wt = (const int32_t*)a.ay.weight + t0;
    const size_t pitch = (size_t)a.out_w * NC;
    const uint8_t* __restrict__ in = tmp_in + (size_t)lo * pitch + (size_t)ox * NC;
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = 0;
    for (uint32_t j = 0; j < nt; j++) {
      const int32_t w = wt[j];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] += (int32_t)in[(size_t)j * pitch + c] * w;
    }
    const uint32_t bps = a.od.out_type == 0 ? 1 : a.od.out_type == 2 ? 4 : 2;
    uint8_t* const p = OutPixelPtr(a.od, (int)a.out_w, (int)a.out_h, (int)(a.mirror ? a.out_w - 1 - ox : ox), (int)oy, bps);
    const size_t step = a.od.planar ? (size_t)a.od.plane_stride : (size_t)bps;
    const float k255 = 1.0f / 255;
#pragma unroll
    for (int c = 0; c < NC; c++) StoreSample(a.od, p + c * step, SlotValue(a.od, c, (float)ResizeU8Round(acc[c]) * k255));
  }
}

// ---- JPEG reconstruction: coefficients back into JPEG layout --------------------------------------------------------------------------
__global__ void JpegCoefKernel(const FrameDev* __restrict__ frames, int fidx, JpegCoefArgs a) {
  const FrameDev& f = frames[fidx];
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;       // (block, natural coefficient index)
  const uint32_t nblk = f.bw * f.bh;
  if (t >= nblk * 64 || *f.status != 0) return;      // (a frame whose entropy stages failed has no usable coefficient offsets)
  const uint32_t o = t >> 6, i = t & 63, v = i >> 3, u = i & 7;
  const uint32_t bx = o % f.bw, by = o / f.bw;
  const uint32_t g = (by / 32) * f.xgroups + bx / 32;
  const size_t base = (size_t)g * 65536 + f.coef_off[o] + (u * 8 + v);   // libjxl stores the transpose of JPEG's (v, u) layout
  if (f.subsampled) {
    // chroma-subsampled frames carry no chroma-from-luma (the LF stage rejects it); a channel's block (sx, sy) keeps its coefficients at
    // the slot of block (sx << hs, sy << vs) and its LF sample at (sx, sy) of the padded grid; component planes are packed one after another
    for (uint32_t c = 0; c < a.ncomp; c++) {
      const int ch = c == 0 ? 1 : c == 1 ? 0 : 2;
      const uint32_t hs = f.hs[ch], vs = f.vs[ch];
      if ((bx & ((1u << hs) - 1u)) | (by & ((1u << vs) - 1u))) continue;
      const uint32_t sx = bx >> hs, sy = by >> vs, cw = f.bw >> hs;
      const int32_t val = i == 0 ? f.lfq[ch][(size_t)sy * f.bw + sx] : f.coeff[ch][base];
      a.out[((size_t)a.comp_off[c] + (size_t)sy * cw + sx) * 64 + i] = (int16_t)val;
    }
    return;
  }
  const int32_t y = i == 0 ? f.lfq[1][o] : f.coeff[1][base];
  if (a.ncomp == 1) { a.out[(size_t)o * 64 + i] = (int16_t)y; return; }
  a.out[(size_t)o * 64 + i] = (int16_t)y;
  const size_t tile = (size_t)(by / 8) * f.cw + bx / 8;
  for (int c = 1; c < 3; c++) {
    const int ch = c == 1 ? 0 : 2;                                    // Cb rides in the X slot, Cr in the B slot
    int32_t val;
    if (i == 0) val = f.lfq[ch][o];
    else {
      const int32_t fac = c == 1 ? (int32_t)f.ytox[tile] : (int32_t)f.ytob[tile];
      const int32_t ff = fac * 2048 / 84;                             // (C++ division: truncates toward zero)
      const int32_t scale = (2048 * a.qt[0][i] / a.qt[c][i]) * ff;
      const int32_t cfl = (y * ((scale + 1024) >> 11) + 1024) >> 11;
      val = f.coeff[ch][base] + cfl;
    }
    a.out[((size_t)c * nblk + o) * 64 + i] = (int16_t)val;
  }
}

inline dim3 Grid2(uint32_t w, uint32_t h) { return dim3((w + 31) / 32, (h + 7) / 8); }
const dim3 kBlock2(32, 8);

}  // namespace

void LaunchIntToFloat(const int32_t* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t w, uint32_t h, float factor, void* stream, uint32_t float_bits,
                      uint32_t float_exp_bits) {
  hipLaunchKernelGGL(IntToFloatKernel, Grid2(w, h), kBlock2, 0, (hipStream_t)stream, src, src_stride, dst, dst_stride, w, h, factor, float_bits, float_exp_bits);
}
void LaunchXybModToFloat(const int32_t* cy, const int32_t* cx, const int32_t* cb, uint32_t src_stride, float* const dst[3], uint32_t dst_stride, uint32_t w, uint32_t h,
                         const float fac[3], void* stream) {
  hipLaunchKernelGGL(XybModToFloatKernel, Grid2(w, h), kBlock2, 0, (hipStream_t)stream, cy, cx, cb, src_stride, dst[0], dst[1], dst[2], dst_stride, w, h, fac[0], fac[1], fac[2]);
}
void LaunchSplines(float* const p[3], uint32_t stride, uint32_t w, uint32_t h, const SplineSegmentDev* segs, const uint32_t* row_start, const uint32_t* indices, void* stream) {
  hipLaunchKernelGGL(SplineKernel, dim3((w + 255) / 256, h), dim3(256), 0, (hipStream_t)stream, p[0], p[1], p[2], stride, w, h, segs, row_start, indices);
}
void LaunchUpsamplePlane(const float* src, uint32_t src_stride, uint32_t w, uint32_t h, float* dst, uint32_t dst_stride, uint32_t ow, uint32_t oh, uint32_t up,
                         const float* weights, void* stream) {
  hipLaunchKernelGGL(UpsamplePlaneKernel, Grid2(ow, oh), kBlock2, 0, (hipStream_t)stream, src, src_stride, (int)w, (int)h, dst, dst_stride, (int)ow, (int)oh, (int)up, weights);
}
void LaunchNoise(const NoiseArgs& a, void* stream) {
  const uint32_t gx = (a.w + a.group_dim - 1) / a.group_dim, gy = (a.h + a.group_dim - 1) / a.group_dim;
  hipLaunchKernelGGL(NoiseRandomKernel, dim3(gx, gy), dim3(64), 0, (hipStream_t)stream, a.noise[0], a.noise[1], a.noise[2], a.noise_stride, a.w, a.h, a.group_dim,
                     a.visible_frame_index, a.nonvisible_frame_index);
  hipLaunchKernelGGL(NoiseAddKernel, Grid2(a.w, a.h), kBlock2, 0, (hipStream_t)stream, a);
}
void LaunchColor(const ColorArgs& a, void* stream) { hipLaunchKernelGGL(ColorKernel, Grid2(a.w, a.h), kBlock2, 0, (hipStream_t)stream, a); }
void LaunchWrite(const WriteArgs& a, void* stream) { hipLaunchKernelGGL(WriteKernel, Grid2(a.img_w, a.img_h), kBlock2, 0, (hipStream_t)stream, a); }
void LaunchEcPlanesOut(const EcPlanesOutArgs& a, void* stream) {
  if (!a.num_planes || !a.w || !a.h || a.num_planes > 65535) return;      // (the host caps the requests at 4096: OutputSpec::planes)
  hipLaunchKernelGGL(EcPlanesOutKernel, dim3((a.w + 255) / 256, std::min<uint32_t>(a.h, 65535u), a.num_planes), dim3(256), 0, (hipStream_t)stream, a);
}
void LaunchEcIntToFloat(const EcFrameArgs& a, void* stream) {
  if (!a.num_extra) return;
  dim3 g = Grid2(a.w, a.h); g.z = a.num_extra;
  hipLaunchKernelGGL(EcIntToFloatKernel, g, kBlock2, 0, (hipStream_t)stream, a);
}
void LaunchEcUpsample(const EcFrameArgs& a, void* stream) {
  if (!a.num_extra) return;
  dim3 g = Grid2(a.ow, a.oh); g.z = a.num_extra;
  hipLaunchKernelGGL(EcUpsampleKernel, g, kBlock2, 0, (hipStream_t)stream, a);
}
void LaunchPatches(const PatchFrameArgs& a, const EcChanDev* table, const PatchEntryDev* entries, const PatchEcDev* pec, const uint32_t* tile_start, const uint32_t* tile_list,
                   void* stream) {
  const uint32_t tiles_x = (a.w + 31) / 32, tiles_y = (a.h + 31) / 32;
  hipLaunchKernelGGL(PatchKernel, dim3(tiles_x * tiles_y), dim3(256), 0, (hipStream_t)stream, a, table, entries, pec, tile_start, tile_list, tiles_x);
}
void LaunchBlend(const BlendArgs& a, const EcChanDev* table, void* stream) {
  hipLaunchKernelGGL(BlendColorKernel, Grid2(a.img_w, a.img_h), kBlock2, 0, (hipStream_t)stream, a, table);
  if (!a.num_extra) return;
  dim3 g = Grid2(a.img_w, a.img_h); g.z = a.num_extra;
  hipLaunchKernelGGL(BlendEcKernel, g, kBlock2, 0, (hipStream_t)stream, a, table);
}
void LaunchSpot(float* const p[3], uint32_t stride, const EcChanDev* table, uint32_t num_extra, uint32_t use_canvas, uint32_t w, uint32_t h, void* stream) {
  hipLaunchKernelGGL(SpotKernel, Grid2(w, h), kBlock2, 0, (hipStream_t)stream, p[0], p[1], p[2], stride, table, num_extra, use_canvas, w, h);
}
void LaunchJpegCoefficients(const FrameDev* frames, int fidx, const JpegCoefArgs& a, uint32_t bw, uint32_t bh, void* stream) {
  const uint32_t n = bw * bh * 64;
  hipLaunchKernelGGL(JpegCoefKernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, frames, fidx, a);
}
void LaunchCopyPlane(const float* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t w, uint32_t h, void* stream) {
  hipLaunchKernelGGL(CopyPlaneKernel, Grid2(w, h), kBlock2, 0, (hipStream_t)stream, src, src_stride, dst, dst_stride, w, h);
}

template <int NC> static void LaunchResizeNc(const ResizeArgs* table, const ResizeGroup& g, hipStream_t st) {
  const dim3 block(64, 4);
  const uint32_t gx = (g.max_out_w + 63) / 64;
  hipLaunchKernelGGL((ResizeKernel<NC, false>), dim3(gx, std::min<uint32_t>((g.max_in_h + 3) / 4, 65535u), g.count), block, 0, st, table + g.first);
  hipLaunchKernelGGL((ResizeKernel<NC, true>), dim3(gx, (g.max_out_h + 3) / 4, g.count), block, 0, st, table + g.first);
}
template <int NC> static void LaunchResizeU8Nc(const ResizeArgs* table, const ResizeGroup& g, hipStream_t st) {
  const dim3 block(64, 4);
  const uint32_t gx = (g.max_out_w + 63) / 64;
  hipLaunchKernelGGL((ResizeU8Kernel<NC, false>), dim3(gx, std::min<uint32_t>((g.max_in_h + 3) / 4, 65535u), g.count), block, 0, st, table + g.first);
  hipLaunchKernelGGL((ResizeU8Kernel<NC, true>), dim3(gx, (g.max_out_h + 3) / 4, g.count), block, 0, st, table + g.first);
}
void LaunchResizeGroup(const ResizeArgs* table, const ResizeGroup& g, void* stream) {
  if (!g.count || g.count > kResizeGroupMax || !g.max_out_w || !g.max_in_h || !g.max_out_h) return;
  if (g.u8) {      // (a group is of one arithmetic: Batch::BuildResizeTable)
    switch (g.slots) {
      case 1: LaunchResizeU8Nc<1>(table, g, (hipStream_t)stream); break;
      case 2: LaunchResizeU8Nc<2>(table, g, (hipStream_t)stream); break;
      case 3: LaunchResizeU8Nc<3>(table, g, (hipStream_t)stream); break;
      default: LaunchResizeU8Nc<4>(table, g, (hipStream_t)stream); break;
    }
    return;
  }
  switch (g.slots) {
    case 1: LaunchResizeNc<1>(table, g, (hipStream_t)stream); break;
    case 2: LaunchResizeNc<2>(table, g, (hipStream_t)stream); break;
    case 3: LaunchResizeNc<3>(table, g, (hipStream_t)stream); break;
    default: LaunchResizeNc<4>(table, g, (hipStream_t)stream); break;
  }
}
void LaunchChromaUpsample(const float* src, uint32_t src_stride, float* dst, uint32_t dst_stride, uint32_t hs, uint32_t vs, uint32_t out_w, uint32_t out_h, void* stream) {
  ChromaUpArgs a{src, dst, src_stride, dst_stride, hs, vs, out_w, out_h};
  hipLaunchKernelGGL(ChromaUpsampleKernel, Grid2(out_w, out_h), kBlock2, 0, (hipStream_t)stream, a);
}

}  // namespace jxlhip
