// jxl-hip: the per-sample tail of the decoder — upsampling, colour transform, transfer function, sample conversion and the write into the caller's
// layout (libjxl's stage_{upsampling,chroma_upsampling,xyb,ycbcr,from_linear,write}.cc).  Device code only, one definition per formula: the fused tile
// kernels of single-frame images (kernels.hip) and the host-planned frame tail (kernels_features.hip) both call these, so what the two paths write can
// differ only in the samples they are given.  Arithmetic and operation order are those of oracle/render.h; the library is built with -ffp-contract=off,
// so every fmaf below is one that libjxl has and no other product is fused.
#pragma once
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace jxlhip {

// mirror at the border, as every stage of libjxl's pipeline mirrors its own input
__device__ __forceinline__ int MirrorD(int x, int size) {
  while (x < 0 || x >= size) x = x < 0 ? -x - 1 : 2 * size - 1 - x;
  return x;
}

// ---- transfer functions (stage_from_linear.cc) ---------------------------------------------------------------------------------------------------
// base/fast_math-inl.h FastLog2f / FastPow2f / FastPowf
__device__ __forceinline__ float FastPowf(float base, float exponent) {
  const int32_t x_bits = __float_as_int(base);
  const int32_t exp_shifted = (x_bits - 0x3f2aaaab) >> 23;
  const float t = __int_as_float(x_bits - (int32_t)((uint32_t)exp_shifted << 23)) - 1.0f;
  float yp = fmaf(7.4245873327820566E-01f, t, 1.4287160470083755E+00f); yp = fmaf(yp, t, -1.8503833400518310E-06f);
  float yq = fmaf(1.7409343003366853E-01f, t, 1.0096718572241148E+00f); yq = fmaf(yq, t, 9.9032814277590719E-01f);
  const float x = (yp / yq + (float)exp_shifted) * exponent;
  const float floorx = floorf(x);
  const float exp = __int_as_float((int32_t)((uint32_t)((int32_t)floorx + 127) << 23));
  const float frac = x - floorx;
  float num = frac + 1.01749063e+01f;
  num = fmaf(num, frac, 4.88687798e+01f);
  num = fmaf(num, frac, 9.85506591e+01f);
  num = num * exp;
  float den = fmaf(frac, 2.10242958e-01f, -2.22328856e-02f);
  den = fmaf(den, frac, -1.94414990e+01f);
  den = fmaf(den, frac, 9.85506633e+01f);
  return num / den;
}
// cms/transfer_functions-inl.h TF_SRGB
__device__ __forceinline__ float LinearToSrgb(float v) {
  const float x = fabsf(v);
  const float lin = x * 12.92f;
  const float s = sqrtf(x);
  float yp = 7.352629620e-1f, yq = 2.424867759e-2f;
  yp = fmaf(yp, s, 1.474205315f); yq = fmaf(yq, s, 9.258482155e-1f);
  yp = fmaf(yp, s, 3.903842876e-1f); yq = fmaf(yq, s, 1.340816930f);
  yp = fmaf(yp, s, 5.287254571e-3f); yq = fmaf(yq, s, 3.036675394e-1f);
  yp = fmaf(yp, s, -5.135152395e-4f); yq = fmaf(yq, s, 1.004519624e-2f);
  const float poly = yp / yq;
  return copysignf(x > 0.0031308f ? poly : lin, v);
}
__device__ __forceinline__ float GammaFromLinear(float v, float inverse_gamma) { return v <= 1e-5f ? 0.0f : FastPowf(v, inverse_gamma); }   // OpGamma
__device__ __forceinline__ float Rec709FromLinear(float v) { return v <= 0.018f ? 4.5f * v : fmaf(1.099f, FastPowf(v, 0.45f), -0.099f); }   // TF_709

// Linear RGB -> the output's transfer function.  mode: FrameDev::color_mode's values (0 sRGB, 1 linear, 4 gamma, 5 Rec.709, 6 PQ, 7 HLG — behind the inverse OOTF,
// which mixes the three channels); P: FrameDev or ColorArgs (inverse_gamma, hdr_par as decoder.cc FillColor sets them).  The triple goes in and comes back by
// value: by reference, OutputKernel took two registers more.
template <typename P> __device__ __forceinline__ float3 TransferFromLinear(const P& p, uint32_t mode, float r, float g, float b) {
  if (mode == 0) { r = LinearToSrgb(r); g = LinearToSrgb(g); b = LinearToSrgb(b); }
  else if (mode == 4) { r = GammaFromLinear(r, p.inverse_gamma); g = GammaFromLinear(g, p.inverse_gamma); b = GammaFromLinear(b, p.inverse_gamma); }
  else if (mode == 5) { r = Rec709FromLinear(r); g = Rec709FromLinear(g); b = Rec709FromLinear(b); }
  else if (mode == 6) { r = PqFromLinear(r, p.hdr_par[0]); g = PqFromLinear(g, p.hdr_par[0]); b = PqFromLinear(b, p.hdr_par[0]); }
  else if (mode == 7) {
    HlgInverseOotf(p.hdr_par, r, g, b, [](float x, float e) { return FastPowf(x, e); });
    r = HlgFromLinear(r); g = HlgFromLinear(g); b = HlgFromLinear(b);
  }
  return make_float3(r, g, b);
}

// ---- inverse transfer functions: encoded samples -> linear light (1.0 = the image's intensity target), for images that are not XYB on their way to a requested
// output encoding (ColorKernel).  The textbook definitions in float32 with the device's powf / expf — no fast approximations, nothing here is held bit for bit against
// libjxl.  Negative inputs as the forward functions above treat them: odd extension; the power law gives 0 at or below GammaFromLinear's threshold.
__device__ __forceinline__ float SrgbToLinear(float v) {            // IEC 61966-2-1
  const float x = fabsf(v);
  return copysignf(x <= 0.04045f ? x * (1.0f / 12.92f) : powf((x + 0.055f) * (1.0f / 1.055f), 2.4f), v);
}
__device__ __forceinline__ float GammaToLinear(float v, float gamma) { return v <= 1e-5f ? 0.0f : powf(v, gamma); }      // gamma: 1 / the encoding exponent
__device__ __forceinline__ float Rec709ToLinear(float v) { return v < 0.081f ? v * (1.0f / 4.5f) : powf((v + 0.099f) * (1.0f / 1.099f), 1.0f / 0.45f); }
// SMPTE ST 2084 EOTF, Y = (max(p - c1, 0) / (c2 - c3 p))^(1 / m1) with p = E^(1 / m2); scale = 10000 / intensity target.  In double, as HlgFromLinear is: towards code
// 1.0 the denominator is the difference of two numbers a hundred times its size and the power 1 / m1 = 6.3 multiplies what that loses — in float32, 5e-5 of the value
// (measured: 6e-4 on a linear light of 10, code 1.0 of a 1000-nit image)
__device__ __forceinline__ float PqToLinear(float v, float scale) {
  const double m1 = 2610.0 / 16384, m2 = 2523.0 / 4096 * 128, c1 = 3424.0 / 4096, c2 = 2413.0 / 4096 * 32, c3 = 2392.0 / 4096 * 32;
  const double p = pow(fabs((double)v), 1.0 / m2);
  return copysignf((float)(pow(fmax(p - c1, 0.0) / (c2 - c3 * p), 1.0 / m1) * (double)scale), v);
}
// BT.2100 HLG inverse OETF: scene light, 1.0 at signal 1.0
__device__ __forceinline__ float HlgToLinear(float v) {
  const float kA = 0.17883277f, kB = 1 - 4 * kA, kC = 0.5599107295f;
  const float e = fabsf(v);
  return copysignf(e <= 0.5f ? e * e * (1.0f / 3) : (expf((e - kC) * (1.0f / kA)) + kB) * (1.0f / 12), v);
}
// BT.2100 HLG OOTF: display = scene x Y_s^(gamma - 1); par = {gamma - 1, apply?, luminances of the source's primaries} (the inverse of HlgInverseOotf, skipped in its band)
__device__ __forceinline__ void HlgOotf(const float* par, float& r, float& g, float& b) {
  if (par[1] == 0.0f) return;
  const float luminance = fmaf(par[2], r, fmaf(par[3], g, par[4] * b));
  const float ratio = fminf(powf(fmaxf(luminance, 0.0f), par[0]), 1e9f);
  r *= ratio; g *= ratio; b *= ratio;
}
// Encoded samples of encoding `kind` (FrameDev::color_mode's values: 0 sRGB, 1 linear, 4 gamma, 5 Rec.709, 6 PQ, 7 HLG) -> linear light.  kind is the same for the whole
// launch (a kernel argument): one scalar branch, not a select over the functions
__device__ __forceinline__ float3 TransferToLinear(const float* par, uint32_t kind, float r, float g, float b) {
  switch (kind) {
    case 0: r = SrgbToLinear(r); g = SrgbToLinear(g); b = SrgbToLinear(b); break;
    case 4: r = GammaToLinear(r, par[0]); g = GammaToLinear(g, par[0]); b = GammaToLinear(b, par[0]); break;
    case 5: r = Rec709ToLinear(r); g = Rec709ToLinear(g); b = Rec709ToLinear(b); break;
    case 6: r = PqToLinear(r, par[0]); g = PqToLinear(g, par[0]); b = PqToLinear(b, par[0]); break;
    case 7: r = HlgToLinear(r); g = HlgToLinear(g); b = HlgToLinear(b); HlgOotf(par, r, g, b); break;
    default: break;
  }
  return make_float3(r, g, b);
}

// ---- colour transforms ----------------------------------------------------------------------------------------------------------------------------
// stage_xyb.cc: XYB -> linear RGB (bias, cube, 3x3 matrix).  P: FrameDev or ColorArgs (opsin_inv, neg_bias, neg_bias_cbrt as decoder.cc FillColor sets them)
template <typename P> __device__ __forceinline__ void XybToLinear(const P& p, float X, float Y, float B, float& r, float& g, float& b) {
  const float gr = (Y + X) - p.neg_bias_cbrt[0];
  const float gg = (Y - X) - p.neg_bias_cbrt[1];
  const float gb = B - p.neg_bias_cbrt[2];
  const float mr = fmaf(gr * gr, gr, p.neg_bias[0]);
  const float mg = fmaf(gg * gg, gg, p.neg_bias[1]);
  const float mb = fmaf(gb * gb, gb, p.neg_bias[2]);
  r = fmaf(p.opsin_inv[2], mb, fmaf(p.opsin_inv[1], mg, p.opsin_inv[0] * mr));
  g = fmaf(p.opsin_inv[5], mb, fmaf(p.opsin_inv[4], mg, p.opsin_inv[3] * mr));
  b = fmaf(p.opsin_inv[8], mb, fmaf(p.opsin_inv[7], mg, p.opsin_inv[6] * mr));
}
// stage_ycbcr.cc: planes in codestream order Cb, Y, Cr -> RGB
__device__ __forceinline__ void YcbcrToRgb(float Cb, float Y, float Cr, float& r, float& g, float& b) {
  const float c128 = 128.0f / 255, crcr = 1.402f, cbcb = 1.772f, cgcb = -0.114f * cbcb / 0.587f, cgcr = -0.299f * crcr / 0.587f;
  const float yb = Y + c128;
  r = fmaf(crcr, Cr, yb);
  g = fmaf(cgcr, Cr, fmaf(cgcb, Cb, yb));
  b = fmaf(cbcb, Cb, yb);
}

// ---- write stage (stage_write.cc) -----------------------------------------------------------------------------------------------------------------
// binary32 -> binary16 bits, round to nearest even
__device__ __forceinline__ uint16_t FloatToHalfBits(float fv) {
  const uint32_t x = __float_as_uint(fv);
  const uint32_t sign = (x >> 16) & 0x8000;
  const int32_t exp = (int32_t)((x >> 23) & 0xFF) - 127 + 15;
  uint32_t mant = x & 0x7FFFFF;
  const uint32_t inf = sign | 0x7C00;
  if (((x >> 23) & 0xFF) == 0xFF) return (uint16_t)(inf | (mant ? 0x200 : 0));
  if (exp >= 31) return (uint16_t)inf;
  if (exp <= 0) {
    if (exp < -10) return (uint16_t)sign;
    mant |= 0x800000;
    const int shift = 14 - exp;
    uint32_t m = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (m & 1))) m++;
    return (uint16_t)(sign | m);
  }
  const uint32_t m = mant >> 13, rem = mant & 0x1FFF;
  uint32_t r = (uint32_t)(exp << 10) | m;
  if (rem > 0x1000 || (rem == 0x1000 && (m & 1))) r++;
  return (uint16_t)(sign | r);
}

__device__ __forceinline__ void StoreSample(const OutputDesc& o, uint8_t* p, float v) {
  if (o.out_type == 0) {
    p[0] = (uint8_t)__float2int_rn(fminf(1.0f, fmaxf(0.0f, v)) * o.out_int_mul);
  } else if (o.out_type == 1) {
    const uint32_t u = (uint32_t)__float2int_rn(fminf(1.0f, fmaxf(0.0f, v)) * o.out_int_mul);
    if (o.out_big_endian) { p[0] = (uint8_t)(u >> 8); p[1] = (uint8_t)u; } else { p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); }
  } else if (o.out_type == 2) {
    const uint32_t u = __float_as_uint(v);
    if (o.out_big_endian) { p[0] = (uint8_t)(u >> 24); p[1] = (uint8_t)(u >> 16); p[2] = (uint8_t)(u >> 8); p[3] = (uint8_t)u; }
    else { p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); p[2] = (uint8_t)(u >> 16); p[3] = (uint8_t)(u >> 24); }
  } else {
    const uint32_t u = FloatToHalfBits(v);
    if (o.out_big_endian) { p[0] = (uint8_t)(u >> 8); p[1] = (uint8_t)u; } else { p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); }
  }
}

// Position of sample (x, y) of the w x h image in the output buffer: the header's orientation (1..8, EXIF numbering as in
// codestream_header.rs JxlOrientation) is applied by the write stage — 2 flip-h, 3 rotate 180, 4 flip-v, 5 transpose,
// 6 rotate 90 cw, 7 anti-transpose, 8 rotate 90 ccw; out_stride already refers to the oriented width.  Interleaved: the pixel's first sample;
// planar: its sample in plane 0, a row holding one sample per pixel.
__device__ __forceinline__ uint8_t* OutPixelPtr(const OutputDesc& o, int w, int h, int x, int y, uint32_t bps) {
  int ox = x, oy = y;
  switch (o.out_orient) {
    case 2: ox = w - 1 - x; break;
    case 3: ox = w - 1 - x; oy = h - 1 - y; break;
    case 4: oy = h - 1 - y; break;
    case 5: ox = y; oy = x; break;
    case 6: ox = h - 1 - y; oy = x; break;
    case 7: ox = h - 1 - y; oy = w - 1 - x; break;
    case 8: ox = y; oy = w - 1 - x; break;
    default: break;
  }
  return o.out + (size_t)oy * o.out_stride + (size_t)ox * (o.planar ? bps : o.out_channels * bps);
}

// the sample of channel slot c as it is stored: untouched, or (float output, OutputSpec::affine) v x scale[c] + bias[c] in one rounding
__device__ __forceinline__ float SlotValue(const OutputDesc& o, int c, float v) { return o.affine ? fmaf(v, o.scale[c], o.bias[c]) : v; }

// pixel (x, y) of the w x h image -> 1, 2, 3 or 4 samples, interleaved or one per plane (o.planar and o.affine are the same for the whole launch's image: uniform branches)
__device__ __forceinline__ void StorePixel(const OutputDesc& o, int w, int h, int x, int y, float r, float g, float b, float a) {
  const uint32_t bps = o.out_type == 0 ? 1 : o.out_type == 2 ? 4 : 2;
  uint8_t* p = OutPixelPtr(o, w, h, x, y, bps);
  const uint32_t nc = o.out_channels;
  const size_t step = o.planar ? (size_t)o.plane_stride : (size_t)bps;   // from one slot's sample to the next one's
  if (nc <= 2) {
    StoreSample(o, p, SlotValue(o, 0, o.is_gray ? r : g));  // gray images carry the same value in all channels; otherwise take G
    if (nc == 2) StoreSample(o, p + step, SlotValue(o, 1, a));
  } else {
    StoreSample(o, p, SlotValue(o, 0, r)); StoreSample(o, p + step, SlotValue(o, 1, g)); StoreSample(o, p + 2 * step, SlotValue(o, 2, b));
    if (nc == 4) StoreSample(o, p + 3 * step, SlotValue(o, 3, a));
  }
}

// ---- upsampling -----------------------------------------------------------------------------------------------------------------------------------
// Non-separable 2x / 4x / 8x upsampling (stage_upsampling.cc; same definition and accumulation order as oracle/render.h UpsamplePlane): output sample (ox, oy)
// of a w x h plane, 25 taps, result clamped to the window's range.  fetch(x, y): the plane's sample; weights: 15 / 55 / 210 coefficients of the symmetric
// (5N x 5N) kernel matrix, N = up / 2.
template <typename Fetch> __device__ __forceinline__ float UpsampleSample(Fetch fetch, int w, int h, int ox, int oy, int up, const float* __restrict__ weights) {
  const int N = up / 2;
  const int x = ox / up, sx = ox % up, y = oy / up, sy = oy % up;
  const int ky = sy < N ? sy : up - 1 - sy, kx = sx < N ? sx : up - 1 - sx;
  const bool fy = sy >= N, fx = sx >= N;
  float sum = 0.0f, mn = 0.0f, mx = 0.0f;
  for (int iy = 0; iy < 5; iy++) {
    const int yy = MirrorD(y + iy - 2, h);
    const int mi = 5 * ky + (fy ? 4 - iy : iy);
    for (int ix = 0; ix < 5; ix++) {
      const int xx = MirrorD(x + ix - 2, w);
      const float v = fetch(xx, yy);
      const int mj = 5 * kx + (fx ? 4 - ix : ix);
      const int lo = mi < mj ? mi : mj, hi = mi < mj ? mj : mi;
      const float k = weights[5 * N * lo - lo * (lo - 1) / 2 + hi - lo];
      sum = fmaf(k, v, sum);
      if (iy == 0 && ix == 0) { mn = v; mx = v; } else { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    }
  }
  return sum < mn ? mn : (sum > mx ? mx : sum);
}

// Sample (x, y) of a chroma-subsampled channel at full resolution (stage_chroma_upsampling.cc: horizontal, then vertical, each with the (1/4, 3/4) kernel —
// out[2x] = 0.25 in[x-1] + 0.75 in[x], out[2x+1] = 0.25 in[x+1] + 0.75 in[x] —, neighbours clamped at the channel's own edges; the vertical step works on
// horizontally upsampled rows, exactly as two stages would).  `plane` holds the channel packed top-left with row pitch `stride`; width x height is the size of
// the FULL grid that (x, y) addresses: pixels for the frame's planes, LF samples for the 1:8 decode.
__device__ __forceinline__ float SubsampledSample(const float* __restrict__ plane, uint32_t stride, uint32_t hs, uint32_t vs, uint32_t width, uint32_t height, uint32_t x, uint32_t y) {
  if (!(hs | vs)) return plane[(size_t)y * stride + x];
  const uint32_t cw = (width + (1u << hs) - 1) >> hs, ch = (height + (1u << vs) - 1) >> vs;
  const uint32_t sx = x >> hs, sy = y >> vs;
  auto hval = [&](uint32_t row) -> float {
    const float* in = plane + (size_t)row * stride;
    if (!hs) return in[x];
    const float mid = in[sx] * 0.75f;
    const uint32_t nb = (x & 1) ? min(sx + 1, cw - 1) : (sx ? sx - 1 : 0);
    return fmaf(0.25f, in[nb], mid);
  };
  if (!vs) return hval(sy);
  const float mid = hval(sy) * 0.75f;
  const uint32_t nb = (y & 1) ? min(sy + 1, ch - 1) : (sy ? sy - 1 : 0);
  return fmaf(0.25f, hval(nb), mid);
}

// ---- integer chroma from luma of a JPEG transcode (dec_group.cc, jpeg branch; the formula of JpegCoefKernel) -------------------------------------------------
// What a 4:4:4 chroma coefficient takes from the quantised luma coefficient y at the same place: fac is the tile's ytox / ytob, ratio the host's division
// 2048 x qt[0][i] / qt[c][i].  JpegCflFactor: fac * 2048 / 84, C++ division (truncates toward zero).  The sums a damaged stream can drive out of range are
// formed in uint32_t: they wrap, nothing is undefined.  JpegIdctPlanesKernel and JpegGatherKernel both call these: one definition.
__device__ __forceinline__ int32_t JpegCflFactor(int32_t fac) { return fac * 2048 / 84; }
__device__ __forceinline__ int32_t JpegCflTerm(int32_t y, int32_t ratio, int32_t ff) {
  const int32_t scale = (int32_t)((uint32_t)ratio * (uint32_t)ff);
  return (int32_t)((uint32_t)y * (uint32_t)((int32_t)((uint32_t)scale + 1024u) >> 11) + 1024u) >> 11;
}

}  // namespace jxlhip
