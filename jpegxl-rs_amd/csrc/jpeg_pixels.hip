// jxl-hip: the samples libjpeg gives for the original file of a JPEG transcode (decoder.cc Batch::DecodeJpegPixels) — integer arithmetic throughout, no part of the
// float VarDCT pipeline.  Input: the int16 coefficient planes JpegCoefKernel leaves in device memory (natural order, MCU-padded block grids) and the JPEG
// quantisation tables.  Output: the caller's pixels through the write stage (pixel_ops.h StorePixel).
//   JpegIdctKernel       dequantisation and libjpeg's jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2) -> u8 component planes of the padded grids
//   JpegColorOutKernel   "fancy" chroma upsampling (jdsample.c h2v1 / h2v2 triangle filters; plain replication for planes at most two samples wide), fixed-point
//                        YCbCr -> RGB (jdcolor.c), sample k enters the write stage as (float)k x (1 / 255)
// Every sum that a damaged stream can drive out of range is formed in uint32_t: it wraps, nothing is undefined; the samples of such a stream mean nothing, but every
// address is derived from the host's table alone.
#include "kernels.h"
#include "pixel_ops.h"
#include <hip/hip_runtime.h>

namespace jxlhip {

namespace {

constexpr uint32_t kIdctBlocksPerWave = 8, kIdctWaves = 4;
constexpr uint32_t kIdctBlockStride = 72;      // dwords from one block's workspace to the next: 64 + 8, so that the eight blocks' column stores of pass 1 fall on different banks

template <int N> __device__ __forceinline__ int32_t Descale(uint32_t x) { return (int32_t)(x + (1u << (N - 1))) >> N; }

// jidctint.c's 1-D transform (the even part from i0, i2, i4, i6, the odd part from i1, i3, i5, i7), results descaled by N bits
template <int N> __device__ __forceinline__ void JpegIdct1D(const uint32_t i[8], int32_t out[8]) {
  uint32_t z1 = (i[2] + i[6]) * 4433u;
  const uint32_t t2 = z1 - i[6] * 15137u, t3 = z1 + i[2] * 6270u;
  const uint32_t t0 = (i[0] + i[4]) << 13, t1 = (i[0] - i[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995; z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  out[0] = Descale<N>(t10 + a3); out[7] = Descale<N>(t10 - a3);
  out[1] = Descale<N>(t11 + a2); out[6] = Descale<N>(t11 - a2);
  out[2] = Descale<N>(t12 + a1); out[5] = Descale<N>(t12 - a1);
  out[3] = Descale<N>(t13 + a0); out[4] = Descale<N>(t13 - a0);
}

__device__ __forceinline__ uint32_t ClampU8(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

// A wavefront takes eight blocks, lane = (block j, k).  Pass 1: the lane owns column k of its block; pass 2: row k.
__global__ __launch_bounds__(256) void JpegIdctKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) int32_t ws[kIdctWaves][kIdctBlocksPerWave * kIdctBlockStride];
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  if (blockIdx.x * (kIdctWaves * kIdctBlocksPerWave) >= im.nblk || *f.status != 0) return;     // (uniform over the workgroup)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane >> 3, k = lane & 7;
  const uint32_t blk = (blockIdx.x * kIdctWaves + wave) * kIdctBlocksPerWave + j;
  const bool live = blk < im.nblk;
  const uint32_t c = im.ncomp == 3 ? (blk >= im.comp_first[2] ? 2u : blk >= im.comp_first[1] ? 1u : 0u) : 0u;
  const uint32_t local = blk - im.comp_first[c], gw = im.grid_w[c], bx = local % gw, by = local / gw;
  int32_t* const w = ws[wave] + j * kIdctBlockStride;
  if (live) {
    if (k == 0) {
      // the entropy stages of a damaged stream may have placed other transforms than DCT8: the frame fails through its status word (its samples are not delivered)
      const uint32_t sx = c ? bx << im.hs : bx, sy = c ? by << im.vs : by;
      if (sx < f.bw && sy < f.bh && (f.blk_info[(size_t)sy * f.bw + sx] & 31u) != 0) atomicOr(f.status, (uint32_t)kErrVarblock);
    }
    const int16_t* __restrict__ cf = im.coef + (size_t)blk * 64 + k;
    const int32_t* __restrict__ q = im.qt[c] + k;
    uint32_t in[8];
#pragma unroll
    for (int r = 0; r < 8; r++) in[r] = (uint32_t)(int32_t)cf[r * 8] * (uint32_t)q[r * 8];
    int32_t col[8];
    JpegIdct1D<11>(in, col);
#pragma unroll
    for (int r = 0; r < 8; r++) w[r * 8 + k] = col[r];
  }
  __syncthreads();
  if (!live) return;
  uint32_t in[8];
  const int4 lo = *(const int4*)(w + k * 8), hi = *(const int4*)(w + k * 8 + 4);
  in[0] = (uint32_t)lo.x; in[1] = (uint32_t)lo.y; in[2] = (uint32_t)lo.z; in[3] = (uint32_t)lo.w;
  in[4] = (uint32_t)hi.x; in[5] = (uint32_t)hi.y; in[6] = (uint32_t)hi.z; in[7] = (uint32_t)hi.w;
  int32_t row[8];
  JpegIdct1D<18>(in, row);
  uint2 px;
  px.x = ClampU8(row[0] + 128) | ClampU8(row[1] + 128) << 8 | ClampU8(row[2] + 128) << 16 | ClampU8(row[3] + 128) << 24;
  px.y = ClampU8(row[4] + 128) | ClampU8(row[5] + 128) << 8 | ClampU8(row[6] + 128) << 16 | ClampU8(row[7] + 128) << 24;
  *(uint2*)(im.plane[c] + ((size_t)by * 8 + k) * ((size_t)gw * 8) + (size_t)bx * 8) = px;
}

// The two chroma samples of output pixels (2 sx, 2 sx + 1) of row y from plane s (jdsample.c): cw x ch is the component's real extent, the padded part of the grid is
// never a tap and a tap beyond an edge is the edge sample — which gives libjpeg's special first and last columns, (4 c + 8) >> 4 and (4 c + 7) >> 4, s[0] and s[cw - 1]
__device__ __forceinline__ void ChromaPair(const uint8_t* __restrict__ s, uint32_t pitch, uint32_t vs, uint32_t cw, uint32_t ch, uint32_t sx, uint32_t y, int32_t out[2]) {
  const uint32_t sy = y >> vs;
  const uint8_t* __restrict__ r0 = s + (size_t)sy * pitch;
  if (cw <= 2) { out[0] = out[1] = r0[sx]; return; }      // (libjpeg does not interpolate such a plane at all: h2v1_upsample / h2v2_upsample)
  const uint32_t xl = sx ? sx - 1 : 0, xr = min(sx + 1, cw - 1);
  if (!vs) {
    const int32_t m = 3 * r0[sx];
    out[0] = (m + r0[xl] + 1) >> 2; out[1] = (m + r0[xr] + 2) >> 2;
    return;
  }
  const uint32_t nb = (y & 1) ? min(sy + 1, ch - 1) : (sy ? sy - 1 : 0);
  const uint8_t* __restrict__ r1 = s + (size_t)nb * pitch;
  const int32_t cm = 3 * r0[sx] + r1[sx], cl = 3 * r0[xl] + r1[xl], cr = 3 * r0[xr] + r1[xr];
  out[0] = (3 * cm + cl + 8) >> 4; out[1] = (3 * cm + cr + 7) >> 4;
}

// A thread takes the output pixels (2 t, 2 t + 1) of a row: they share their chroma position in the subsampled modes.
__global__ __launch_bounds__(256) void JpegColorOutKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  const uint32_t t = blockIdx.x * 32 + threadIdx.x, x0 = t * 2, y = blockIdx.y * 8 + threadIdx.y;
  if (x0 >= im.width || y >= im.height || *f.status != 0) return;
  const uint32_t npix = x0 + 1 < im.width ? 2 : 1;
  const float k255 = 1.0f / 255;
  const uint8_t* __restrict__ yrow = im.plane[0] + (size_t)y * ((size_t)im.grid_w[0] * 8);
  const int32_t lum[2] = {yrow[x0], yrow[x0 + 1]};      // (x0 + 1 is inside the padded grid: its width is a multiple of 8)
  if (im.ncomp == 1) {
    for (uint32_t i = 0; i < npix; i++) { const float v = (float)lum[i] * k255; StorePixel(f.od, (int)im.width, (int)im.height, (int)(x0 + i), (int)y, v, v, v, 1.0f); }
    return;
  }
  int32_t cb[2], cr[2];
  if (!im.hs) {
    const size_t o = (size_t)y * ((size_t)im.grid_w[1] * 8) + x0;
    cb[0] = im.plane[1][o]; cb[1] = im.plane[1][o + 1]; cr[0] = im.plane[2][o]; cr[1] = im.plane[2][o + 1];
  } else {
    const uint32_t cw = (im.width + 1) >> 1, ch = (im.height + (1u << im.vs) - 1) >> im.vs, pitch = im.grid_w[1] * 8;
    ChromaPair(im.plane[1], pitch, im.vs, cw, ch, t, y, cb);
    ChromaPair(im.plane[2], pitch, im.vs, cw, ch, t, y, cr);
  }
  for (uint32_t i = 0; i < npix; i++) {
    const int32_t u = cb[i] - 128, v = cr[i] - 128;
    const int32_t r = min(max(lum[i] + ((91881 * v + 32768) >> 16), 0), 255);
    const int32_t g = min(max(lum[i] + ((-22554 * u - 46802 * v + 32768) >> 16), 0), 255);
    const int32_t b = min(max(lum[i] + ((116130 * u + 32768) >> 16), 0), 255);
    StorePixel(f.od, (int)im.width, (int)im.height, (int)(x0 + i), (int)y, (float)r * k255, (float)g * k255, (float)b * k255, 1.0f);
  }
}

}  // namespace

void LaunchJpegPixelGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream) {
  if (!g.count || g.count > kJpegPixelGroupMax || !g.max_nblk || !g.max_w || !g.max_h) return;
  const uint32_t per_wg = kIdctWaves * kIdctBlocksPerWave;
  hipLaunchKernelGGL(JpegIdctKernel, dim3((g.max_nblk + per_wg - 1) / per_wg, 1, g.count), dim3(256), 0, (hipStream_t)stream, frames, table + g.first);
  hipLaunchKernelGGL(JpegColorOutKernel, dim3((g.max_w + 63) / 64, (g.max_h + 7) / 8, g.count), dim3(32, 8), 0, (hipStream_t)stream, frames, table + g.first);
}

}  // namespace jxlhip
