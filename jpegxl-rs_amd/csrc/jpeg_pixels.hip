// jxl-hip: the samples libjpeg gives for the original file of a JPEG transcode (decoder.cc Batch::DecodeJpegPixels) — integer arithmetic throughout, no part of the
// float VarDCT pipeline.  Input: the quantised coefficients where the HF stage left them (FrameDev::coeff, the DC terms in FrameDev::lfq) and the JPEG
// quantisation tables.  Output: the caller's pixels through the write stage (pixel_ops.h StorePixel).
//   JpegIdctPlanesKernel chroma from luma (4:4:4), dequantisation and libjpeg's jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2) -> u8 component planes of the
//                        padded grids; zeroes the coefficients it read
//   JpegGatherKernel     the same coefficients, read and zeroed the same way, into the int16 arena of the JPEG writer (jpeg_write.hip): batch reconstruction and
//                        reconstruction jobs of the pipeline, one launch per group of images
//   JpegColorOutKernel   "fancy" chroma upsampling (jdsample.c h2v1 / h2v2 triangle filters; plain replication for planes at most two samples wide), fixed-point
//                        YCbCr -> RGB (jdcolor.c), sample k enters the write stage as (float)k x (1 / 255)
//   JpegDcOutKernel      libjpeg's 1/8 decode where every component takes the 1 x 1 IDCT (grey, 4:4:4, 4:2:2): the picture straight from the DC terms in FrameDev::lfq —
//                        such a frame's decode ends behind the LF stage, it has no coefficient and no pixel planes
//   JpegIdctScaledKernel / JpegColorOutScaledKernel   the same two stages for libjpeg's scaled decodes (scale 1/2, 1/4, 1/8: jdmaster.c, jidctred.c): reduced IDCTs
//                        of 4 x 4, 2 x 2 or 1 x 1 samples per block (8 x 8 for 4:2:0 chroma at 1/2) -> planes of n x n samples per block -> the scaled picture
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

// jidctred.c's 1-D transforms of the reduced IDCTs, same constants' scale (CONST_BITS 13).  jpeg_idct_4x4: four results from i0, i2, i6 (even part, one bit more
// than the 8-point form: i0 << 14) and i1, i3, i5, i7; i4 is not an input.  jpeg_idct_2x2: two results from i0 (<< 15) and i1, i3, i5, i7.
template <int N> __device__ __forceinline__ void JpegIdct1D4(const uint32_t i[8], int32_t out[4]) {
  const uint32_t t0 = i[0] << 14;
  const uint32_t t2 = i[2] * 15137u + i[6] * (uint32_t)-6270;
  const uint32_t t10 = t0 + t2, t12 = t0 - t2;
  const uint32_t a0 = i[7] * (uint32_t)-1730 + i[5] * 11893u + i[3] * (uint32_t)-17799 + i[1] * 8697u;
  const uint32_t a2 = i[7] * (uint32_t)-4176 + i[5] * (uint32_t)-4926 + i[3] * 7373u + i[1] * 20995u;
  out[0] = Descale<N>(t10 + a2); out[3] = Descale<N>(t10 - a2);
  out[1] = Descale<N>(t12 + a0); out[2] = Descale<N>(t12 - a0);
}
template <int N> __device__ __forceinline__ void JpegIdct1D2(const uint32_t i[8], int32_t out[2]) {
  const uint32_t t10 = i[0] << 15;
  const uint32_t t0 = i[7] * (uint32_t)-5906 + i[5] * 6967u + i[3] * (uint32_t)-10426 + i[1] * 29692u;
  out[0] = Descale<N>(t10 + t0); out[1] = Descale<N>(t10 - t0);
}

__device__ __forceinline__ uint32_t ClampU8(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

// The integer IDCT straight from the HF stage's coefficient planes (FrameDev::coeff, FrameDev::lfq): what JpegCoefKernel (kernels_features.hip) would have
// gathered into JPEG layout is read where the HF stage left it, and zeroed, so that the coefficient set is clean for its next user as after IdctTileKernel.
//   Work: a wavefront takes eight *positions* of the image's list, lane = (position j, k).  A position of a grey or subsampled image is one block of one component
//   (components one after another, block raster order of their padded grids, as comp_first says); a position of a 4:4:4 colour image is one block position of the
//   frame, whose lane group walks Y, Cb, Cr in three steps.  Pass 1: the lane owns column k (u = k) of its block; pass 2: row k.
//   Mapping: block (sx, sy) of component c is frame block (sx << hs, sy << vs); its coefficients are the 64 dwords at g x 65536 + coef_off[o] of channel ch (Y = 1,
//   Cb in the X slot 0, Cr in the B slot 2), g the 256x256 group of that frame block; libjxl stores the transpose of JPEG's (v, u), so column u = k is the eight
//   consecutive dwords 8 k .. 8 k + 7: two 16-byte loads per lane, 256 contiguous bytes per block, eight such runs per wavefront.  The DC term is lfq at (sx, sy)
//   of the padded grid (which is o itself at 4:4:4).  qt and cfl_ratio of the table are kept in the same transposed layout and are read the same way.
//   Chroma from luma (4:4:4 only): a chroma coefficient is coeff + cfl(y) with JpegCoefKernel's formula; the lane keeps Y's quantised column in registers from
//   step 0 on, so chroma never reads Y's dwords from memory.
//   One reader per dword: a (channel, frame block) pair belongs to exactly one (position, step), and of its 64 dwords lane k alone reads — and then zeroes —
//   8 k .. 8 k + 7; DCT8 blocks of one group have disjoint slots (the placement gives every varblock its own).  So no dword is read by one lane and zeroed by
//   another: there is no order between wavefronts (or workgroups) to get wrong, in particular none between "chroma reads Y" and "Y is zeroed".  (A damaged
//   stream with larger varblocks breaks the disjointness; such a frame fails with kErrVarblock, its samples are not delivered and its planes are zeroed whole.)
//   Addresses: (sx << hs, sy << vs) is checked against the frame's grid, coef_off — written by the placement for every block of a frame that has not failed, as
//   the float IDCT kernels rely on — is in addition brought to a multiple of 64 at most 65536 - 64, so that whatever a damaged stream left there stays inside
//   the group's 65536 dwords and 16-byte aligned.
//   LDS: 72 dwords per block.  Pass 1's column stores are ds_write_b32 (banks (a / 4) % 32, one 32-lane half at a time): the half's lanes (j = 0 .. 3, k) hit
//   banks (8 j + k + 8 r) % 32, all different.  Pass 2 reads rows with ds_read_b128.
// One body for both kernels (JpegIdctBody): kScaled = false is the 8 x 8 form above with n = 8 a constant.  kScaled = true is libjpeg's scaled decode
// (JpegPixelImage::scale = 2, 4, 8) with the reduced transforms of jidctred.c: positions, lanes, the mapping of a component block to its frame block, its group and its
// 64 dwords, the two 16-byte loads of column u = k, chroma from luma with Y's column kept in registers, the DC term from lfq, kErrVarblock and the clamped coef_off are
// shared; what differs is the transform and the store.
//   Component c takes the n x n transform, n = im.n[c] (8, 4, 2, 1): components of one image differ (4:2:0: luma 8 / scale, chroma twice that), so the blocks of one
//   wavefront do — n is a per-lane value, the two barriers of a step stay outside every branch on it (steps and `walk` are uniform over the workgroup as above).
//   Every lane loads and zeroes its 8 dwords whatever n is — the columns and rows the reduced transforms ignore, all of a block's AC terms at n = 1 —: the coefficient
//   set must be clean for its next user.
//   Pass 1 (lane = column k): n = 8 all columns; n = 4 all but column 4 (jpeg_idct_4x4 never reads it); n = 2 columns 0, 1, 3, 5, 7; n = 1 lane 0 alone, which hands
//   the dequantised DC term through.  The lane writes n results, rows r = 0 .. n - 1, to w[8 r + k].  Pass 2 (lanes k < n, row k): eight workspace entries (of which
//   the transform uses those of the columns above) -> n samples, + 128, clamped, one store of n bytes at row by x n + k, column bx x n of the plane (pitch
//   grid_w x n, so every store is aligned to its own size).
//   LDS: 72 dwords per block as in the 8 x 8 form.  Pass 1's stores are ds_write_b32, banks (a / 4) % 32, one 32-lane half at a time: the half's lanes (j = 0 .. 3,
//   k) hit banks (8 j + k + 8 r) % 32 in store r — the 8 x 8 form's pattern with lanes missing (column 4 at n = 4, the even columns but 0 at n = 2, all but lane 0 at
//   n = 1) and with only the first n of its eight stores: a subset of a conflict-free pattern.  Pass 2 reads rows with two ds_read_b128 from the lanes k < n, at the
//   8 x 8 form's addresses 72 j + 8 k: again a subset.  The entries of a row that pass 1 did not write (column 4; the even columns) are read and not used.
// Regions (Batch::JpegRegion): the positions of an image are the blocks of im.reg_*[c], the block rectangle of component c that the image's decoded groups cover — the
// whole grid for an image without a region.  Position -> (c, bx, by) goes through that rectangle; everything behind it — frame block, group, loads, zeroing — is as above.
// The rectangle is whole groups: every coefficient the HF stage wrote (for the groups of FrameDev::hf_list) is read and zeroed, a skipped group's dwords were never written.
template <bool kScaled> __device__ __forceinline__ void JpegIdctBody(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table,
                                                                    int32_t (*ws)[kIdctBlocksPerWave * kIdctBlockStride]) {
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  if (blockIdx.x * (kIdctWaves * kIdctBlocksPerWave) >= im.npos || *f.status != 0) return;     // (uniform over the workgroup; a failed frame's planes are zeroed by ZeroFailedCoefKernel)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane >> 3, k = lane & 7;
  const uint32_t pos = (blockIdx.x * kIdctWaves + wave) * kIdctBlocksPerWave + j;
  const bool walk = im.ncomp == 3 && !im.hs;                 // 4:4:4: Y, Cb, Cr of one block position
  const uint32_t steps = walk ? 3u : 1u;                     // (uniform over the workgroup: the barriers below are reached by all of it)
  uint32_t c = 0, bx = 0, by = 0;
  {
    if (!walk && im.ncomp == 3) c = pos >= im.comp_first[2] ? 2u : pos >= im.comp_first[1] ? 1u : 0u;
    const uint32_t local = pos - (walk ? 0u : im.comp_first[c]), gw = max(im.reg_w[c], 1u);
    bx = im.reg_x0[c] + local % gw; by = im.reg_y0[c] + local / gw;
  }
  int32_t* const w = ws[wave] + j * kIdctBlockStride;
  int32_t ycol[8] = {0, 0, 0, 0, 0, 0, 0, 0};               // Y's quantised column k (4:4:4), for the chroma steps
  size_t tile = 0;
  for (uint32_t step = 0; step < steps; step++) {
    if (walk) c = step;
    const uint32_t ch = im.ncomp == 1 ? 1u : (c == 0 ? 1u : c == 1 ? 0u : 2u);
    const uint32_t hs = c ? im.hs : 0u, vs = c ? im.vs : 0u;
    const uint32_t n = kScaled ? im.n[c] : 8u, pitch = kScaled ? im.pitch[c] : im.grid_w[c] * 8u;      // (scale 1: the branches on n below fold away)
    const uint32_t sx = bx << hs, sy = by << vs;            // the frame block that carries this component block
    const bool live = pos < im.npos && bx < im.grid_w[c] && by < im.grid_h[c] && sx < f.bw && sy < f.bh;
    if (live) {
      const size_t o = (size_t)sy * f.bw + sx;
      if (k == 0 && (f.blk_info[o] & 31u) != 0) atomicOr(f.status, (uint32_t)kErrVarblock);
      const uint32_t g = (sy / 32) * f.xgroups + sx / 32;
      const uint32_t coff = min(f.coef_off[o] & ~63u, 65536u - 64u);
      int4* const src = (int4*)(f.coeff[ch] + (size_t)g * 65536 + coff + k * 8);
      const int4 lo = src[0], hi = src[1];
      if (lo.x | lo.y | lo.z | lo.w) src[0] = make_int4(0, 0, 0, 0);      // consumed — also what a reduced transform does not use: the planes stay clean for the next decode
      if (hi.x | hi.y | hi.z | hi.w) src[1] = make_int4(0, 0, 0, 0);
      int32_t cf[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};   // cf[v]: coefficient (v, u = k)
      const int4 qlo = *(const int4*)(im.qt[c] + k * 8), qhi = *(const int4*)(im.qt[c] + k * 8 + 4);
      const int32_t q[8] = {qlo.x, qlo.y, qlo.z, qlo.w, qhi.x, qhi.y, qhi.z, qhi.w};
      if (walk) {
        if (c == 0) {
          tile = (size_t)(sy / 8) * f.cw + sx / 8;
#pragma unroll
          for (int r = 0; r < 8; r++) ycol[r] = cf[r];
        } else {
          const int32_t ff = JpegCflFactor(c == 1 ? (int32_t)f.ytox[tile] : (int32_t)f.ytob[tile]);
          const int32_t* __restrict__ ratio = im.cfl_ratio[c - 1] + k * 8;   // 2048 qt[0][i] / qt[c][i], the host's division
          const int4 rlo = *(const int4*)ratio, rhi = *(const int4*)(ratio + 4);
          const int32_t rt[8] = {rlo.x, rlo.y, rlo.z, rlo.w, rhi.x, rhi.y, rhi.z, rhi.w};
#pragma unroll
          for (int r = 0; r < 8; r++) cf[r] = (int32_t)((uint32_t)cf[r] + (uint32_t)JpegCflTerm(ycol[r], rt[r], ff));
        }
      }
      if (k == 0) cf[0] = f.lfq[ch][(size_t)by * f.bw + bx];              // (no chroma from luma on the DC term: the LF stage has its own)
      uint32_t in[8];
#pragma unroll
      for (int r = 0; r < 8; r++) in[r] = (uint32_t)(int32_t)(int16_t)cf[r] * (uint32_t)q[r];     // (int16_t: the width JPEG gives a coefficient, as JpegCoefKernel stores it)
      if (n == 8) {
        int32_t col[8];
        JpegIdct1D<11>(in, col);
#pragma unroll
        for (int r = 0; r < 8; r++) w[r * 8 + k] = col[r];
      } else if (n == 4) {
        if (k != 4) {
          int32_t col[4];
          JpegIdct1D4<12>(in, col);
#pragma unroll
          for (int r = 0; r < 4; r++) w[r * 8 + k] = col[r];
        }
      } else if (n == 2) {
        if (k == 0 || (k & 1)) {
          int32_t col[2];
          JpegIdct1D2<13>(in, col);
          w[k] = col[0]; w[8 + k] = col[1];
        }
      } else if (k == 0) w[0] = (int32_t)in[0];
    }
    __syncthreads();
    if (live && k < n) {
      uint32_t in[8];
      const int4 lo = *(const int4*)(w + k * 8), hi = *(const int4*)(w + k * 8 + 4);
      in[0] = (uint32_t)lo.x; in[1] = (uint32_t)lo.y; in[2] = (uint32_t)lo.z; in[3] = (uint32_t)lo.w;
      in[4] = (uint32_t)hi.x; in[5] = (uint32_t)hi.y; in[6] = (uint32_t)hi.z; in[7] = (uint32_t)hi.w;
      uint8_t* const dst = im.plane[c] + ((size_t)by * n + k) * (size_t)pitch + (size_t)bx * n;
      if (n == 8) {
        int32_t row[8];
        JpegIdct1D<18>(in, row);
        uint2 px;
        px.x = ClampU8(row[0] + 128) | ClampU8(row[1] + 128) << 8 | ClampU8(row[2] + 128) << 16 | ClampU8(row[3] + 128) << 24;
        px.y = ClampU8(row[4] + 128) | ClampU8(row[5] + 128) << 8 | ClampU8(row[6] + 128) << 16 | ClampU8(row[7] + 128) << 24;
        *(uint2*)dst = px;
      } else if (n == 4) {
        int32_t row[4];
        JpegIdct1D4<19>(in, row);
        *(uint32_t*)dst = ClampU8(row[0] + 128) | ClampU8(row[1] + 128) << 8 | ClampU8(row[2] + 128) << 16 | ClampU8(row[3] + 128) << 24;
      } else if (n == 2) {
        int32_t row[2];
        JpegIdct1D2<20>(in, row);
        *(uint16_t*)dst = (uint16_t)(ClampU8(row[0] + 128) | ClampU8(row[1] + 128) << 8);
      } else *dst = (uint8_t)ClampU8(Descale<3>(in[0]) + 128);
    }
    if (step + 1 < steps) __syncthreads();                  // (the next step's pass 1 overwrites the workspace)
  }
}

__global__ __launch_bounds__(256) void JpegIdctPlanesKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) int32_t ws[kIdctWaves][kIdctBlocksPerWave * kIdctBlockStride];
  JpegIdctBody<false>(frames, table, ws);
}
__global__ __launch_bounds__(256) void JpegIdctScaledKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) int32_t ws[kIdctWaves][kIdctBlocksPerWave * kIdctBlockStride];
  JpegIdctBody<true>(frames, table, ws);
}

// The quantised coefficients of a group of images from the HF stage's planes into the int16 arena of the JPEG writer (jpeg_write.hip; decoder.cc Batch::PlanJpegWrite):
// natural order, component planes back to back from im.coef_out on, grids as the table says.  What JpegCoefKernel (kernels_features.hip) does per image with a thread
// per coefficient, in one launch per group and with the access pattern of JpegIdctPlanesKernel above — the same positions (eight per wavefront, lane = (position j, k),
// a 4:4:4 colour position walks Y, Cb, Cr), the same mapping of a component block to its frame block, its group and its 64 dwords, the same two 16-byte loads of column
// u = k, the same zeroing of what was read, the same DC term from lfq, the same chroma from luma (pixel_ops.h JpegCflTerm) with Y's column kept in registers.  Only the
// shifts are per component here (comp_hs / comp_vs: reconstruction also takes samplings the pixel path refuses), and chroma from luma applies when all of them are 0.
//   One reader per dword, as above: a (channel, frame block) pair belongs to exactly one (position, step), and of its 64 dwords lane k alone reads — and then zeroes —
//   8 k .. 8 k + 7.  So there is no order between wavefronts or workgroups to get wrong; the coefficient set is clean behind the launch, except for frames that
//   failed (a block that is not DCT8 sets kErrVarblock; a failed frame is skipped from then on): those are zeroed whole by ZeroFailedCoefKernel behind the launch.
//   Addresses: every one comes from the host's table and the frame's grid; (sx << hs, sy << vs) is checked against the frame's grid, coef_off is brought to a multiple
//   of 64 at most 65536 - 64.  The stream decides values only.
//   Transpose: the lane holds column u = k, eight values v = 0 .. 7, the arena wants out[v x 8 + u] as int16_t.  Through LDS, 128 bytes per block and 1 KB per
//   wavefront, no padding: row v of block j lives in the 16-byte slot 8 j + (v ^ 2 (j & 3)).
//     Column stores: lanes k and k ^ 1 first exchange half of their values (two __shfl_xor of packed pairs), so that the even lane holds the dwords {u = k, k + 1} of
//     rows 0, 2, 4, 6 and the odd lane those of rows 1, 3, 5, 7: four ds_write_b32 per lane.  Store i of lane (j, k) goes to row v = 2 i + (k & 1), dword
//     32 j + 4 (v ^ 2 (j & 3)) + (k >> 1).  Banks of a store are (a / 4) % 32, one 32-lane half (j & 3 = 0 .. 3, k) at a time: v ^ 2 (j & 3) =
//     2 (i ^ (j & 3)) + (k & 1) takes each of the eight slots once over ((j & 3), (k & 1)), and k >> 1 the four dwords of a slot: 32 lanes, 32 banks.
//     Row loads: lane (j, k) reads slot 8 j + k with one ds_read_b128 — row v = k ^ 2 (j & 3) of its block.  Banks of that load are (a / 4) % 64, sixteen 16-byte
//     slots, over the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and the same + 32): the slots 8 j + k mod 16 of a group are {0-3}, {12-15}, {4-7},
//     {8-11} resp. {4-7}, {8-11}, {0-3}, {12-15}: all sixteen different.
//   The lane then stores its row as one 16-byte vector; the eight lanes of a block fill one contiguous, 128-byte aligned run of 128 bytes.
__global__ __launch_bounds__(256) void JpegGatherKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) uint32_t ts[kIdctWaves][kIdctBlocksPerWave * 32];
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  if (blockIdx.x * (kIdctWaves * kIdctBlocksPerWave) >= im.npos || *f.status != 0) return;     // (a failed frame's planes are zeroed by ZeroFailedCoefKernel)
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane >> 3, k = lane & 7;
  const uint32_t pos = (blockIdx.x * kIdctWaves + wave) * kIdctBlocksPerWave + j;
  const bool walk = im.ncomp == 3 && !(im.comp_hs[0] | im.comp_vs[0] | im.comp_hs[1] | im.comp_vs[1] | im.comp_hs[2] | im.comp_vs[2]);   // 4:4:4: Y, Cb, Cr of one block position
  const uint32_t steps = walk ? 3u : 1u;                     // (uniform over the workgroup: the barriers below are reached by all of it)
  uint32_t c = 0, bx = 0, by = 0;
  {
    if (!walk && im.ncomp == 3) c = pos >= im.comp_first[2] ? 2u : pos >= im.comp_first[1] ? 1u : 0u;
    const uint32_t local = pos - (walk ? 0u : im.comp_first[c]), gw = im.grid_w[c];
    bx = local % gw; by = local / gw;
  }
  uint32_t* const tw = ts[wave] + j * 32;
  const uint32_t sw = 2 * (j & 3), odd = k & 1;
  int32_t ycol[8] = {0, 0, 0, 0, 0, 0, 0, 0};               // Y's quantised column k (4:4:4), for the chroma steps
  size_t tile = 0;
  for (uint32_t step = 0; step < steps; step++) {
    if (walk) c = step;
    const uint32_t ch = im.ncomp == 1 ? 1u : (c == 0 ? 1u : c == 1 ? 0u : 2u);
    const uint32_t hs = im.comp_hs[c], vs = im.comp_vs[c], gw = im.grid_w[c];
    const uint32_t sx = bx << hs, sy = by << vs;            // the frame block that carries this component block
    const bool live = pos < im.npos && by < im.grid_h[c] && sx < f.bw && sy < f.bh;
    int32_t cf[8] = {0, 0, 0, 0, 0, 0, 0, 0};               // cf[v]: coefficient (v, u = k)
    if (live) {
      const size_t o = (size_t)sy * f.bw + sx;
      if (k == 0 && (f.blk_info[o] & 31u) != 0) atomicOr(f.status, (uint32_t)kErrVarblock);
      const uint32_t g = (sy / 32) * f.xgroups + sx / 32;
      const uint32_t coff = min(f.coef_off[o] & ~63u, 65536u - 64u);
      int4* const src = (int4*)(f.coeff[ch] + (size_t)g * 65536 + coff + k * 8);
      const int4 lo = src[0], hi = src[1];
      if (lo.x | lo.y | lo.z | lo.w) src[0] = make_int4(0, 0, 0, 0);      // consumed: the coefficient set stays clean for its next user
      if (hi.x | hi.y | hi.z | hi.w) src[1] = make_int4(0, 0, 0, 0);
      cf[0] = lo.x; cf[1] = lo.y; cf[2] = lo.z; cf[3] = lo.w; cf[4] = hi.x; cf[5] = hi.y; cf[6] = hi.z; cf[7] = hi.w;
      if (walk) {
        if (c == 0) {
          tile = (size_t)(sy / 8) * f.cw + sx / 8;
#pragma unroll
          for (int r = 0; r < 8; r++) ycol[r] = cf[r];
        } else {
          const int32_t ff = JpegCflFactor(c == 1 ? (int32_t)f.ytox[tile] : (int32_t)f.ytob[tile]);
          const int32_t* __restrict__ ratio = im.cfl_ratio[c - 1] + k * 8;   // 2048 qt[0][i] / qt[c][i], the host's division
          const int4 rlo = *(const int4*)ratio, rhi = *(const int4*)(ratio + 4);
          const int32_t rt[8] = {rlo.x, rlo.y, rlo.z, rlo.w, rhi.x, rhi.y, rhi.z, rhi.w};
#pragma unroll
          for (int r = 0; r < 8; r++) cf[r] = (int32_t)((uint32_t)cf[r] + (uint32_t)JpegCflTerm(ycol[r], rt[r], ff));
        }
      }
      if (k == 0) cf[0] = f.lfq[ch][(size_t)by * f.bw + bx];              // (no chroma from luma on the DC term: the LF stage has its own)
    }
    // (int16_t: the width JPEG gives a coefficient, as JpegCoefKernel stores it.)  The lane sends the rows its partner k ^ 1 stores: the odd lane its even rows.
    uint32_t p[8];
#pragma unroll
    for (int r = 0; r < 8; r++) p[r] = (uint32_t)cf[r] & 0xFFFFu;
    const uint32_t r0 = (uint32_t)__shfl_xor((int)(odd ? p[0] | p[2] << 16 : p[1] | p[3] << 16), 1, 64);
    const uint32_t r1 = (uint32_t)__shfl_xor((int)(odd ? p[4] | p[6] << 16 : p[5] | p[7] << 16), 1, 64);
    uint32_t d[4];
    if (odd) { d[0] = (r0 & 0xFFFFu) | p[1] << 16; d[1] = (r0 >> 16) | p[3] << 16; d[2] = (r1 & 0xFFFFu) | p[5] << 16; d[3] = (r1 >> 16) | p[7] << 16; }
    else { d[0] = p[0] | r0 << 16; d[1] = p[2] | (r0 >> 16) << 16; d[2] = p[4] | r1 << 16; d[3] = p[6] | (r1 >> 16) << 16; }
#pragma unroll
    for (uint32_t i = 0; i < 4; i++) tw[4 * ((2 * i + odd) ^ sw) + (k >> 1)] = d[i];
    __syncthreads();
    if (live) {
      const uint4 row = *(const uint4*)(tw + 4 * k);
      const uint32_t v = k ^ sw;
      *(uint4*)(im.coef_out + ((size_t)im.comp_first[c] + (size_t)by * gw + bx) * 64 + v * 8) = row;
    }
    if (step + 1 < steps) __syncthreads();                  // (the next step's column stores overwrite the rows)
  }
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

// The end of all three colour-out kernels: the npix (1 or 2) pixels (x0, y), (x0 + 1, y) of a w x h picture from their u8 component samples — grey (ncomp == 1) as
// they are, else fixed-point YCbCr -> RGB (jdcolor.c) — into the write stage; sample k enters it as (float)k x (1 / 255)
// (`from`: 1 leaves pixel x0 out — the pair straddles the left edge of the rectangle a region's colour launch is confined to)
__device__ __forceinline__ void StoreJpegPair(const OutputDesc& od, uint32_t ncomp, uint32_t w, uint32_t h, uint32_t x0, uint32_t y, uint32_t npix, const int32_t lum[2],
                                              const int32_t cb[2], const int32_t cr[2], uint32_t from = 0) {
  const float k255 = 1.0f / 255;
  if (ncomp == 1) {
    for (uint32_t i = from; i < npix; i++) { const float v = (float)lum[i] * k255; StorePixel(od, (int)w, (int)h, (int)(x0 + i), (int)y, v, v, v, 1.0f); }
    return;
  }
  for (uint32_t i = from; i < npix; i++) {
    const int32_t u = cb[i] - 128, v = cr[i] - 128;
    const int32_t r = min(max(lum[i] + ((91881 * v + 32768) >> 16), 0), 255);
    const int32_t g = min(max(lum[i] + ((-22554 * u - 46802 * v + 32768) >> 16), 0), 255);
    const int32_t b = min(max(lum[i] + ((116130 * u + 32768) >> 16), 0), 255);
    StorePixel(od, (int)w, (int)h, (int)(x0 + i), (int)y, (float)r * k255, (float)g * k255, (float)b * k255, 1.0f);
  }
}

// A thread takes the output pixels (2 t, 2 t + 1) of a row: they share their chroma position in the subsampled modes.
// The launch covers the rectangle im.rect_* of the picture and writes no pixel outside it: the whole picture, or — an image decoded by region (Batch::JpegRegion) — the
// crop mapped to the stored picture, the only part of the intermediate the resample reads.  The edge rules of ChromaPair stay those of the *picture* (cw x ch is the
// component's extent): at a rectangle's edge inside the picture the neighbouring chroma sample is a real one, decoded with the margin of one MCU the region has.
__global__ __launch_bounds__(256) void JpegColorOutKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  const uint32_t t = (im.rect_x0 >> 1) + blockIdx.x * 32 + threadIdx.x, x0 = t * 2, y = im.rect_y0 + blockIdx.y * 8 + threadIdx.y;
  const uint32_t xe = min(im.rect_x0 + im.rect_w, im.width), ye = min(im.rect_y0 + im.rect_h, im.height);
  if (x0 >= xe || y >= ye || *f.status != 0) return;
  const uint32_t npix = x0 + 1 < xe ? 2 : 1, from = x0 < im.rect_x0 ? 1u : 0u;
  if (from >= npix) return;
  const uint8_t* __restrict__ yrow = im.plane[0] + (size_t)y * ((size_t)im.grid_w[0] * 8);
  const int32_t lum[2] = {yrow[x0], yrow[x0 + 1]};      // (x0 + 1 is inside the padded grid: its width is a multiple of 8)
  int32_t cb[2] = {128, 128}, cr[2] = {128, 128};
  if (im.ncomp == 1) {
  } else if (!im.hs) {
    const size_t o = (size_t)y * ((size_t)im.grid_w[1] * 8) + x0;
    cb[0] = im.plane[1][o]; cb[1] = im.plane[1][o + 1]; cr[0] = im.plane[2][o]; cr[1] = im.plane[2][o + 1];
  } else {
    const uint32_t cw = (im.width + 1) >> 1, ch = (im.height + (1u << im.vs) - 1) >> im.vs, pitch = im.grid_w[1] * 8;
    ChromaPair(im.plane[1], pitch, im.vs, cw, ch, t, y, cb);
    ChromaPair(im.plane[2], pitch, im.vs, cw, ch, t, y, cr);
  }
  StoreJpegPair(f.od, im.ncomp, im.width, im.height, x0, y, npix, lum, cb, cr, from);
}

// JpegColorOutKernel for libjpeg's scaled decodes: the picture is im.out_w x im.out_h, component c's plane has im.pitch[c] bytes per row and im.ext_w[c] x im.ext_h[c]
// real samples.  Luma always has the picture's extent, chroma too at 4:4:4 and at 4:2:0 (whose chroma took the IDCT of twice the size: jdmaster.c) — no upsampling at
// all; 4:2:2 chroma (im.chroma_up) has half the width: jdsample.c's h2v1 "fancy" rule if the smallest IDCT is larger than 1 x 1 (im.chroma_fancy) and the plane is more
// than two samples wide, else plain replication.  A thread takes the output pixels (2 t, 2 t + 1) of a row, as above; colour conversion and the write stage are the same.
__global__ __launch_bounds__(256) void JpegColorOutScaledKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  // (confined to im.rect_*, a rectangle of the scaled picture, as JpegColorOutKernel is)
  const uint32_t t = (im.rect_x0 >> 1) + blockIdx.x * 32 + threadIdx.x, x0 = t * 2, y = im.rect_y0 + blockIdx.y * 8 + threadIdx.y;
  const uint32_t xe = min(im.rect_x0 + im.rect_w, im.out_w), ye = min(im.rect_y0 + im.rect_h, im.out_h);
  if (x0 >= xe || y >= ye || *f.status != 0) return;
  const uint32_t npix = x0 + 1 < xe ? 2 : 1, from = x0 < im.rect_x0 ? 1u : 0u;
  if (from >= npix) return;
  const uint8_t* __restrict__ yrow = im.plane[0] + (size_t)y * im.pitch[0];
  const int32_t lum[2] = {yrow[x0], npix == 2 ? yrow[x0 + 1] : 0};      // (a row of n = 1 samples per block may end at x0)
  int32_t cb[2] = {128, 128}, cr[2] = {128, 128};
  if (im.ncomp == 1) {
  } else if (!im.chroma_up) {
    const size_t o = (size_t)y * im.pitch[1] + x0, o1 = o + (npix == 2 ? 1 : 0);
    cb[0] = im.plane[1][o]; cb[1] = im.plane[1][o1]; cr[0] = im.plane[2][o]; cr[1] = im.plane[2][o1];
  } else {
    // (t < ext_w: out_w <= 2 ext_w.  A width of at most 2 makes ChromaPair replicate)
    const uint32_t cw = im.chroma_fancy ? im.ext_w[1] : 1u;
    ChromaPair(im.plane[1], im.pitch[1], 0, cw, im.ext_h[1], t, y, cb);
    ChromaPair(im.plane[2], im.pitch[1], 0, cw, im.ext_h[1], t, y, cr);
  }
  StoreJpegPair(f.od, im.ncomp, im.out_w, im.out_h, x0, y, npix, lum, cb, cr, from);
}

// libjpeg's 1/8 decode of an image whose components all take the 1 x 1 "IDCT" (grey, 4:4:4, 4:2:2 at scale 8 — JpegPixelImage::n[c] == 1 for every c; the entries of a
// kJpegGroupDc run): the n = 1 case of JpegIdctScaledKernel + JpegColorOutScaledKernel with nothing in between.  A sample is clamp(DESCALE(dc x qt[c][0], 3) + 128) of
// one DC term, and the DC terms are FrameDev::lfq, which the LF stage wrote: the frame has no coefficient planes and no pixel planes (FrameDev::lf_only ==
// kLfOnlyJpegDc), the HF stage never ran for it.  A thread takes the output pixels (2 t, 2 t + 1) of a row, as above.
//   Luma sample (x, y) is the DC term of component block (x, y): lfq[Y] at y x f.bw + x (the LF planes have the frame grid's pitch, whatever the component's grid is).
//   Chroma (x >> hs, y): 4:2:2 replicates — jdsample.c has no fancy upsampling when the smallest IDCT is 1 x 1 (chroma_fancy == 0), and vs == 0 for every entry here.
//   Loads: two dwords per component and thread, lanes on consecutive pairs — a row of a wavefront is one contiguous run of 64 dwords, read by two instructions of 8-byte
//   lane stride, both out of the same lines.  No 8-byte load: y x f.bw + x0 is odd for odd f.bw and y.  At 4:2:2 both pixels take the one chroma dword t.
//   Addresses: x < out_w <= grid_w[0] <= f.bw and y < out_h <= grid_h[0] <= f.bh, x >> hs < grid_w[1], all from the host's table (PlanJpegPixels checks the grids against
//   the frame's); the stream decides values only.  The product is formed in uint32_t like every sum here.
//   A block that is not DCT8 fails the frame with kErrVarblock as in JpegIdctBody (block info is the LF stage's): the lane of a block's luma sample looks at it; the
//   frame block of a 4:2:2 chroma block, (2 t, y), is one of those.  Pixels other lanes stored before the word was set mean nothing: the image has failed.
__global__ __launch_bounds__(256) void JpegDcOutKernel(const FrameDev* __restrict__ frames, const JpegPixelImage* __restrict__ table) {
  const JpegPixelImage& im = table[blockIdx.z];
  const FrameDev& f = frames[im.frame];
  const uint32_t t = blockIdx.x * 32 + threadIdx.x, x0 = t * 2, y = blockIdx.y * 8 + threadIdx.y;
  if (x0 >= im.out_w || y >= im.out_h || x0 >= f.bw || y >= f.bh || *f.status != 0) return;
  const uint32_t npix = x0 + 1 < im.out_w && x0 + 1 < f.bw ? 2 : 1;
  const size_t row = (size_t)y * f.bw;
  auto sample = [&](uint32_t c, uint32_t ch, uint32_t x) -> int32_t {
    return (int32_t)ClampU8(Descale<3>((uint32_t)(int32_t)(int16_t)f.lfq[ch][row + x] * (uint32_t)im.qt[c][0]) + 128);      // (int16_t: the width JPEG gives a coefficient, as in JpegIdctBody)
  };
  uint32_t other = 0;
  for (uint32_t i = 0; i < npix; i++) other |= f.blk_info[row + x0 + i] & 31u;
  const int32_t lum[2] = {sample(0, 1, x0), npix == 2 ? sample(0, 1, x0 + 1) : 0};      // (Y lives in channel 1, Cb in the X slot 0, Cr in the B slot 2)
  int32_t cb[2] = {128, 128}, cr[2] = {128, 128};
  if (im.ncomp == 3) {
    const uint32_t hs = im.hs ? 1u : 0u;
    const uint32_t c0 = x0 >> hs, c1 = npix == 2 ? (x0 + 1) >> hs : c0;      // (4:2:2: c0 == c1 == t, whose frame block (2 t, y) is the luma block looked at above)
    cb[0] = sample(1, 0, c0); cr[0] = sample(2, 2, c0);
    if (c1 != c0) { cb[1] = sample(1, 0, c1); cr[1] = sample(2, 2, c1); } else { cb[1] = cb[0]; cr[1] = cr[0]; }
  }
  if (other) { atomicOr(f.status, (uint32_t)kErrVarblock); return; }
  StoreJpegPair(f.od, im.ncomp, im.out_w, im.out_h, x0, y, npix, lum, cb, cr);
}

}  // namespace

void LaunchJpegIdctGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream) {
  if (!g.count || g.count > kJpegPixelGroupMax || !g.max_npos || !g.max_w || !g.max_h || g.scaled == kJpegGroupDc) return;     // (a DC-only run has no coefficients)
  const uint32_t per_wg = kIdctWaves * kIdctBlocksPerWave;
  if (g.scaled) hipLaunchKernelGGL(JpegIdctScaledKernel, dim3((g.max_npos + per_wg - 1) / per_wg, 1, g.count), dim3(256), 0, (hipStream_t)stream, frames, table + g.first);
  else hipLaunchKernelGGL(JpegIdctPlanesKernel, dim3((g.max_npos + per_wg - 1) / per_wg, 1, g.count), dim3(256), 0, (hipStream_t)stream, frames, table + g.first);
}
void LaunchJpegGatherGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream) {
  if (!g.count || g.count > kJpegPixelGroupMax || !g.max_npos) return;
  const uint32_t per_wg = kIdctWaves * kIdctBlocksPerWave;
  hipLaunchKernelGGL(JpegGatherKernel, dim3((g.max_npos + per_wg - 1) / per_wg, 1, g.count), dim3(256), 0, (hipStream_t)stream, frames, table + g.first);
}
void LaunchJpegColorOutGroup(const FrameDev* frames, const JpegPixelImage* table, const JpegPixelGroup& g, void* stream) {
  if (!g.count || g.count > kJpegPixelGroupMax || !g.max_npos || !g.max_w || !g.max_h) return;
  if (g.scaled == kJpegGroupDc) hipLaunchKernelGGL(JpegDcOutKernel, dim3((g.max_w + 63) / 64, (g.max_h + 7) / 8, g.count), dim3(32, 8), 0, (hipStream_t)stream, frames, table + g.first);
  else if (g.scaled) hipLaunchKernelGGL(JpegColorOutScaledKernel, dim3((g.max_w + 63) / 64, (g.max_h + 7) / 8, g.count), dim3(32, 8), 0, (hipStream_t)stream, frames, table + g.first);
  else hipLaunchKernelGGL(JpegColorOutKernel, dim3((g.max_w + 63) / 64, (g.max_h + 7) / 8, g.count), dim3(32, 8), 0, (hipStream_t)stream, frames, table + g.first);
}

}  // namespace jxlhip
