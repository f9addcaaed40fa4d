// jxl-hip: device-side writer of sequential Huffman JPEG scans (batch JPEG reconstruction, decoder.cc Batch::ReconstructJpegs).
// Input: the int16 coefficient planes JpegCoefKernel leaves in device memory (natural order, MCU-padded block grids).  Output: for every
// restart segment of every eligible scan the byte-stuffed bytes of its complete bytes plus the bits of its last, incomplete byte; the host
// pads that byte and splices the segments between the markers (jpeg_recon.cc SpliceJpegScan).
//   pass 1   JpegBlockBitsKernel   one wavefront per 8x8 block, lane k = zigzag coefficient k: bits of the block's Huffman code
//   offsets  ScanU32 (tile sums, scan of the tile sums, per-tile scan): bit position of every block; JpegSegBytesKernel: bytes per restart
//            segment (every segment starts on a byte), scanned again into the segment's place in the raw buffer
//   pass 2   JpegPackKernel        the same symbols again, written MSB-first at the block's bit position with atomicOr on a zeroed buffer
//   stuffing JpegCountFFKernel per 1024-byte chunk, scan, JpegStuffKernel copies with 00 behind every FF; JpegSegRecordKernel says where
//            every segment landed
// Both passes derive a lane's code from JpegLaneCode, so the sizes of pass 1 are exactly what pass 2 writes; pass 2 checks every store
// against the block's own bit count and the buffer size all the same.
#include "kernels.h"
#include <hip/hip_runtime.h>

namespace jxlhip {

namespace {

__constant__ uint8_t kJpegNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the scan a block / segment of the batch-wide arrays belongs to (first_block / first_seg ascend; empty scans share a start and are skipped)
template <bool kBySeg>
__device__ inline const JpegScanDev& FindScan(const JpegScanDev* scans, uint32_t n, uint32_t idx) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if ((kBySeg ? scans[mid].first_seg : scans[mid].first_block) <= idx) lo = mid; else hi = mid;
  }
  return scans[lo];
}

// Where block `b` of the batch sits: its coefficients, the block its DC is predicted from (the previous block of the same component in scan
// order; none at the start of the scan and behind a restart boundary), its restart segment and Huffman tables.
struct BlockRef { uint32_t blk, pred, seg, seg_first, dc, ac; bool has_pred; };
__device__ inline BlockRef LocateBlock(const JpegScanDev& s, uint32_t b) {
  BlockRef r;
  const uint32_t sb = b - s.first_block, mcu = sb / s.blocks_per_mcu;
  uint32_t j = sb % s.blocks_per_mcu, ci = 0;
  for (; ci + 1 < s.ncomp; ci++) { const uint32_t cnt = (uint32_t)s.h[ci] * s.v[ci]; if (j < cnt) break; j -= cnt; }
  const uint32_t h = s.h[ci], v = s.v[ci], my = mcu / s.scan_cols, mx = mcu % s.scan_cols;
  r.blk = s.plane[ci] + (my * v + j / h) * s.pitch[ci] + mx * h + j % h;
  r.dc = s.dc[ci]; r.ac = s.ac[ci];
  const uint32_t segk = s.restart ? mcu / s.restart : 0;
  r.seg = s.first_seg + segk;
  r.seg_first = s.first_block + segk * s.restart * s.blocks_per_mcu;
  r.has_pred = true; r.pred = 0;
  if (j > 0) r.pred = s.plane[ci] + (my * v + (j - 1) / h) * s.pitch[ci] + mx * h + (j - 1) % h;
  else if (mcu == 0 || (s.restart && mcu % s.restart == 0)) r.has_pred = false;
  else { const uint32_t pm = mcu - 1, py = pm / s.scan_cols, px = pm % s.scan_cols; r.pred = s.plane[ci] + (py * v + v - 1) * s.pitch[ci] + px * h + h - 1; }
  return r;
}

// What lane `lane` (zigzag position) contributes to its block's code: up to three ZRL symbols (zrl_n codes of zrl_len bits) and one piece
// of at most 31 bits (Huffman code + magnitude bits; the DC difference in lane 0, the end-of-block symbol in lane 63 when that coefficient is
// zero).  A lane that meets one of the host writer's errors contributes nothing and reports it: 1 DC category >= 12, 2 AC category >= 16,
// 4 a symbol the table has no code for.
struct LaneCode { uint32_t zrl_code, zrl_len, zrl_n, bits, len, err; };
__device__ inline LaneCode JpegLaneCode(int c, uint32_t lane, uint64_t ac_mask, int pred, const JpegHuffDev& dct, const JpegHuffDev& act) {
  LaneCode o = {0, 0, 0, 0, 0, 0};
  if (lane == 0) {
    int temp = c - pred, temp2 = temp;
    if (temp < 0) { temp = -temp; temp2--; }
    const uint32_t nbits = temp ? 32 - __builtin_clz((uint32_t)temp) : 0;
    if (nbits >= 12) { o.err = 1; return o; }
    const uint32_t d = dct.depth[nbits];
    if (d > 16) { o.err = 4; return o; }
    o.bits = (((uint32_t)dct.code[nbits] & ((1u << d) - 1u)) << nbits) | ((uint32_t)temp2 & ((1u << nbits) - 1u));
    o.len = d + nbits;
    return o;
  }
  if (c == 0) {
    if (lane != 63) return o;
    const uint32_t d = act.depth[0];                       // trailing zeros: end of block
    if (d > 16) { o.err = 4; return o; }
    o.bits = act.code[0] & ((1u << d) - 1u); o.len = d;
    return o;
  }
  const uint32_t temp = (uint32_t)(c < 0 ? -c : c), temp2 = (uint32_t)(c < 0 ? c - 1 : c);
  const uint32_t nbits = 32 - __builtin_clz(temp);
  if (nbits >= 16) { o.err = 2; return o; }
  const uint64_t below = ac_mask & ((1ull << lane) - 1ull);
  const uint32_t prev = below ? 63 - __builtin_clzll(below) : 0, run = lane - prev - 1;
  const uint32_t sym = ((run & 15) << 4) | nbits, d = act.depth[sym];
  o.zrl_n = run >> 4;
  if (o.zrl_n) { o.zrl_len = act.depth[0xF0]; o.zrl_code = act.code[0xF0] & ((1u << (o.zrl_len & 31)) - 1u); }
  if (d > 16 || o.zrl_len > 16) { o.zrl_n = o.zrl_len = 0; o.err = 4; return o; }
  o.bits = (((uint32_t)act.code[sym] & ((1u << d) - 1u)) << nbits) | (temp2 & ((1u << nbits) - 1u));
  o.len = d + nbits;
  return o;
}

__device__ inline LaneCode BlockLaneCode(const JpegWritePlan& p, const JpegScanDev& s, const BlockRef& r, uint32_t lane) {
  const int c = p.coef[(size_t)r.blk * 64 + kJpegNatural[lane]];
  const int pred = r.has_pred ? (int)p.coef[(size_t)r.pred * 64] : 0;
  const uint64_t ac_mask = __ballot(c != 0) & ~1ull;
  return JpegLaneCode(c, lane, ac_mask, pred, p.tables[r.dc], p.tables[r.ac]);
}

// ---- pass 1: bits per block ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void JpegBlockBitsKernel(JpegWritePlan p) {
  const uint32_t b = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (b >= p.num_blocks) return;
  const JpegScanDev& s = FindScan<false>(p.scans, p.num_scans, b);
  if (*p.frames[s.frame].status != 0) { if (lane == 0) p.bits[b] = 0; return; }      // (a frame whose entropy stages failed has no coefficients)
  const BlockRef r = LocateBlock(s, b);
  const LaneCode lc = BlockLaneCode(p, s, r, lane);
  uint32_t n = lc.zrl_n * lc.zrl_len + lc.len, err = lc.err;
  for (int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d, 64); err |= __shfl_xor(err, d, 64); }
  if (lane == 0) {
    p.bits[b] = n;
    if (err) atomicOr(&p.flags[s.image], err);
  }
}

// ---- exclusive scan of n uint32 values into n + 1 uint64 (out[n] = total): tiles of 1024 ------------------------------------------------
__device__ inline uint64_t BlockExclusiveScan(uint64_t v, uint64_t* lds, uint64_t* total) {     // 256 threads
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint64_t o = t >= d ? lds[t - d] : 0;
    __syncthreads();
    lds[t] += o;
    __syncthreads();
  }
  const uint64_t incl = lds[t];
  *total = lds[255];
  __syncthreads();
  return incl - v;
}
__global__ __launch_bounds__(256) void ScanTileSumKernel(const uint32_t* __restrict__ in, uint32_t n, uint64_t* __restrict__ tile_sum) {
  __shared__ uint64_t lds[256];
  const uint32_t i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  uint64_t v = 0;
  for (uint32_t k = 0; k < 4; k++) if (i0 + k < n) v += in[i0 + k];
  uint64_t total;
  BlockExclusiveScan(v, lds, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void ScanTilePrefixKernel(uint64_t* __restrict__ tile_sum, uint32_t ntiles, uint64_t* __restrict__ out_total) {
  __shared__ uint64_t lds[256];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < ntiles; base += 256) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = i < ntiles ? tile_sum[i] : 0;
    uint64_t total;
    const uint64_t ex = BlockExclusiveScan(v, lds, &total);
    if (i < ntiles) tile_sum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *out_total = carry;
}
__global__ __launch_bounds__(256) void ScanTileApplyKernel(const uint32_t* __restrict__ in, uint32_t n, const uint64_t* __restrict__ tile_prefix, uint64_t* __restrict__ out) {
  __shared__ uint64_t lds[256];
  const uint32_t i0 = blockIdx.x * 1024 + threadIdx.x * 4;
  uint32_t x[4];
  uint64_t v = 0;
  for (uint32_t k = 0; k < 4; k++) { x[k] = i0 + k < n ? in[i0 + k] : 0; v += x[k]; }
  uint64_t total;
  uint64_t pos = tile_prefix[blockIdx.x] + BlockExclusiveScan(v, lds, &total);
  for (uint32_t k = 0; k < 4; k++) { if (i0 + k < n) out[i0 + k] = pos; pos += x[k]; }
}
void ScanU32(const uint32_t* in, uint32_t n, uint64_t* out, uint64_t* tile_tmp, hipStream_t stream) {
  const uint32_t ntiles = (n + 1023) / 1024;
  if (ntiles) hipLaunchKernelGGL(ScanTileSumKernel, dim3(ntiles), dim3(256), 0, stream, in, n, tile_tmp);
  hipLaunchKernelGGL(ScanTilePrefixKernel, dim3(1), dim3(256), 0, stream, tile_tmp, ntiles, out + n);
  if (ntiles) hipLaunchKernelGGL(ScanTileApplyKernel, dim3(ntiles), dim3(256), 0, stream, in, n, tile_tmp, out);
}

// ---- restart segments: bits and bytes of each ---------------------------------------------------------------------------------------------
__device__ inline void SegmentBlocks(const JpegScanDev& s, uint32_t g, uint32_t* first, uint32_t* end) {
  const uint64_t per = (uint64_t)s.restart * s.blocks_per_mcu, k = g - s.first_seg;
  const uint64_t a = s.restart ? k * per : 0, e = s.restart ? a + per : s.num_blocks;
  *first = s.first_block + (uint32_t)(a < s.num_blocks ? a : s.num_blocks);
  *end = s.first_block + (uint32_t)(e < s.num_blocks ? e : s.num_blocks);
}
__global__ __launch_bounds__(256) void JpegSegBytesKernel(JpegWritePlan p) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= p.num_segs) return;
  const JpegScanDev& s = FindScan<true>(p.scans, p.num_scans, g);
  uint32_t first, end;
  SegmentBlocks(s, g, &first, &end);
  const uint64_t nbits = p.bitpos[end] - p.bitpos[first];
  p.seg_bits[g] = (uint32_t)nbits;                      // (the host keeps scans whose worst case does not fit 32 bits off this path)
  p.seg_bytes[g] = (uint32_t)((nbits + 7) >> 3);
}

// ---- pass 2: the bits ------------------------------------------------------------------------------------------------------------------
// `n` bits (1..32, n + (pos & 31) <= 63) MSB-first at bit `pos` of a byte stream kept in 32-bit words
__device__ inline void PutBits(uint32_t* words, uint64_t pos, uint32_t v, uint32_t n, uint64_t nwords) {
  const uint64_t w = pos >> 5;
  const uint64_t x = (uint64_t)v << (64 - (uint32_t)(pos & 31) - n);
  const uint32_t hi = (uint32_t)(x >> 32), lo = (uint32_t)x;
  if (hi && w < nwords) atomicOr(&words[w], __builtin_bswap32(hi));
  if (lo && w + 1 < nwords) atomicOr(&words[w + 1], __builtin_bswap32(lo));
}
__global__ __launch_bounds__(256) void JpegPackKernel(JpegWritePlan p, uint32_t* __restrict__ raw, uint64_t raw_words) {
  const uint32_t b = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (b >= p.num_blocks) return;
  const JpegScanDev& s = FindScan<false>(p.scans, p.num_scans, b);
  if (*p.frames[s.frame].status != 0) return;
  const uint32_t block_bits = p.bits[b];
  if (block_bits == 0) return;
  const BlockRef r = LocateBlock(s, b);
  const LaneCode lc = BlockLaneCode(p, s, r, lane);
  const uint32_t n = lc.zrl_n * lc.zrl_len + lc.len;
  uint32_t incl = n;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += o; }
  if (n == 0 || incl > block_bits) return;               // (cannot happen: both passes count the same code; a store never leaves the block's own bits)
  uint64_t pos = p.seg_off[r.seg] * 8 + (p.bitpos[b] - p.bitpos[r.seg_first]) + (incl - n);
  if (pos + n > raw_words * 32) return;
  for (uint32_t k = 0; k < lc.zrl_n; k++) { PutBits(raw, pos, lc.zrl_code, lc.zrl_len, raw_words); pos += lc.zrl_len; }
  if (lc.len) PutBits(raw, pos, lc.bits, lc.len, raw_words);
}

// ---- byte stuffing ------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kStuffChunk = 1024;      // bytes of the raw buffer per workgroup: 256 threads x one 32-bit word
__device__ inline uint32_t CountFF(uint32_t w, uint32_t nbytes) {
  uint32_t n = 0;
  for (uint32_t k = 0; k < nbytes; k++) n += ((w >> (8 * k)) & 0xFF) == 0xFF;
  return n;
}
__global__ __launch_bounds__(256) void JpegCountFFKernel(const uint32_t* __restrict__ raw, uint64_t raw_bytes, uint32_t* __restrict__ ff_count) {
  __shared__ uint64_t lds[256];
  const uint64_t u = (uint64_t)blockIdx.x * kStuffChunk + threadIdx.x * 4;
  const uint32_t nb = u >= raw_bytes ? 0 : (uint32_t)(raw_bytes - u < 4 ? raw_bytes - u : 4);
  const uint32_t cnt = nb ? CountFF(raw[u >> 2], nb) : 0;
  uint64_t total;
  BlockExclusiveScan(cnt, lds, &total);
  if (threadIdx.x == 0) ff_count[blockIdx.x] = (uint32_t)total;
}
__global__ __launch_bounds__(256) void JpegStuffKernel(const uint32_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ ff_before, uint8_t* __restrict__ out,
                                                       uint64_t out_cap) {
  __shared__ uint64_t lds[256];
  const uint64_t u = (uint64_t)blockIdx.x * kStuffChunk + threadIdx.x * 4;
  const uint32_t nb = u >= raw_bytes ? 0 : (uint32_t)(raw_bytes - u < 4 ? raw_bytes - u : 4);
  const uint32_t w = nb ? raw[u >> 2] : 0;
  uint64_t total;
  uint64_t o = u + ff_before[blockIdx.x] + BlockExclusiveScan(nb ? CountFF(w, nb) : 0, lds, &total);
  for (uint32_t k = 0; k < nb; k++) {
    const uint8_t v = (uint8_t)(w >> (8 * k));
    if (o < out_cap) out[o] = v;
    o++;
    if (v == 0xFF) { if (o < out_cap) out[o] = 0; o++; }
  }
}
// one wavefront per restart segment: where its complete bytes start in the stuffed buffer, how many they became, and its last, incomplete byte
__device__ inline uint64_t FFBefore(const uint8_t* raw, const uint64_t* ff_before, uint64_t x, uint32_t lane) {
  const uint64_t chunk = x / kStuffChunk;
  uint32_t n = 0;
  for (uint64_t i = chunk * kStuffChunk + lane; i < x; i += 64) n += raw[i] == 0xFF;
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
  return ff_before[chunk] + n;
}
__global__ __launch_bounds__(256) void JpegSegRecordKernel(JpegWritePlan p, const uint8_t* __restrict__ raw, uint64_t raw_bytes, const uint64_t* __restrict__ ff_before,
                                                           JpegSegDev* __restrict__ recs) {
  const uint32_t g = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (g >= p.num_segs) return;
  const uint64_t u0 = p.seg_off[g], full = p.seg_bits[g] >> 3;
  const uint32_t tail = p.seg_bits[g] & 7;
  if (u0 + full + (tail ? 1 : 0) > raw_bytes) { if (lane == 0) recs[g] = JpegSegDev{0, 0, 0}; return; }
  const uint64_t f0 = FFBefore(raw, ff_before, u0, lane), f1 = FFBefore(raw, ff_before, u0 + full, lane);
  if (lane == 0) recs[g] = JpegSegDev{u0 + f0, (uint32_t)(full + (f1 - f0)), tail ? ((uint32_t)raw[u0 + full] << 8) | tail : 0};
}

}  // namespace

void LaunchJpegSizes(const JpegWritePlan& p, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!p.num_blocks || !p.num_segs) return;
  hipLaunchKernelGGL(JpegBlockBitsKernel, dim3((p.num_blocks + 3) / 4), dim3(256), 0, stream, p);
  ScanU32(p.bits, p.num_blocks, p.bitpos, p.tile_tmp, stream);
  hipLaunchKernelGGL(JpegSegBytesKernel, dim3((p.num_segs + 255) / 256), dim3(256), 0, stream, p);
  ScanU32(p.seg_bytes, p.num_segs, p.seg_off, p.tile_tmp, stream);
}

void LaunchJpegPack(const JpegWritePlan& p, const JpegPackBuffers& o, void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (!p.num_blocks || !p.num_segs) return;
  const uint64_t raw_words = (o.raw_bytes + 3) / 4;      // (the buffer is allocated, and zeroed, up to the next word)
  const uint32_t chunks = (uint32_t)((o.raw_bytes + kStuffChunk - 1) / kStuffChunk);
  (void)hipMemsetAsync(o.raw, 0, raw_words * 4, stream);
  hipLaunchKernelGGL(JpegPackKernel, dim3((p.num_blocks + 3) / 4), dim3(256), 0, stream, p, (uint32_t*)o.raw, raw_words);
  if (chunks) hipLaunchKernelGGL(JpegCountFFKernel, dim3(chunks), dim3(256), 0, stream, (const uint32_t*)o.raw, o.raw_bytes, o.ff_count);
  ScanU32(o.ff_count, chunks, o.ff_before, o.tile_tmp, stream);
  if (chunks) hipLaunchKernelGGL(JpegStuffKernel, dim3(chunks), dim3(256), 0, stream, (const uint32_t*)o.raw, o.raw_bytes, o.ff_before, o.stuffed, o.stuffed_cap);
  hipLaunchKernelGGL(JpegSegRecordKernel, dim3((p.num_segs + 3) / 4), dim3(256), 0, stream, p, o.raw, o.raw_bytes, o.ff_before, o.recs);
}

uint32_t JpegStuffChunkBytes() { return kStuffChunk; }

}  // namespace jxlhip
