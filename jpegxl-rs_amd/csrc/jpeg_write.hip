// jxl-hip: device-side writer of Huffman JPEG scans, sequential and progressive (batch JPEG reconstruction, decoder.cc Batch::ReconstructJpegs and its phases; reconstruction
// jobs of a pipeline).  Input: the int16 coefficient planes JpegGatherKernel (jpeg_pixels.hip) leaves in device memory (natural order, MCU-padded block grids).  Output: for every
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
//
// Progressive scans (JpegScanDev::kind; jpeg_recon.cc EncodeBlockProgressive / EncodeBlockRefinement / EobState are the reference).  The DC kinds are one piece in
// lane 0.  In the AC kinds a block's trailing zeros do not end the block but join an end-of-band run that the canonical writer carries from block to block, together
// with the correction bits of the blocks in the run.  Written per block that is: head (the bits the block emits itself) | EOBn, if the block heads a run | tail (the
// correction bits it buffers), concatenated in plain block order.  A flush point is a block with a non-empty head, a reset point or the first block of a restart
// segment; a span runs from one flush point to the next or to the segment's end; its joining blocks are the flush block, if it joins, and every block behind it; the
// run heads are the joining blocks number 0, 0x7FFF, 2 * 0x7FFF, ... with n = min(0x7FFF, joining blocks left).
//   pass 1   JpegBlockBitsKernel also leaves head / tail / joins (meta) and the flush flag of every block; ProgLaneCode is the shared definition of the four kinds
//   spans    ScanU32 over the flush flags numbers the spans, JpegSpanScatterKernel lists their first blocks, JpegRunHeadKernel adds the EOBn symbol to the bits of
//            every run head (RunHeadCode, shared with pass 2) and flags spans that hold more correction bits than the canonical writer buffers (65473)
//   pass 2   JpegPackKernel writes head, EOBn and tail of a block at its bit position
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

// ---- progressive kinds ------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kMetaHeadMask = 0xFFF, kMetaTailShift = 12, kMetaTailMask = 0xFF, kMetaJoins = 1u << 20;
constexpr uint32_t kEobRunMax = 0x7FFF, kTailBitsMax = (1u << 16) - 64 + 1;     // EobState::BufferEndOfBand flushes at either

__device__ inline uint32_t WaveExclusiveSum(uint32_t v, uint32_t lane, uint32_t* total) {
  uint32_t incl = v;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += o; }
  *total = __shfl(incl, 63, 64);
  return incl - v;
}
__device__ inline uint64_t BitsBelow(uint32_t k) { return (1ull << k) - 1ull; }               // bits 0 .. k - 1, k <= 63
__device__ inline uint64_t BitsUpTo(uint32_t k) { return (2ull << k) - 1ull; }                // bits 0 .. k, k <= 63

// What lane `lane` (zigzag position) places in its block of a progressive scan.  In the head: piece A at a_off; rep_n ZRL codes and piece B from b_off on; one
// correction bit at corr_off of the head or of the tail.  head / tail / joins are the block's (the same in every lane); err as in LaneCode.
//   first DC pass   A = code of the difference of the shifted DC values (category >= 13 is the error)          DC refinement   A = bit Al of c0
//   first AC pass   ZRLs and B = symbol + magnitude bits of |c| >> Al, the zero run counted inside the band; no end-of-block symbol
//   AC refinement   a coefficient that becomes non-zero (|c| >> Al == 1) is a symbol (r << 4) + 1 and its sign, r = z & 15 with z the zeros since the previous such
//                   coefficient; one that already was non-zero has one correction bit.  At a non-zero position up to the last new coefficient the writer has emitted
//                   z >> 4 ZRLs since the previous symbol, so the position emits the difference to the non-zero position in front of it.  The correction bits ride
//                   behind the first code emitted after them; those behind the last new coefficient are the tail.  So an emitting position ("event") writes
//                   A (its first code) | the correction bits between the previous event and itself | B (further ZRLs, the symbol if a ZRL came first).
struct ProgLane { uint32_t a_bits, a_len, a_off, rep_n, rep_code, rep_len, b_bits, b_len, b_off, corr_len, corr_bit, corr_off, corr_in_tail, head, tail, joins, err; };
__device__ inline ProgLane ProgLaneCode(const JpegWritePlan& p, const JpegScanDev& s, const BlockRef& r, uint32_t lane) {
  ProgLane o;
  memset(&o, 0, sizeof(o));
  const int c = p.coef[(size_t)r.blk * 64 + kJpegNatural[lane]];
  if (s.kind == kJpegDcFirst || s.kind == kJpegDcRefine) {
    const int pred = r.has_pred ? (int)p.coef[(size_t)r.pred * 64] : 0;
    if (lane == 0) {
      if (s.kind == kJpegDcRefine) { o.a_bits = (uint32_t)(c >> s.al) & 1u; o.a_len = 1; }
      else {
        int temp = (c >> s.al) - (pred >> s.al), temp2 = temp;
        if (temp < 0) { temp = -temp; temp2--; }
        const uint32_t nbits = temp ? 32 - __builtin_clz((uint32_t)temp) : 0;
        const JpegHuffDev& dct = p.tables[r.dc];
        if (nbits >= 13) o.err = 1;
        else if (dct.depth[nbits] > 16) o.err = 4;
        else {
          const uint32_t d = dct.depth[nbits];
          o.a_bits = (((uint32_t)dct.code[nbits] & ((1u << d) - 1u)) << nbits) | ((uint32_t)temp2 & ((1u << nbits) - 1u));
          o.a_len = d + nbits;
        }
      }
    }
    o.head = __shfl(o.a_len, 0, 64);
    return o;
  }
  const JpegHuffDev& act = p.tables[r.ac];
  const bool in_band = lane >= s.ss && lane <= s.se;
  const uint32_t a = in_band ? (uint32_t)(c < 0 ? -c : c) >> s.al : 0;
  const uint64_t low = BitsBelow(lane);
  if (s.kind == kJpegAcFirst) {
    const uint64_t mask = __ballot(a != 0);
    if (a) {
      const uint32_t nbits = 32 - __builtin_clz(a);
      const uint64_t below = mask & low;
      const uint32_t prev = below ? 63 - __builtin_clzll(below) : s.ss - 1u, run = lane - prev - 1;
      const uint32_t sym = ((run & 15) << 4) | (nbits & 15), d = act.depth[sym];
      o.rep_n = run >> 4;
      if (o.rep_n) { o.rep_len = act.depth[0xF0]; o.rep_code = act.code[0xF0] & ((1u << (o.rep_len & 31)) - 1u); }
      if (nbits >= 16) { o.rep_n = o.rep_len = 0; o.err = 2; }
      else if (d > 16 || o.rep_len > 16) { o.rep_n = o.rep_len = 0; o.err = 4; }
      else {
        const uint32_t temp2 = c < 0 ? ~a : a;
        o.b_bits = (((uint32_t)act.code[sym] & ((1u << d) - 1u)) << nbits) | (temp2 & ((1u << nbits) - 1u));
        o.b_len = d + nbits;
      }
    }
    o.b_off = WaveExclusiveSum(o.rep_n * o.rep_len + o.b_len, lane, &o.head);
    o.joins = mask == 0 || 63u - (uint32_t)__builtin_clzll(mask) < s.se;
    return o;
  }
  // AC refinement
  const bool is_new = a == 1, is_old = a > 1;
  const uint64_t newm = __ballot(is_new), oldm = __ballot(is_old), nzm = newm | oldm;
  const uint64_t zerom = BitsUpTo(s.se) & ~BitsBelow(s.ss) & ~nzm;
  const uint32_t eob = newm ? 63 - __builtin_clzll(newm) : 0;
  if ((is_new || is_old) && lane <= eob) {
    const uint64_t lastnew = newm & low;
    const uint32_t ln = lastnew ? 63 - __builtin_clzll(lastnew) : s.ss - 1u;
    const uint64_t since = low & ~BitsUpTo(ln);                       // positions behind the previous new coefficient, in front of this one
    const uint32_t z = __builtin_popcountll(zerom & since);
    const uint64_t pn = nzm & since;
    const uint32_t zprev = pn ? __builtin_popcountll(zerom & since & BitsBelow(63 - __builtin_clzll(pn))) : 0;
    const uint32_t nz = (z >> 4) - (zprev >> 4);
    const uint32_t zl = act.depth[0xF0], zc = act.code[0xF0] & ((1u << (zl & 31)) - 1u);
    uint32_t piece = 0, plen = 0;
    if (is_new) {
      const uint32_t sym = ((z & 15) << 4) | 1, d = act.depth[sym];
      if (d > 16) o.err = 4;
      else { piece = (((uint32_t)act.code[sym] & ((1u << d) - 1u)) << 1) | (c < 0 ? 0u : 1u); plen = d + 1; }
    }
    if (nz && zl > 16) o.err = 4;
    if (!o.err) {
      if (nz) { o.a_bits = zc; o.a_len = zl; o.rep_n = nz - 1; o.rep_code = zc; o.rep_len = zl; o.b_bits = piece; o.b_len = plen; }
      else { o.a_bits = piece; o.a_len = plen; }
    }
  }
  uint32_t sum;
  const uint32_t ex = WaveExclusiveSum(o.a_len + o.rep_n * o.rep_len + o.b_len, lane, &sum);
  const uint64_t eventm = __ballot(o.a_len != 0), tailm = oldm & ~BitsUpTo(eob);
  o.head = sum + (newm ? (uint32_t)__builtin_popcountll(oldm & BitsBelow(eob)) : 0);
  o.tail = __builtin_popcountll(tailm);
  o.joins = newm == 0 || eob < s.se;
  const uint64_t pem = eventm & low;
  const uint32_t olds_below = __builtin_popcountll(oldm & low);
  o.a_off = ex + (pem ? (uint32_t)__builtin_popcountll(oldm & BitsBelow(63 - __builtin_clzll(pem))) : 0);
  o.b_off = ex + o.a_len + olds_below;
  const uint64_t later = eventm & ~BitsUpTo(lane);
  const uint32_t ne = later ? (uint32_t)__builtin_ctzll(later) : lane;
  const uint32_t ex_ne = __shfl(ex, ne, 64), a_ne = __shfl(o.a_len, ne, 64);
  if (is_old) {
    o.corr_len = 1; o.corr_bit = a & 1;
    if (newm && lane < eob) o.corr_off = ex_ne + a_ne + olds_below;
    else { o.corr_in_tail = 1; o.corr_off = __builtin_popcountll(tailm & low); }
  }
  return o;
}

__device__ inline bool IsResetPoint(const JpegWritePlan& p, const JpegScanDev& s, uint32_t b) {
  uint32_t lo = s.reset_first, hi = s.reset_first + s.reset_count;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; const uint32_t v = p.resets[mid]; if (v == b) return true; if (v < b) lo = mid + 1; else hi = mid; }
  return false;
}

// The EOBn symbol of block `b` of an AC progressive scan, if it heads an end-of-band run (len 0 otherwise).  From the span table: the block's span starts at the
// last flush point f <= b and ends at the next one or at the end of the restart segment.  with_tails (span pass only, where bitpos still holds the scan of
// head + tail): the run head of the span's first run also sums the span's correction bits — behind f every block of the span has an empty head — and reports 8
// when they exceed what the canonical writer buffers before it flushes on its own.
struct RunHead { uint32_t bits, len, err; };
__device__ inline RunHead RunHeadCode(const JpegWritePlan& p, const JpegScanDev& s, const BlockRef& r, uint32_t b, bool with_tails) {
  RunHead o = {0, 0, 0};
  const uint64_t incl = p.span_idx[b] + p.flush[b], nspans = p.span_idx[p.num_blocks];
  if (incl == 0 || incl > nspans) return o;
  const uint32_t f = p.span_first[incl - 1];
  const uint64_t per = s.restart ? (uint64_t)s.restart * s.blocks_per_mcu : s.num_blocks;
  const uint64_t scan_end = (uint64_t)s.first_block + s.num_blocks, seg_end = r.seg_first + per < scan_end ? r.seg_first + per : scan_end;
  uint64_t e = incl < nspans ? p.span_first[incl] : p.num_blocks;
  if (e > seg_end) e = seg_end;
  if (f > b || f < r.seg_first || e <= b) return o;        // (cannot happen: a segment's first block is a flush point)
  const uint32_t mf = p.meta[f];
  const uint32_t first = (mf & kMetaJoins) ? f : f + 1;
  if (b < first || (b - first) % kEobRunMax) return o;
  const uint32_t left = (uint32_t)(e - b), n = left < kEobRunMax ? left : kEobRunMax;
  const uint32_t nbits = 31 - __builtin_clz(n);
  const JpegHuffDev& act = p.tables[r.ac];
  const uint32_t d = act.depth[nbits << 4];
  if (d > 16) { o.err = 4; return o; }
  o.bits = (((uint32_t)act.code[nbits << 4] & ((1u << d) - 1u)) << nbits) | (n & ((1u << nbits) - 1u));
  o.len = d + nbits;
  if (with_tails && b == first && p.bitpos[e] - p.bitpos[f] - (mf & kMetaHeadMask) > kTailBitsMax) o.err = 8;
  return o;
}

// ---- pass 1: bits per block ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void JpegBlockBitsKernel(JpegWritePlan p) {
  const uint32_t b = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (b >= p.num_blocks) return;
  const JpegScanDev& s = FindScan<false>(p.scans, p.num_scans, b);
  if (p.has_spans && lane == 0) { p.meta[b] = 0; p.flush[b] = 0; }
  if (*p.frames[s.frame].status != 0) { if (lane == 0) p.bits[b] = 0; return; }      // (a frame whose entropy stages failed has no coefficients)
  const BlockRef r = LocateBlock(s, b);
  if (s.kind != kJpegSequential) {
    const ProgLane pl = ProgLaneCode(p, s, r, lane);
    uint32_t err = pl.err;
    for (int d = 32; d >= 1; d >>= 1) err |= __shfl_xor(err, d, 64);
    if (lane == 0) {
      p.bits[b] = pl.head + pl.tail;
      p.meta[b] = (pl.head & kMetaHeadMask) | ((pl.tail & kMetaTailMask) << kMetaTailShift) | (pl.joins ? kMetaJoins : 0);
      if (s.kind >= kJpegAcFirst) p.flush[b] = pl.head != 0 || b == r.seg_first || IsResetPoint(p, s, b);
      if (err) atomicOr(&p.flags[s.image], err);
    }
    return;
  }
  const LaneCode lc = BlockLaneCode(p, s, r, lane);
  uint32_t n = lc.zrl_n * lc.zrl_len + lc.len, err = lc.err;
  for (int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d, 64); err |= __shfl_xor(err, d, 64); }
  if (lane == 0) {
    p.bits[b] = n;
    if (err) atomicOr(&p.flags[s.image], err);
  }
}

// ---- spans of the AC progressive kinds: first blocks, then the EOBn symbols of the run heads -------------------------------------------------
__global__ __launch_bounds__(256) void JpegSpanScatterKernel(JpegWritePlan p) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.num_blocks || !p.flush[b]) return;
  const uint64_t k = p.span_idx[b];
  if (k < p.num_blocks) p.span_first[k] = b;
}
__global__ __launch_bounds__(256) void JpegRunHeadKernel(JpegWritePlan p) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= p.num_blocks) return;
  const JpegScanDev& s = FindScan<false>(p.scans, p.num_scans, b);
  if (s.kind < kJpegAcFirst || *p.frames[s.frame].status != 0) return;
  const RunHead h = RunHeadCode(p, s, LocateBlock(s, b), b, true);
  if (h.len) p.bits[b] += h.len;
  if (h.err) atomicOr(&p.flags[s.image], h.err);
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
  if (s.kind != kJpegSequential) {
    const ProgLane pl = ProgLaneCode(p, s, r, lane);
    const uint32_t meta = p.meta[b], head = meta & kMetaHeadMask, tail = (meta >> kMetaTailShift) & kMetaTailMask;
    // (cannot happen: both passes count the same code) head | EOBn | tail are the block's own bits, and every store below stays inside its part
    if (pl.head != head || pl.tail != tail || head + tail > block_bits) return;
    const uint32_t eob_len = block_bits - head - tail;
    const uint64_t base = p.seg_off[r.seg] * 8 + (p.bitpos[b] - p.bitpos[r.seg_first]);
    if (base + block_bits > raw_words * 32) return;
    if (pl.a_len && pl.a_off + pl.a_len <= head) PutBits(raw, base + pl.a_off, pl.a_bits, pl.a_len, raw_words);
    if (pl.b_off + pl.rep_n * pl.rep_len + pl.b_len <= head) {
      uint64_t pos = base + pl.b_off;
      for (uint32_t k = 0; k < pl.rep_n; k++) { PutBits(raw, pos, pl.rep_code, pl.rep_len, raw_words); pos += pl.rep_len; }
      if (pl.b_len) PutBits(raw, pos, pl.b_bits, pl.b_len, raw_words);
    }
    if (pl.corr_len && pl.corr_bit) {
      if (!pl.corr_in_tail) { if (pl.corr_off < head) PutBits(raw, base + pl.corr_off, 1, 1, raw_words); }
      else if (pl.corr_off < tail) PutBits(raw, base + head + eob_len + pl.corr_off, 1, 1, raw_words);
    }
    if (lane == 0 && eob_len && s.kind >= kJpegAcFirst) {
      const RunHead h = RunHeadCode(p, s, r, b, false);
      if (h.len == eob_len) PutBits(raw, base + head, h.bits, h.len, raw_words);
    }
    return;
  }
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
  if (p.has_spans) {
    ScanU32(p.bits, p.num_blocks, p.bitpos, p.tile_tmp, stream);          // head + tail: the span pass takes a span's correction bits from it
    ScanU32(p.flush, p.num_blocks, p.span_idx, p.tile_tmp, stream);
    hipLaunchKernelGGL(JpegSpanScatterKernel, dim3((p.num_blocks + 255) / 256), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(JpegRunHeadKernel, dim3((p.num_blocks + 255) / 256), dim3(256), 0, stream, p);
  }
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
