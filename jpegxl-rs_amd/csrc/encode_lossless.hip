// jxl-hip: device side of the lossless batch encoder (encode_lossless.cc is the host half; the stream shape is described there).
// One workgroup of 256 threads per section that carries samples (a whole single-group image, or one 256 x 256 group); thread x owns column x of the group and walks
// down its rows, keeping the row above in registers.  Neighbours in a lossless stream are source samples, so every token is a pure function of the input and the three
// passes simply derive it again (WalkSection / MakeToken are the one definition):
//   pass 1  EncTokeniseKernel     RCT, group-local W / N / NW, tree walk, residual, hybrid-uint token; counts in an LDS histogram, one global add per used
//                                 (context, token); a sample above 2^bits - 1 flags its image (and is clamped, so that every later index stays in range)
//   (host)  length-limited prefix codes from the histograms, uploaded as one (bit-reversed code | length << 16) table per image
//   pass 2  EncCountKernel        bits per (channel, row) of the section, exclusive scan in LDS over the section's rows in stream order (channel-major), bytes per section;
//           EncSectionScanKernel  exclusive scan of the section bytes: every section's place in the compact buffer
//   pass 3  EncPackKernel         a row's codes + extra bits, LSB-first, at wave- and workgroup-prefix-summed positions: assembled in LDS words, interior words stored,
//                                 the first and last word of a row (shared with its neighbours) ORed into the zeroed buffer
// The pack pass checks every token against its section's byte size before it touches the LDS row, and every word against the buffer, whatever pass 2 said.
#include "encode_lossless.h"
#include <hip/hip_runtime.h>

namespace jxlhip {

namespace {

struct Px { int32_t v[kEncMaxChannels]; };
struct Tok { uint32_t ctx, tok, nbits, extra; };

// the (channel-transformed) samples of one pixel; channels the image does not have are 0
__device__ inline Px LoadPx(const EncImageDev& im, uint32_t x, uint32_t y, uint32_t* over) {
  Px p;
  const uint8_t* s = im.src + (uint64_t)y * im.pitch + (uint64_t)x * im.nch * im.bytes_per_sample;
#pragma unroll
  for (uint32_t c = 0; c < kEncMaxChannels; c++) {
    uint32_t v = 0;
    if (c < im.nch) {
      v = im.bytes_per_sample == 1 ? (uint32_t)s[c] : (uint32_t)s[2 * c] | ((uint32_t)s[2 * c + 1] << 8);
      if (v > im.max_value) { *over = 1; v = im.max_value; }
    }
    p.v[c] = (int32_t)v;
  }
  if (im.rct) {                                   // RCT type 6, forward: (R, G, B) -> (Y, Co, Cg)
    const int32_t co = p.v[0] - p.v[2], tmp = p.v[2] + (co >> 1), cg = p.v[1] - tmp;
    p.v[0] = tmp + (cg >> 1); p.v[1] = co; p.v[2] = cg;
  }
  return p;
}

// bucket of property 9 under the fixed cut-offs (the number of cut-offs below it), clamped-gradient residual, PackSigned, hybrid-uint (4, 2, 0)
__device__ inline Tok MakeToken(int32_t v, int32_t W, int32_t N, int32_t NW, uint32_t* bucket) {
  const int32_t g = W + N - NW;
  constexpr int32_t cuts[kEncNumCuts] = JXL_ENC_CUTS;
  uint32_t b = 0;
#pragma unroll
  for (int i = 0; i < kEncNumCuts; i++) b += g > cuts[i];
  *bucket = b;
  const int32_t m = N < W ? N : W, M = N < W ? W : N;
  const int32_t guess = NW < m ? M : (NW > M ? m : g);
  const int32_t r = v - guess;
  const uint32_t packed = r >= 0 ? (uint32_t)r * 2u : (uint32_t)(-r) * 2u - 1u;
  Tok t;
  t.ctx = 0;
  if (packed < 16) { t.tok = packed; t.nbits = 0; t.extra = 0; return t; }
  const uint32_t n = 31u - (uint32_t)__builtin_clz(packed), mant = packed - (1u << n);
  t.tok = 16u + ((n - 4u) << 2) + (mant >> (n - 2u));
  if (t.tok >= kEncAlphabet) t.tok = kEncAlphabet - 1;      // (cannot happen: samples are clamped to 16 bits)
  t.nbits = n - 2u;
  t.extra = mant & ((1u << t.nbits) - 1u);
  return t;
}

// Calls f(y, tokens of the thread's sample in every channel, active) for every row of the section, in uniform control flow (f may synchronise).  Returns whether the
// thread saw a sample above the image's range.
template <class F>
__device__ inline uint32_t WalkSection(const EncImageDev& im, const EncSectionDev& sec, const uint8_t* leaf_ctx, F&& f) {
  const uint32_t x = threadIdx.x;
  const bool active = x < sec.w && sec.x0 + x < im.xsize;
  uint32_t over = 0, ignored = 0;
  Px up = {}, upleft = {};
  for (uint32_t y = 0; y < sec.h; y++) {
    Px cur = {}, left = {};
    const bool row_ok = active && sec.y0 + y < im.ysize;
    if (row_ok) {
      cur = LoadPx(im, sec.x0 + x, sec.y0 + y, &over);
      if (x) left = LoadPx(im, sec.x0 + x - 1, sec.y0 + y, &ignored);      // (its owner reports it)
    }
    Tok t[kEncMaxChannels];
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) {
      const int32_t W = x ? left.v[c] : (y ? up.v[c] : 0), N = y ? up.v[c] : W, NW = (x && y) ? upleft.v[c] : W;
      uint32_t bucket;
      t[c] = MakeToken(cur.v[c], W, N, NW, &bucket);
      t[c].ctx = leaf_ctx[c * kEncLeaves + bucket];
    }
    f(y, t, row_ok);
    up = cur; upleft = left;
  }
  return over;
}

__device__ inline void LoadLeafCtx(const EncPlan& p, const EncImageDev& im, uint8_t* leaf_ctx) {
  if (threadIdx.x < kEncNumCtx) leaf_ctx[threadIdx.x] = p.leaf_ctx[(im.nch - 1) * kEncNumCtx + threadIdx.x];
}

__global__ __launch_bounds__(256) void EncTokeniseKernel(EncPlan p) {
  __shared__ uint32_t hist[kEncHistSize];
  __shared__ uint8_t leaf_ctx[kEncNumCtx];
  const EncSectionDev sec = p.sections[blockIdx.x];
  const EncImageDev im = p.images[sec.image];
  for (uint32_t i = threadIdx.x; i < kEncHistSize; i += 256) hist[i] = 0;
  LoadLeafCtx(p, im, leaf_ctx);
  __syncthreads();
  const uint32_t over = WalkSection(im, sec, leaf_ctx, [&](uint32_t, const Tok* t, bool active) {
    if (!active) return;
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) if (c < im.nch) atomicAdd(&hist[t[c].ctx * kEncAlphabet + t[c].tok], 1u);
  });
  __syncthreads();
  uint32_t* global_hist = p.hist + (size_t)sec.image * kEncHistSize;
  for (uint32_t i = threadIdx.x; i < kEncHistSize; i += 256) if (hist[i]) atomicAdd(&global_hist[i], hist[i]);
  if (over) atomicOr(&p.flags[sec.image], kEncFlagRange);
}

__global__ __launch_bounds__(256) void EncCountKernel(EncPlan p) {
  __shared__ uint32_t codes[kEncHistSize];
  __shared__ uint32_t rows[kEncMaxChannels * kEncGroupDim];
  __shared__ uint32_t wave_sum[4];
  __shared__ uint8_t leaf_ctx[kEncNumCtx];
  const EncSectionDev sec = p.sections[blockIdx.x];
  const EncImageDev im = p.images[sec.image];
  const uint32_t* image_codes = p.codes + (size_t)sec.image * kEncHistSize;
  for (uint32_t i = threadIdx.x; i < kEncHistSize; i += 256) codes[i] = image_codes[i];
  for (uint32_t i = threadIdx.x; i < kEncMaxChannels * kEncGroupDim; i += 256) rows[i] = 0;
  LoadLeafCtx(p, im, leaf_ctx);
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = sec.h < kEncGroupDim ? sec.h : kEncGroupDim;
  WalkSection(im, sec, leaf_ctx, [&](uint32_t y, const Tok* t, bool active) {
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) {
      if (c >= im.nch) continue;                           // (uniform)
      uint32_t bits = active ? (codes[t[c].ctx * kEncAlphabet + t[c].tok] >> 16) + t[c].nbits : 0;
      for (int d = 32; d >= 1; d >>= 1) bits += __shfl_xor(bits, d, 64);
      if (lane == 0 && bits && y < h) atomicAdd(&rows[c * h + y], bits);
    }
  });
  __syncthreads();
  // exclusive scan over the section's nch * h rows in stream order; a thread owns four consecutive rows
  const uint32_t n = im.nch * h;
  uint32_t v[4], s = 0;
  for (uint32_t k = 0; k < 4; k++) { const uint32_t i = threadIdx.x * 4 + k; v[k] = i < n ? rows[i] : 0; s += v[k]; }
  uint32_t incl = s;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += o; }
  if (lane == 63) wave_sum[wave] = incl;
  __syncthreads();
  uint32_t pos = incl - s, total = 0;
  for (uint32_t w = 0; w < 4; w++) { if (w < wave) pos += wave_sum[w]; total += wave_sum[w]; }
  for (uint32_t k = 0; k < 4; k++) { const uint32_t i = threadIdx.x * 4 + k; if (i < n) p.row_off[sec.row_base + i] = pos; pos += v[k]; }
  if (threadIdx.x == 0) p.sec_bytes[blockIdx.x] = (sec.lead_bits + total + 7) >> 3;
}

__global__ __launch_bounds__(256) void EncSectionScanKernel(EncPlan p) {
  __shared__ uint64_t lds[256];
  const uint32_t t = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < p.num_sections; base += 256) {
    const uint32_t i = base + t;
    const uint64_t v = i < p.num_sections ? p.sec_bytes[i] : 0;
    lds[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
      const uint64_t o = t >= d ? lds[t - d] : 0;
      __syncthreads();
      lds[t] += o;
      __syncthreads();
    }
    if (i < p.num_sections) p.sec_off[i] = carry + lds[t] - v;
    carry += lds[255];
    __syncthreads();
  }
  if (t == 0) p.sec_off[p.num_sections] = carry;
}

// `x` (the value shifted to its place in a pair of words) ORed into words w, w + 1 of the compact buffer
__device__ inline void OrIntoBuffer(const EncPlan& p, uint64_t w, uint64_t x) {
  if ((uint32_t)x && w < p.out_words) atomicOr(&p.out[w], (uint32_t)x);
  if ((uint32_t)(x >> 32) && w + 1 < p.out_words) atomicOr(&p.out[w + 1], (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(256) void EncPackKernel(EncPlan p) {
  __shared__ uint32_t codes[kEncHistSize];
  __shared__ uint32_t rowbuf[kEncMaxChannels][256];        // a row is at most 256 x (15 + 15) bits + 31 bits of word offset: 241 words
  __shared__ uint32_t wave_sum[kEncMaxChannels][4];
  __shared__ uint8_t leaf_ctx[kEncNumCtx];
  const EncSectionDev sec = p.sections[blockIdx.x];
  const EncImageDev im = p.images[sec.image];
  const uint32_t* image_codes = p.codes + (size_t)sec.image * kEncHistSize;
  for (uint32_t i = threadIdx.x; i < kEncHistSize; i += 256) codes[i] = image_codes[i];
  LoadLeafCtx(p, im, leaf_ctx);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = sec.h < kEncGroupDim ? sec.h : kEncGroupDim;
  const uint64_t sec_bit0 = p.sec_off[blockIdx.x] * 8, sec_bits = (uint64_t)p.sec_bytes[blockIdx.x] * 8;
  if (threadIdx.x == 0 && sec.lead_bits <= 8 && sec.lead_bits <= sec_bits)
    OrIntoBuffer(p, sec_bit0 >> 5, (uint64_t)(sec.lead_value & ((1u << sec.lead_bits) - 1u)) << (sec_bit0 & 31));
  uint32_t bad = 0;
  __syncthreads();
  WalkSection(im, sec, leaf_ctx, [&](uint32_t y, const Tok* t, bool active) {
    uint32_t len[kEncMaxChannels], excl[kEncMaxChannels];
    uint64_t bits[kEncMaxChannels];
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) {
      rowbuf[c][threadIdx.x] = 0;
      len[c] = 0; bits[c] = 0;
      if (active && c < im.nch) {
        const uint32_t code = codes[t[c].ctx * kEncAlphabet + t[c].tok], code_len = code >> 16;
        len[c] = code_len + t[c].nbits;
        bits[c] = (uint64_t)(code & 0xFFFFu) | ((uint64_t)t[c].extra << code_len);
      }
      uint32_t incl = len[c];
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl, d, 64); if ((int)lane >= d) incl += o; }
      excl[c] = incl - len[c];
      if (lane == 63) wave_sum[c][wave] = incl;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) {
      if (c >= im.nch || y >= h) continue;                 // (uniform)
      const uint64_t row_rel = (uint64_t)sec.lead_bits + p.row_off[sec.row_base + c * h + y];      // bits of the section before this row
      uint32_t before = excl[c];
      for (uint32_t w = 0; w < 4; w++) if (w < wave) before += wave_sum[c][w];
      if (len[c]) {
        const uint64_t local = ((sec_bit0 + row_rel) & 31) + before;                               // bit of the LDS row
        if (row_rel + before + len[c] > sec_bits || len[c] > 2 * kEncMaxCodeBits || (local + len[c] + 31) / 32 > 256) bad = 1;   // outside the section: never stored
        else {
          const uint64_t x = bits[c] << (local & 31);      // at most 30 + 31 bits
          atomicOr(&rowbuf[c][local >> 5], (uint32_t)x);
          if ((uint32_t)(x >> 32)) atomicOr(&rowbuf[c][(local >> 5) + 1], (uint32_t)(x >> 32));
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t c = 0; c < kEncMaxChannels; c++) {
      if (c >= im.nch || y >= h) continue;
      const uint32_t total = wave_sum[c][0] + wave_sum[c][1] + wave_sum[c][2] + wave_sum[c][3];
      const uint64_t start = sec_bit0 + sec.lead_bits + p.row_off[sec.row_base + c * h + y];
      const uint32_t nwords = total ? (uint32_t)(((start & 31) + total + 31) >> 5) : 0;
      if (threadIdx.x < nwords && nwords <= 256) {
        const uint32_t word = rowbuf[c][threadIdx.x];
        const uint64_t gw = (start >> 5) + threadIdx.x;
        if (word && gw < p.out_words) {
          if (threadIdx.x == 0 || threadIdx.x == nwords - 1) atomicOr(&p.out[gw], word);            // shared with the neighbouring rows
          else p.out[gw] = word;
        }
      }
    }
    __syncthreads();
  });
  if (bad) atomicOr(&p.flags[sec.image], kEncFlagPack);
}

}  // namespace

void EncLaunchTokenise(const EncPlan& p, void* stream) {
  if (p.num_sections) hipLaunchKernelGGL(EncTokeniseKernel, dim3(p.num_sections), dim3(256), 0, (hipStream_t)stream, p);
}
void EncLaunchCount(const EncPlan& p, void* stream) {
  if (p.num_sections) hipLaunchKernelGGL(EncCountKernel, dim3(p.num_sections), dim3(256), 0, (hipStream_t)stream, p);
  hipLaunchKernelGGL(EncSectionScanKernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
}
void EncLaunchPack(const EncPlan& p, void* stream) {
  if (p.num_sections) hipLaunchKernelGGL(EncPackKernel, dim3(p.num_sections), dim3(256), 0, (hipStream_t)stream, p);
}

}  // namespace jxlhip
