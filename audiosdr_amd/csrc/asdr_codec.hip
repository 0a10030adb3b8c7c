// asdr_codec.hip -- the audio codec's kernels (include/asdr_codec.h): delivered int16 rows as G.711 bytes or IMA ADPCM packet rows.
// A deployment that creates no codec launches nothing from this file.
//
// Form:
//  * Rows.  Output row i is channel c = index ? index[i] : i for i < min(*count, capacity_rows), read from input row c (the chain's
//    rows) or i (rows_compact: a resampler's rows behind the same index).  An entry outside 0 .. n_channels - 1 is skipped: nothing
//    is written for it and no state is touched.
//  * G.711 is fully parallel.  A lane takes one 16-byte piece (8 samples) and writes 8 bytes as two dwords; neighbouring lanes sit on
//    neighbouring pieces of one row (the row access rule of DESIGN.md 2), and rows shorter than a workgroup share one.  The
//    exponent is a find-first-bit (clz); no table, no LDS.  A row's bytes are padded with zeros to a multiple of 4, so every store
//    is a whole dword.
//  * ADPCM is a recurrence per channel: a lane owns a ROW, a wave (= a workgroup) 64 rows.  The rows come through LDS 64 samples at
//    a time: for the global loads the 8 lanes of a row sit on its 8 adjacent 16-byte pieces (eight rows per load instruction); in
//    LDS a row takes 33 words, odd, so the 64 lanes' reads of one offset fall into different banks.  The next chunk's loads are
//    issued before the current chunk's chain runs and land in registers meanwhile.  The chain is branch-free (selects for the three
//    comparisons, the index step computed, not looked up), reads T from LDS, packs 8 nibbles per dword and stores whole dwords:
//    the row's body is ceil(n / 8) dwords, its unused nibbles zero.  The state is read once, the header is written from it, and
//    the state is stored once at the end.
//  * Alignment.  A 16-byte aligned base with a stride that is a multiple of 8 samples loads every piece as 16 bytes, the one the row
//    ends in included (load_piece); any other geometry is read sample by sample, never past the row's last sample.
#include <hip/hip_runtime.h>

#include "asdr_codec_device.h"

namespace {

__device__ const uint16_t kStep[ASDR_CODEC_STEPS] = {ASDR_CODEC_STEP_TABLE};

__device__ inline uint32_t ulaw_byte(int x) {
  const int m = x >> 2;
  const int a = min(abs(m), 8158) + 33;                       // 33 .. 8191
  const int e = 26 - __builtin_clz((uint32_t)a);              // floor(log2 a) - 5
  return (uint32_t)(((e << 4) | ((a >> (e + 1)) & 15)) ^ (m < 0 ? 0x7F : 0xFF));
}

__device__ inline uint32_t alaw_byte(int x) {
  const int m = x >> 3;
  const int a = m < 0 ? -m - 1 : m;                           // 0 .. 4095
  const int e = max(27 - __builtin_clz((uint32_t)max(a, 1)), 0);
  const int q = (e < 2 ? a >> 1 : a >> e) & 15;
  return (uint32_t)(((e << 4) | q) ^ (m < 0 ? 0x55 : 0xD5));
}

// the rows of this call: grid_rows, cut to the device count in the index forms
__device__ inline int live_rows(const CodecArgs &a) {
  int rows = a.grid_rows;
  if (a.index) rows = min(rows, min(*a.count, a.capacity_rows));
  return max(rows, 0);                                        // a negative count delivers nothing
}

// one 16-byte piece of an input row, samples s .. s + 7 with s < n_samples.  What it holds past n_samples is never used: the G.711
// pass clears those bytes, the ADPCM chain stops before them.  In the aligned geometry it is one load even where the row ends inside
// it (an aligned 16-byte piece cannot cross a page); otherwise eight 2-byte loads, those past the row's end reading its last
// sample again, so none of them waits behind a bound check.
__device__ inline uint4 load_piece(const CodecArgs &a, int64_t in_row, int s) {
  const int16_t *src = a.rows + (in_row * a.row_stride + s);
  if (a.aligned) return *(const uint4 *)src;
  const int last = a.n_samples - 1 - s;
  uint32_t h[8];
#pragma unroll
  for (int j = 0; j < 8; j++) h[j] = (uint32_t)(uint16_t)src[min(j, last)];
  return make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
}

template <int KIND>
__device__ inline uint32_t g711_word(uint32_t w01, uint32_t w23) {
  const int x0 = (int)(int16_t)(w01 & 0xFFFFu), x1 = (int)w01 >> 16, x2 = (int)(int16_t)(w23 & 0xFFFFu), x3 = (int)w23 >> 16;
  if (KIND == ASDR_CODEC_ULAW) return ulaw_byte(x0) | (ulaw_byte(x1) << 8) | (ulaw_byte(x2) << 16) | (ulaw_byte(x3) << 24);
  return alaw_byte(x0) | (alaw_byte(x1) << 8) | (alaw_byte(x2) << 16) | (alaw_byte(x3) << 24);
}

// one sample through the encoder: returns the nibble, advances p and i4 = 4 i, the byte offset of T[i] (one shift less between a
// step and the next table read, which is the chain's critical path)
__device__ inline uint32_t adpcm_step(int x, int &p, int &i4, const uint32_t *T) {
  const int s = (int)*(const uint32_t *)((const char *)T + i4);
  int d = x - p;
  const bool neg = d < 0;
  d = abs(d);
  const int h = s >> 1, q = s >> 2;
  const bool c4 = d >= s;
  d -= c4 ? s : 0;
  const bool c2 = d >= h;
  d -= c2 ? h : 0;
  const bool c1 = d >= q;
  const int v = (s >> 3) + (c4 ? s : 0) + (c2 ? h : 0) + (c1 ? q : 0);
  const int c = (c4 ? 4 : 0) | (c2 ? 2 : 0) | (c1 ? 1 : 0);
  p = min(max(neg ? p - v : p + v, -32768), 32767);
  i4 = min(max(i4 + (c4 ? 8 * (c - 3) : -4), 0), 4 * ASDR_CODEC_MAX_STEP_INDEX);   // i += c < 4 ? -1 : 2 (c - 3)
  return (uint32_t)c | (neg ? 8u : 0u);
}

// 8 samples (four staged words) into one dword of nibbles, the first sample in the lowest
__device__ inline uint32_t adpcm_dword(const uint32_t *x, int &p, int &i4, const uint32_t *T) {
  uint32_t nib = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t w = x[k];
    nib |= adpcm_step((int)(int16_t)(w & 0xFFFFu), p, i4, T) << (8 * k);
    nib |= adpcm_step((int)w >> 16, p, i4, T) << (8 * k + 4);
  }
  return nib;
}

}  // namespace

// grid ceil(rows * pieces / 256): lane w takes piece w % pieces of row w / pieces
template <int KIND>
__global__ __launch_bounds__(ASDR_CODEC_THREADS) void asdr_codec_g711_kernel(CodecArgs a) {
  const uint32_t w = blockIdx.x * (uint32_t)ASDR_CODEC_THREADS + threadIdx.x;   // the host keeps rows * pieces below 2^32
  const uint32_t row = w / (uint32_t)a.pieces, p = w - row * (uint32_t)a.pieces;
  if (row >= (uint32_t)live_rows(a)) return;
  const int c = a.index ? a.index[row] : (int)row;
  if ((uint32_t)c >= (uint32_t)a.n_channels) return;
  const int64_t in_row = (a.index && !a.rows_compact) ? c : (int64_t)row;
  const int s = 8 * (int)p;
  const uint4 v = load_piece(a, in_row, s);
  uint32_t *o = (uint32_t *)(a.out + ((int64_t)row * a.out_stride + s));
  uint32_t b0 = g711_word<KIND>(v.x, v.y), b1 = g711_word<KIND>(v.z, v.w);
  const int tail = a.n_samples - s;                           // >= 1: the row's samples from s on; the bytes past them are 0
  if (tail < 4) b0 &= 0xFFFFFFFFu >> (8 * (4 - tail));
  if (tail < 8) b1 = tail > 4 ? b1 & (0xFFFFFFFFu >> (8 * (8 - tail))) : 0u;
  o[0] = b0;
  if (tail > 4) o[1] = b1;                                    // the row ends at the next multiple of 4 bytes
}

// grid ceil(rows / 64), 64 lanes: lane l owns row 64 blockIdx.x + l
__global__ __launch_bounds__(ASDR_CODEC_ROWS) void asdr_codec_adpcm_kernel(CodecArgs a) {
  __shared__ uint32_t lds[96 + ASDR_CODEC_ROWS + ASDR_CODEC_ROWS * ASDR_CODEC_ROW_WORDS];
  uint32_t *T = lds;                                          // [89]
  int32_t *srow = (int32_t *)(lds + 96);                      // [64]: the rows' input rows, -1 for none
  uint32_t *win = lds + 96 + ASDR_CODEC_ROWS;                 // [64][33]
  const int lane = threadIdx.x;
  const int row0 = blockIdx.x * ASDR_CODEC_ROWS;
  const int rows = live_rows(a);
  if (row0 >= rows) return;                                   // the whole wave
  const int row = row0 + lane;
  int c = -1;
  if (row < rows) {
    c = a.index ? a.index[row] : row;
    if ((uint32_t)c >= (uint32_t)a.n_channels) c = -1;
  }
  const bool active = c >= 0;
  srow[lane] = !active ? -1 : (a.index && !a.rows_compact) ? c : row;
  for (int k = lane; k < ASDR_CODEC_STEPS; k += ASDR_CODEC_ROWS) T[k] = kStep[k];
  int p = 0, i4 = 0;                                          // i4 = 4 i
  uint32_t *o = (uint32_t *)(a.out + (int64_t)row * a.out_stride);
  if (active) {
    const uint32_t st = *(const uint32_t *)(a.state + c);     // predictor | step_index << 16 | reserved << 24
    p = (int)(int16_t)(st & 0xFFFFu);
    i4 = 4 * min((int)((st >> 16) & 0xFFu), ASDR_CODEC_MAX_STEP_INDEX);
    o[0] = st & 0x00FFFFFFu;                                  // the header: the state before the row's first sample
  }
  o += 1;
  __syncthreads();

  // staging: in pass t the lane takes piece (lane & 7) of row 8 t + (lane >> 3)
  const int piece = lane & 7, sub = lane >> 3;
  int in_rows[8];
#pragma unroll
  for (int t = 0; t < 8; t++) in_rows[t] = max(srow[8 * t + sub], 0);   // a row without a channel stages row 0: readable, and never used
  const int last_piece = (a.n_samples - 1) & ~7;
  uint4 v[8];
  auto request = [&](int s0) {                                // unconditional loads: all eight are in flight together
    const int s = min(s0 + 8 * piece, last_piece);            // a piece past the row's end stages the last one again, unused as well
    if (a.aligned) {                                          // decided once, outside the eight loads
#pragma unroll
      for (int t = 0; t < 8; t++) v[t] = *(const uint4 *)(a.rows + ((int64_t)in_rows[t] * a.row_stride + s));
    } else {
#pragma unroll
      for (int t = 0; t < 8; t++) {
        v[t] = load_piece(a, in_rows[t], s);
        __builtin_amdgcn_sched_barrier(0);                    // a piece's eight loads at a time: 64 in flight cost 64 registers
      }
    }
  };
  request(0);
  const uint32_t *x = win + lane * ASDR_CODEC_ROW_WORDS;
  for (int s0 = 0; s0 < a.n_samples; s0 += ASDR_CODEC_CHUNK) {
#pragma unroll
    for (int t = 0; t < 8; t++) {
      uint32_t *d = win + (8 * t + sub) * ASDR_CODEC_ROW_WORDS + 4 * piece;
      d[0] = v[t].x; d[1] = v[t].y; d[2] = v[t].z; d[3] = v[t].w;
    }
    __syncthreads();
    if (s0 + ASDR_CODEC_CHUNK < a.n_samples) request(s0 + ASDR_CODEC_CHUNK);   // in flight while the chain runs
    const int m = min(ASDR_CODEC_CHUNK, a.n_samples - s0);
    if (m == ASDR_CODEC_CHUNK) {
#pragma unroll 1
      for (int g = 0; g < 8; g += ASDR_CODEC_GROUP) {           // a group's dwords leave in one store where the compiler can merge them
        uint32_t nib[ASDR_CODEC_GROUP];
#pragma unroll
        for (int dw = 0; dw < ASDR_CODEC_GROUP; dw++) nib[dw] = adpcm_dword(x + 4 * (g + dw), p, i4, T);
        if (active) {
#pragma unroll
          for (int dw = 0; dw < ASDR_CODEC_GROUP; dw++) o[g + dw] = nib[dw];
        }
      }
    } else {                                                  // the row's last, partial chunk
      const int full = m >> 3, rem = m & 7;
      for (int dw = 0; dw < full; dw++) {
        const uint32_t nib = adpcm_dword(x + 4 * dw, p, i4, T);
        if (active) o[dw] = nib;
      }
      if (rem) {
        uint32_t nib = 0;
        for (int j = 0; j < rem; j++) {
          const uint32_t w = x[4 * full + (j >> 1)];
          nib |= adpcm_step((j & 1) ? (int)w >> 16 : (int)(int16_t)(w & 0xFFFFu), p, i4, T) << (4 * j);
        }
        if (active) o[full] = nib;
      }
    }
    o += ASDR_CODEC_CHUNK / 8;
    __syncthreads();                                          // every lane has read the window before it is overwritten
  }
  if (active) *(uint32_t *)(a.state + c) = ((uint32_t)p & 0xFFFFu) | ((uint32_t)(i4 >> 2) << 16);
}

extern "C" int asdr_launch_codec_g711(const CodecArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->grid_rows <= 0) return 0;
  const uint64_t items = (uint64_t)a->grid_rows * (uint32_t)a->pieces;
  if (items >= (1ULL << 32)) return -1;
  const dim3 grid((uint32_t)((items + ASDR_CODEC_THREADS - 1) / ASDR_CODEC_THREADS));
  if (a->kind == ASDR_CODEC_ULAW) hipLaunchKernelGGL(asdr_codec_g711_kernel<ASDR_CODEC_ULAW>, grid, dim3(ASDR_CODEC_THREADS), 0, stream, *a);
  else hipLaunchKernelGGL(asdr_codec_g711_kernel<ASDR_CODEC_ALAW>, grid, dim3(ASDR_CODEC_THREADS), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_codec_adpcm(const CodecArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->grid_rows <= 0) return 0;
  const dim3 grid(((uint32_t)a->grid_rows + ASDR_CODEC_ROWS - 1) / ASDR_CODEC_ROWS);
  hipLaunchKernelGGL(asdr_codec_adpcm_kernel, grid, dim3(ASDR_CODEC_ROWS), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
