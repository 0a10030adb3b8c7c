// asdr_tone.hip -- the tone squelch's kernel (include/asdr_tone.h): CTCSS decode, tone squelch and a sub-audible high-pass on the int16
// audio rows the FM demodulator writes.  A deployment that creates no tone squelch launches nothing from this file.
//
// Form.  A workgroup of four waves owns ASDR_TONE_ROWS = 16 channels and walks their rows one 128-sample block at a
// time.  The three natures of the work have a mapping each:
//  * Staging: a lane takes one 16-byte piece (8 samples) of a row, the 16 lanes of a row its 16 pieces, the workgroup 16 rows.  A row
//    lives in LDS as a ring of two blocks (128 words + 1, odd): block b goes to half b & 1, so the 45 samples before it (the other
//    half's tail; hist of the record before the first block) are in place without a move.  The next block's load is issued before
//    the current block's work.
//  * Decimator (step 1), lanes across outputs: 128 lanes, one d_k each, 23 word reads and 46 multiply-adds in int32.
//  * Correlation (step 2), lanes across the 64 table slots: a wave takes four channels in turn, their accumulators in registers.
//    A block's eight d are wave-uniform LDS reads; the cosine table sits in 4 KB of LDS as packed int16 pairs (C[j], C[j - 256]), one
//    read per sample and tone.  At a window's end the wave reduces the 64 powers to (best, P_best, other) by butterflies and leaves
//    them in LDS for the channel's owner.
//  * Recurrence (steps 3 to 5), a lane of wave 0 per channel: the biquad cascade on the staged row, the mute, and the window's
//    verdict.  The 16 lanes' reads of one offset fall into different banks (both pitches are odd).
//  * Output: the lane that staged a piece reads the filtered piece back and stores 16 bytes.
//  * State: read once before the first block and written once behind the last, with 8- and 16-byte accesses.
// Rows past n_channels in the last workgroup read channel n_channels - 1 again and write nothing.
#include <hip/hip_runtime.h>

#include "asdr_tone_device.h"

namespace {

struct CicTaps { int h[46]; };
constexpr CicTaps cic_taps() {                                // the coefficients of (1 + z + ... + z^15)^3
  CicTaps t{};
  for (int i = 0; i < 16; i++)
    for (int j = 0; j < 16; j++)
      for (int k = 0; k < 16; k++) t.h[i + j + k]++;
  return t;
}
constexpr CicTaps kCic = cic_taps();

__device__ inline int clamp16(int x) { return min(max(x, -32768), 32767); }
__device__ inline int lo16(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ inline int hi16(uint32_t w) { return (int)w >> 16; }
__device__ inline uint64_t sq(int x) { return (uint64_t)((int64_t)x * x); }

// step 3 of one sample
__device__ inline int tone_highpass(int x, int sections, const int32_t (&coef)[ASDR_TONE_MAX_SECTIONS][5], int (&hs)[ASDR_TONE_MAX_SECTIONS][4]) {
  int u = x * 256;
#pragma unroll
  for (int s = 0; s < ASDR_TONE_MAX_SECTIONS; s++) {
    if (s < sections) {                                       // the same in every lane
      const uint64_t acc = (uint64_t)((int64_t)coef[s][0] * u) + (uint64_t)((int64_t)coef[s][1] * hs[s][0]) + (uint64_t)((int64_t)coef[s][2] * hs[s][1]) -
                           (uint64_t)((int64_t)coef[s][3] * hs[s][2]) - (uint64_t)((int64_t)coef[s][4] * hs[s][3]);
      const int64_t v = (int64_t)(acc + (1ull << 27)) >> 28;
      const int o = (int)min(max(v, -(int64_t)(1 << 30)), (int64_t)((1 << 30) - 1));
      hs[s][1] = hs[s][0]; hs[s][0] = u; hs[s][3] = hs[s][2]; hs[s][2] = o;
      u = o;
    }
  }
  return clamp16((u + 128) >> 8);
}

}  // namespace

// grid ceil(n_channels / 16), 256 lanes
__global__ __launch_bounds__(ASDR_TONE_THREADS) void asdr_tone_kernel(ToneArgs a) {
  __shared__ uint32_t ring[ASDR_TONE_ROWS * ASDR_TONE_RING_PITCH];   // [16][129]: two blocks of x as int16 pairs
  __shared__ uint32_t ybuf[ASDR_TONE_ROWS * ASDR_TONE_OUT_PITCH];    // [16][65]: the block's y
  __shared__ int dbuf[ASDR_TONE_ROWS * 8];                           // the block's d
  __shared__ __attribute__((aligned(16))) uint32_t ctab[ASDR_TONE_TABLE];
  __shared__ uint64_t vpow[ASDR_TONE_ROWS], voth[ASDR_TONE_ROWS];    // a window's P_best and other ...
  __shared__ int vbest[ASDR_TONE_ROWS];                              // ... and best
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, piece = t & 15, row = t >> 4;
  const int c0 = blockIdx.x * ASDR_TONE_ROWS, last_c = a.n_channels - 1;
  const int rc = min(c0 + row, last_c);

  ((uint4 *)ctab)[t] = ((const uint4 *)a.table)[t];

  // hist: 96 bytes as six 16-byte pieces, into the tail of ring half 1
  const int hrow = t / 6, hpiece = t % 6;
  if (t < 6 * ASDR_TONE_ROWS) {
    const uint4 h = ((const uint4 *)(a.state + min(c0 + hrow, last_c)))[hpiece];
    uint32_t *d = ring + hrow * ASDR_TONE_RING_PITCH + 104 + 4 * hpiece;
    d[0] = h.x; d[1] = h.y; d[2] = h.z; d[3] = h.w;
  }

  // the recurrence part's channel: wave 0, lane t
  const bool owner = t < ASDR_TONE_ROWS, live = owner && c0 + t <= last_c;
  const int oc = min(c0 + t, last_c);
  int hs[ASDR_TONE_MAX_SECTIONS][4] = {};
  uint64_t last_power = 0, last_other = 0, min_power = 0;
  uint32_t windows = 0, matches = 0, openings = 0, open_blocks = 0, hang_left = 0, open = 0, hang_windows = 0;
  int detected = -1, last_best = -1, want = ASDR_TONE_PASS, own_wb = 0;
  if (owner) {
    const uint4 *rec = (const uint4 *)(a.state + oc);
    const uint4 r6 = rec[6], r7 = rec[7], r8 = rec[8], r9 = rec[9], r10 = rec[10], r11 = rec[11];
    hs[0][0] = (int)r6.x; hs[0][1] = (int)r6.y; hs[0][2] = (int)r6.z; hs[0][3] = (int)r6.w;
    hs[1][0] = (int)r7.x; hs[1][1] = (int)r7.y; hs[1][2] = (int)r7.z; hs[1][3] = (int)r7.w;
    hs[2][0] = (int)r8.x; hs[2][1] = (int)r8.y; hs[2][2] = (int)r8.z; hs[2][3] = (int)r8.w;
    last_power = r9.x | ((uint64_t)r9.y << 32); last_other = r9.z | ((uint64_t)r9.w << 32);
    windows = r10.x; matches = r10.y; openings = r10.z; open_blocks = r10.w;
    detected = lo16(r11.x); last_best = hi16(r11.x);
    own_wb = (int)(r11.y & 0xFFFFu); hang_left = (r11.y >> 16) & 0xFFu; open = (r11.y >> 24) & 1u;
    const ToneSetting st = a.set[oc];
    min_power = st.min_power; want = st.want; hang_windows = st.hang_windows;
  }

  // the correlation part's channels: rows 4 wave .. 4 wave + 3, lane = tone
  const uint32_t step = a.steps[lane];
  const bool tone = lane < a.n_tones;
  int re[ASDR_TONE_WAVE_ROWS], im[ASDR_TONE_WAVE_ROWS], wb[ASDR_TONE_WAVE_ROWS];
#pragma unroll
  for (int q = 0; q < ASDR_TONE_WAVE_ROWS; q++) {
    const char *rec = (const char *)(a.state + min(c0 + ASDR_TONE_WAVE_ROWS * wave + q, last_c));
    const uint2 v = ((const uint2 *)(rec + 192))[lane];
    re[q] = (int)v.x; im[q] = (int)v.y;
    wb[q] = __builtin_amdgcn_readfirstlane((int)(*(const uint32_t *)(rec + 180) & 0xFFFFu));
  }

  auto request = [&](int b) { return *(const uint4 *)(a.in + (((int64_t)rc * a.in_stride_blocks + b) * 128 + 8 * piece)); };
  uint4 next_x = request(0);

  for (int b = 0; b < a.n_blocks; b++) {
    const int half = b & 1;
    {
      const uint4 x = next_x;
      if (b + 1 < a.n_blocks) next_x = request(b + 1);
      uint32_t *d = ring + row * ASDR_TONE_RING_PITCH + 64 * half + 4 * piece;
      d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
    }
    __syncthreads();

    // step 1: d_k of row r from the words 8 k - 15 .. 8 k + 7 of the block (word m holds the samples of taps 45 - 2 m and 44 - 2 m)
    if (t < 8 * ASDR_TONE_ROWS) {
      const int r = t & 15, k = t >> 4;
      const uint32_t *x = ring + r * ASDR_TONE_RING_PITCH;
      const int base = 64 * half + 8 * k - 15;
      int s = 2048;
#pragma unroll
      for (int m = 0; m < 23; m++) {
        const uint32_t w = x[(base + m) & 127];
        s += kCic.h[45 - 2 * m] * lo16(w) + kCic.h[44 - 2 * m] * hi16(w);   // |s| <= 2^27
      }
      dbuf[r * 8 + k] = s >> 12;
    }
    __syncthreads();

    // step 2, and the powers at a window's end
#pragma unroll
    for (int q = 0; q < ASDR_TONE_WAVE_ROWS; q++) {
      const int r = ASDR_TONE_WAVE_ROWS * wave + q;
      const uint32_t p0 = 8u * (uint32_t)wb[q];
      int64_t R = 0, S = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int d = dbuf[r * 8 + k];
        const uint32_t e = ctab[(step * (p0 + k)) >> 22];
        R += (int64_t)d * lo16(e);
        S += (int64_t)d * hi16(e);
      }
      if (tone) {
        re[q] = (int)((uint32_t)re[q] + (uint32_t)(int)(R >> 9));
        im[q] = (int)((uint32_t)im[q] + (uint32_t)(int)(S >> 9));
      }
      if (++wb[q] == a.window) {                              // the same in every lane
        const uint64_t P = sq(re[q]) + sq(im[q]);
        uint64_t bp = P;
        int bi = lane;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint64_t op = __shfl_xor(bp, d);
          const int oi = __shfl_xor(bi, d);
          const bool take = op > bp || (op == bp && oi < bi);
          bp = take ? op : bp; bi = take ? oi : bi;
        }
        const int dist = lane - bi;
        uint64_t other = (dist >= 2 || dist <= -2) ? P : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint64_t oo = __shfl_xor(other, d);
          other = oo > other ? oo : other;
        }
        if (lane == 0) { vpow[r] = bp; voth[r] = other; vbest[r] = bi; }
        re[q] = im[q] = 0; wb[q] = 0;
      }
    }

    // steps 3 and 4
    if (owner) {
      const bool muted = want != ASDR_TONE_PASS && open == 0;
      const uint32_t keep = muted ? 0u : 0xFFFFFFFFu;
      open_blocks += muted ? 0u : 1u;
      const uint32_t *x = ring + t * ASDR_TONE_RING_PITCH + 64 * half;
      uint32_t *y = ybuf + t * ASDR_TONE_OUT_PITCH;
#pragma unroll 1
      for (int g = 0; g < 64; g += 4) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = x[g + k];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int y0 = tone_highpass(lo16(w[k]), a.sections, a.coef, hs);
          const int y1 = tone_highpass(hi16(w[k]), a.sections, a.coef, hs);
          w[k] = (((uint32_t)y0 & 0xFFFFu) | ((uint32_t)y1 << 16)) & keep;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) y[g + k] = w[k];
      }
    }
    __syncthreads();

    // step 5
    if (owner && ++own_wb == a.window) {
      const uint64_t P = vpow[t], other = voth[t];
      const int best = vbest[t];
      detected = (P >= min_power && 16ull * (P >> 8) >= (uint64_t)a.dominance * (other >> 8)) ? best : -1;
      const bool match = want == ASDR_TONE_PASS || (want == ASDR_TONE_ANY ? detected >= 0 : detected == want);
      if (match) { openings += open ^ 1u; open = 1; hang_left = hang_windows; }
      else if (open && hang_left > 0) hang_left--;
      else open = 0;
      windows++; matches += match ? 1u : 0u;
      last_best = best; last_power = P; last_other = other;
      own_wb = 0;
    }

    {
      const uint32_t *d = ybuf + row * ASDR_TONE_OUT_PITCH + 4 * piece;
      const uint4 y = make_uint4(d[0], d[1], d[2], d[3]);
      if (c0 + row <= last_c) *(uint4 *)(a.out + (((int64_t)(c0 + row) * a.out_stride_blocks + b) * 128 + 8 * piece)) = y;
    }
  }

  // the last block's half of the ring was complete before that block's first barrier
  if (t < 6 * ASDR_TONE_ROWS && c0 + hrow <= last_c) {
    const uint32_t *d = ring + hrow * ASDR_TONE_RING_PITCH + 64 * ((a.n_blocks - 1) & 1) + 40 + 4 * hpiece;
    ((uint4 *)(a.state + c0 + hrow))[hpiece] = make_uint4(d[0], d[1], d[2], d[3]);
  }
#pragma unroll
  for (int q = 0; q < ASDR_TONE_WAVE_ROWS; q++) {
    const int c = c0 + ASDR_TONE_WAVE_ROWS * wave + q;
    if (c <= last_c) ((uint2 *)((char *)(a.state + c) + 192))[lane] = make_uint2((uint32_t)re[q], (uint32_t)im[q]);
  }
  if (live) {
    uint4 *rec = (uint4 *)(a.state + oc);
    rec[6] = make_uint4((uint32_t)hs[0][0], (uint32_t)hs[0][1], (uint32_t)hs[0][2], (uint32_t)hs[0][3]);
    rec[7] = make_uint4((uint32_t)hs[1][0], (uint32_t)hs[1][1], (uint32_t)hs[1][2], (uint32_t)hs[1][3]);
    rec[8] = make_uint4((uint32_t)hs[2][0], (uint32_t)hs[2][1], (uint32_t)hs[2][2], (uint32_t)hs[2][3]);
    rec[9] = make_uint4((uint32_t)last_power, (uint32_t)(last_power >> 32), (uint32_t)last_other, (uint32_t)(last_other >> 32));
    rec[10] = make_uint4(windows, matches, openings, open_blocks);
    rec[11] = make_uint4(((uint32_t)detected & 0xFFFFu) | ((uint32_t)last_best << 16), (uint32_t)own_wb | (hang_left << 16) | (open << 24), 0u, 0u);
  }
}

extern "C" int asdr_launch_tone(const ToneArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0 || a->n_blocks <= 0) return 0;
  const dim3 grid(((uint32_t)a->n_channels + ASDR_TONE_ROWS - 1) / ASDR_TONE_ROWS);
  hipLaunchKernelGGL(asdr_tone_kernel, grid, dim3(ASDR_TONE_THREADS), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
