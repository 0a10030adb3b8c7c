// asdr_dcs.hip -- the DCS squelch's kernel (include/asdr_dcs.h): code search and code squelch on the int16 audio rows the FM
// demodulator writes.  A deployment that creates no DCS squelch launches nothing from this file.
//
// Form.  A workgroup of four waves owns ROWS channels -- 64 in a bank of ASDR_DCS_WIDE_CHANNELS channels or more, 16
// in a smaller one, which so fills more of the chip -- and walks their rows one 128-sample block at a time:
//  * Staging: a lane takes one 16-byte piece (8 samples) of a row, the 16 lanes of a row its 16 pieces, the workgroup 16 rows a
//    pass, ROWS / 16 passes.  A row lives in LDS as a ring of two blocks (128 words + 1, odd): block b goes to half b & 1, so the 45
//    samples before it (the other half's tail; hist of the record before the first block) are in place without a move.  The next
//    block's loads are issued before the current block's work.
//  * Output: the lane that staged a piece stores it from its registers, or zeros, by the row's mask in LDS: the channel's open as it
//    stood at the block's start, which the channel's owner left there behind the block before (the record's, before the first).
//  * Decimator (step 1) and bit filter (step 2), lanes across outputs: one d_k per lane from 23 word reads and 46 multiply-adds in
//    int32 into the row's ring of the last 32 d (block b at (b & 3) * 8; dhist of the record in front of the first block), then one
//    s per lane from 20 reads of that ring.
//  * Slicer, clock and register (steps 3 and 4), a lane of wave 0 per channel: 8 short steps on the row's 8 s, then the table scan
//    on the at most one bit the block gave, the table read wave-uniformly from LDS.
//  * State: read once before the first block and written once behind the last, in 16-byte accesses.
// Rows past n_channels in the last workgroup read channel n_channels - 1 again and write nothing.
#include <hip/hip_runtime.h>

#include "asdr_dcs_device.h"

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

__device__ inline int lo16(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ inline int hi16(uint32_t w) { return (int)w >> 16; }
__device__ inline uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

}  // namespace

// grid ceil(n_channels / ROWS), 256 lanes
template <int ROWS>
__global__ __launch_bounds__(ASDR_DCS_THREADS) void asdr_dcs_kernel(DcsArgs a) {
  constexpr int PASSES = ROWS / 16;
  __shared__ uint32_t ring[ROWS * ASDR_DCS_RING_PITCH];       // [ROWS][129]: two blocks of x as int16 pairs
  __shared__ int dring[ROWS * ASDR_DCS_D_PITCH];              // [ROWS][33]: the last 32 d
  __shared__ int sbuf[ROWS * ASDR_DCS_S_PITCH];               // [ROWS][9]: the block's s
  __shared__ uint32_t keep[2][ROWS];                          // all ones, or 0 for a muted row: of block b in keep[b & 1]
  __shared__ uint32_t tab[ASDR_DCS_MAX_CODES];
  const int t = threadIdx.x, piece = t & 15, sub = t >> 4;    // in pass p the lane takes piece `piece` of row 16 p + sub
  const int c0 = blockIdx.x * ROWS, last_c = a.n_channels - 1;

  if (t < ASDR_DCS_MAX_CODES) tab[t] = a.table[t];

  // hist: 96 bytes as six 16-byte pieces, into the tail of ring half 1; dhist: 48 bytes as three, in front of block 0's place
  for (int i = t; i < 9 * ROWS; i += ASDR_DCS_THREADS) {
    const int r = i / 9, q = i % 9;
    const uint4 h = ((const uint4 *)(a.state + min(c0 + r, last_c)))[q];
    if (q < 6) {
      uint32_t *d = ring + r * ASDR_DCS_RING_PITCH + 104 + 4 * q;
      d[0] = h.x; d[1] = h.y; d[2] = h.z; d[3] = h.w;
    } else {
      int *d = dring + r * ASDR_DCS_D_PITCH + 8 * (q - 5);
      d[0] = lo16(h.x); d[1] = hi16(h.x); d[2] = lo16(h.y); d[3] = hi16(h.y);
      d[4] = lo16(h.z); d[5] = hi16(h.z); d[6] = lo16(h.w); d[7] = hi16(h.w);
    }
  }

  // the sequential part's channel: wave 0, lane t
  const bool owner = t < ROWS, live = owner && c0 + t <= last_c;
  const int oc = min(c0 + t, last_c);
  uint32_t sr = 0, bits = 0, hits = 0, detections = 0, openings = 0, open_blocks = 0, edges = 0, open = 0;
  int detected = -1, cand = -1, clk = 0, quiet = 0, age = 255, run = 0, bit = 0, want = ASDR_DCS_PASS, hyst = 0;
  if (owner) {
    const uint4 *rec = (const uint4 *)(a.state + oc);
    const uint4 r9 = rec[9], r10 = rec[10], r11 = rec[11];
    sr = r9.x; bits = r9.y; hits = r9.z; detections = r9.w;
    openings = r10.x; open_blocks = r10.y; edges = r10.z; detected = lo16(r10.w); cand = hi16(r10.w);
    clk = (int)(r11.x & 0xFFFFu); quiet = (int)(r11.x >> 16);
    age = (int)(r11.y & 0xFFu); run = (int)((r11.y >> 8) & 0xFFu); bit = (int)((r11.y >> 16) & 1u); open = (r11.y >> 24) & 1u;
    const DcsSetting st = a.set[oc];
    want = st.want;
    hyst = (int)min(st.hysteresis, 0x7FFFFFFFu);              // |s| < 2^20: every hysteresis from there on holds b alike
    keep[0][t] = (want == ASDR_DCS_PASS || open) ? 0xFFFFFFFFu : 0u;
  }

  uint4 next_x[PASSES];
  auto request = [&](int b) {
#pragma unroll
    for (int p = 0; p < PASSES; p++)
      next_x[p] = *(const uint4 *)(a.in + (((int64_t)min(c0 + 16 * p + sub, last_c) * a.in_stride_blocks + b) * 128 + 8 * piece));
  };
  request(0);

  for (int b = 0; b < a.n_blocks; b++) {
    const int half = b & 1, slot = 8 * (b & 3);
    uint4 x[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) x[p] = next_x[p];
    if (b + 1 < a.n_blocks) request(b + 1);
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      uint32_t *d = ring + (16 * p + sub) * ASDR_DCS_RING_PITCH + 64 * half + 4 * piece;
      d[0] = x[p].x; d[1] = x[p].y; d[2] = x[p].z; d[3] = x[p].w;
    }
    __syncthreads();

    // step 5, from the registers
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const int r = 16 * p + sub, c = c0 + r;
      const uint32_t m = keep[half][r];
      if (c <= last_c)
        *(uint4 *)(a.out + (((int64_t)c * a.out_stride_blocks + b) * 128 + 8 * piece)) = make_uint4(x[p].x & m, x[p].y & m, x[p].z & m, x[p].w & m);
    }

    // step 1: d_k of row r from the words 8 k - 15 .. 8 k + 7 of the block (word m holds the samples of taps 45 - 2 m and 44 - 2 m)
#pragma unroll
    for (int i = t; i < 8 * ROWS; i += ASDR_DCS_THREADS) {
      const int r = i % ROWS, k = i / ROWS;
      const uint32_t *xr = ring + r * ASDR_DCS_RING_PITCH;
      const int base = 64 * half + 8 * k - 15;
      int s = 2048;
#pragma unroll
      for (int m = 0; m < 23; m++) {
        const uint32_t w = xr[(base + m) & 127];
        s += kCic.h[45 - 2 * m] * lo16(w) + kCic.h[44 - 2 * m] * hi16(w);   // |s| <= 2^27
      }
      dring[r * ASDR_DCS_D_PITCH + slot + k] = s >> 12;
    }
    __syncthreads();

    // step 2: the sum of the 20 newest d at k
#pragma unroll
    for (int i = t; i < 8 * ROWS; i += ASDR_DCS_THREADS) {
      const int r = i % ROWS, k = i / ROWS;
      const int *dr = dring + r * ASDR_DCS_D_PITCH;
      int s = 0;
#pragma unroll
      for (int j = 0; j < 20; j++) s += dr[(slot + k - j) & 31];
      sbuf[r * ASDR_DCS_S_PITCH + k] = s;
    }
    __syncthreads();

    // steps 3 and 4
    if (owner) {
      open_blocks += (want == ASDR_DCS_PASS || open) ? 1u : 0u;
      bool took = false;
      int took_bit = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int s = sbuf[t * ASDR_DCS_S_PITCH + k];
        const int nb = s > hyst ? 1 : (s < -hyst ? 0 : bit);
        const bool edge = nb != bit;
        const int e = clk < ASDR_DCS_HALF ? clk : clk - ASDR_DCS_CLOCK;
        int moved = clk - (e >> 2);                           // 0 .. 2625
        moved = moved >= ASDR_DCS_CLOCK ? moved - ASDR_DCS_CLOCK : moved;
        clk = edge ? moved : clk;
        edges += edge ? 1u : 0u;
        bit = nb;
        const int p = clk;
        clk += 128;
        if (p < ASDR_DCS_HALF && clk >= ASDR_DCS_HALF) { took = true; took_bit = bit; }
        clk = clk >= ASDR_DCS_CLOCK ? clk - ASDR_DCS_CLOCK : clk;
      }
      if (took) {
        sr = (sr >> 1) | ((uint32_t)took_bit << 22);
        bits++;
        age = min(age + 1, 255);
        quiet = min(quiet + 1, 65535);
        int best = 0, dist = 32;
        for (int i = 0; i < a.n_codes; i++) {                 // the same bounds and words in every lane
          const int d = __popc(sr ^ tab[i]);
          if (d < dist) { dist = d; best = i; }
        }
        if (dist <= a.max_errors) {
          hits++;
          run = (best == cand && age == 23) ? min(run + 1, 255) : 1;
          cand = best; age = 0;
          if (run >= a.confirm) {
            detections += detected != best ? 1u : 0u;
            detected = best; quiet = 0;
          }
        }
        if (detected >= 0 && quiet > a.hold_bits) detected = -1;
        const bool match = want == ASDR_DCS_PASS || (want == ASDR_DCS_ANY ? detected >= 0 : detected == want);
        openings += (match && !open) ? 1u : 0u;
        open = match ? 1u : 0u;
      }
      keep[half ^ 1][t] = (want == ASDR_DCS_PASS || open) ? 0xFFFFFFFFu : 0u;
    }
  }

  // the last block's half of the ring was complete before that block's first barrier, its d before the second
  const int last_b = a.n_blocks - 1;
  for (int i = t; i < 9 * ROWS; i += ASDR_DCS_THREADS) {
    const int r = i / 9, q = i % 9;
    if (c0 + r > last_c) continue;
    uint4 v;
    if (q < 6) {
      const uint32_t *d = ring + r * ASDR_DCS_RING_PITCH + 64 * (last_b & 1) + 40 + 4 * q;
      v = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
      const int *d = dring + r * ASDR_DCS_D_PITCH;
      const int first = 8 * (last_b & 3) + 16 + 8 * (q - 6);  // the 24 newest end with the last block's 8: they start 16 before them
      v = make_uint4(pack16(d[first & 31], d[(first + 1) & 31]), pack16(d[(first + 2) & 31], d[(first + 3) & 31]),
                     pack16(d[(first + 4) & 31], d[(first + 5) & 31]), pack16(d[(first + 6) & 31], d[(first + 7) & 31]));
    }
    ((uint4 *)(a.state + c0 + r))[q] = v;
  }
  if (live) {
    uint4 *rec = (uint4 *)(a.state + oc);
    rec[9] = make_uint4(sr, bits, hits, detections);
    rec[10] = make_uint4(openings, open_blocks, edges, pack16(detected, cand));
    rec[11] = make_uint4((uint32_t)clk | ((uint32_t)quiet << 16), (uint32_t)age | ((uint32_t)run << 8) | ((uint32_t)bit << 16) | (open << 24), 0u, 0u);
  }
}

extern "C" int asdr_launch_dcs(const DcsArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0 || a->n_blocks <= 0) return 0;
  if (a->n_channels >= ASDR_DCS_WIDE_CHANNELS) {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_DCS_ROWS - 1) / ASDR_DCS_ROWS);
    hipLaunchKernelGGL(asdr_dcs_kernel<ASDR_DCS_ROWS>, grid, dim3(ASDR_DCS_THREADS), 0, stream, *a);
  } else {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_DCS_NARROW_ROWS - 1) / ASDR_DCS_NARROW_ROWS);
    hipLaunchKernelGGL(asdr_dcs_kernel<ASDR_DCS_NARROW_ROWS>, grid, dim3(ASDR_DCS_THREADS), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
