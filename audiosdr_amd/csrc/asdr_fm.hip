// asdr_fm.hip -- the FM demodulator's kernel (include/asdr_fm.h): a tuner bank's int16 I/Q rows into int16 audio rows, with a noise
// squelch.  A deployment that creates no FM demodulator launches nothing from this file.
//
// Form.  A workgroup of four waves owns ROWS channels -- 64 in a bank of ASDR_FM_WIDE_CHANNELS channels or more, 16
// in a smaller one, which so fills more of the chip -- and walks their rows one 128-sample block at a time:
//  * Pointwise part (steps 1 to 4: conjugate product, CORDIC, gain, noise probe), lanes across samples.  A lane takes one 16-byte
//    piece (8 samples) of I and of Q; the 16 lanes of a row sit on its 16 adjacent pieces, a wave on 4 rows, the workgroup on 16,
//    so ROWS / 16 passes cover the rows.  The sample before a piece's first, and the two v before it, come from the neighbouring lane
//    by one cross-lane read each; the lane of a row's first piece gets them from the row's carry words in LDS, which the lane of
//    the row's last piece rewrites behind it (both lanes are in one wave, whose LDS accesses keep their order).  The block's sums N
//    and P are reduced over the row's 16 lanes by four butterfly steps in 64 bits.  v goes to LDS as packed int16 pairs.  The next
//    pass's (or block's) two loads are issued before the current pass's arithmetic and land in registers meanwhile.
//  * Recurrence part (steps 5 and 6 and the squelch), a lane of wave 0 per channel.  A staged row takes 65 words, odd, so the
//    lanes' reads of one offset fall into different banks.  The squelch is decided from N first; y (or 0) replaces v in place.
//  * Output: the lane that staged a piece reads it back and stores it as 16 bytes, so no barrier is needed between a block's
//    output and the next block's staging.  Nothing is read twice from HBM, and a muted block never leaves as anything but zeros.
//  * State: wave 0 reads each record once before the first block and writes it once behind the last, as three 16-byte stores.
// Rows past n_channels in the last workgroup read channel n_channels - 1 again and write nothing.
#include <hip/hip_runtime.h>

#include "asdr_fm_device.h"

namespace {

// A[k] = floor(atan(2^-k) / (2 pi) * 2^32 + 0.5)
constexpr uint32_t kAtan[ASDR_FM_CORDIC_ITERS] = {536870912u, 316933406u, 167458907u, 85004756u, 42667331u, 21354465u, 10679838u,
                                                  5340245u,   2670163u,   1335087u,   667544u,   333772u,   166886u,   83443u,
                                                  41722u,     20861u,     10430u,     5215u,     2608u,     1304u};

__device__ inline int clamp16(int x) { return min(max(x, -32768), 32767); }

// steps 1 to 3 of one sample: v from (I, Q) and the sample before it
__device__ inline int fm_discriminate(int I, int Q, int Ip, int Qp, uint32_t gain) {
  const int64_t re64 = (int64_t)I * Ip + (int64_t)Q * Qp, im64 = (int64_t)Q * Ip - (int64_t)I * Qp;   // |.| <= 2^31
  const uint64_t big = (uint64_t)max(re64 < 0 ? -re64 : re64, im64 < 0 ? -im64 : im64);
  // branch-free, so that a piece's eight samples interleave.  The shift by 29 - L, L = 64 - clz, is -3 .. 28: done as a left shift
  // by 0 .. 31 (below 2^32 in magnitude) and an arithmetic right shift by 3, which floors as the right shift alone would
  const int up = __builtin_clzll(big | 1) - 32;
  int re = (int)((re64 << up) >> 3), im = (int)((im64 << up) >> 3);   // |.| < 2^29
  const int ng = re >> 31;                                    // re < 0: negate both, start from pi
  re = (re ^ ng) - ng; im = (im ^ ng) - ng;
  uint32_t theta = (uint32_t)ng << 31;
#pragma unroll
  for (int k = 0; k < ASDR_FM_CORDIC_ITERS; k++) {
    const int sg = im >> 31;                                  // 0 or -1: (x ^ sg) - sg is x or -x
    const int dr = ((im >> k) ^ sg) - sg, di = ((re >> k) ^ sg) - sg;
    re += dr; im -= di;
    theta += (kAtan[k] ^ (uint32_t)sg) - (uint32_t)sg;
  }
  const int v = clamp16((int)(((int64_t)(int)theta * (int64_t)gain) >> 31));   // |.| <= 2^24 before the clamp
  return big ? v : 0;                                         // re == im == 0 gives theta = 0
}

__device__ inline uint64_t row_sum(uint64_t x) {              // over the 16 lanes of a row
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) x += __shfl_xor(x, d);
  return x;
}

// steps 5 and 6 of one sample
__device__ inline int fm_filter(int v, int hp_shift, int a, int &m, int &s) {
  const int mn = (int)((uint32_t)m + (uint32_t)((int)(((uint32_t)v << 15) - (uint32_t)m) >> hp_shift));
  const int xn = clamp16(v - ((int)((uint32_t)mn + (1u << 14)) >> 15));
  m = hp_shift ? mn : m;                                      // selects: the lanes of a wave differ in hp_shift
  const int x = hp_shift ? xn : v;
  const int d = (int)(((uint32_t)x << 15) - (uint32_t)s);
  s = (int)((uint32_t)s + (uint32_t)(((int64_t)d * a) >> 15));
  return clamp16((int)((uint32_t)s + (1u << 14)) >> 15);
}

}  // namespace

// grid ceil(n_channels / ROWS), 256 lanes
template <int ROWS>
__global__ __launch_bounds__(ASDR_FM_THREADS) void asdr_fm_kernel(FmArgs a) {
  constexpr int PASSES = ROWS / 16;
  __shared__ uint32_t vbuf[ROWS * ASDR_FM_PITCH];             // [ROWS][65]: v, then y, as int16 pairs
  __shared__ uint64_t nbuf[ROWS], pbuf[ROWS];                 // the block's N and P
  __shared__ uint32_t carry_iq[ROWS];                         // the sample before the next one: I | Q << 16
  __shared__ uint32_t carry_v[ROWS];                          // the two v before the next one: v2 | v1 << 16
  __shared__ uint32_t gains[ROWS];
  const int t = threadIdx.x, lane = t & 63, piece = t & 15, sub = t >> 4;   // in pass p the lane takes piece `piece` of row 16 p + sub
  const int c0 = blockIdx.x * ROWS;
  const int last_c = a.n_channels - 1;

  // the recurrence part's channel: wave 0, lane t
  const bool owner = t < ROWS, live = owner && c0 + t <= last_c;
  const int oc = min(c0 + t, last_c);
  int m = 0, s = 0, hp_shift = 0, deemph = 32768, hang_blocks = 0;
  uint64_t open_noise = 0, close_noise = 0, last_noise = 0, last_power = 0;
  uint32_t openings = 0, open_blocks = 0, hang_left = 0, open = 0;
  if (owner) {
    const uint4 *rec = (const uint4 *)(a.state + oc);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    carry_iq[t] = r0.x;
    carry_v[t] = (r0.y >> 16) | (r0.y << 16);                 // the record holds v1 | v2 << 16
    s = (int)r0.z; m = (int)r0.w;
    last_noise = r1.x | ((uint64_t)r1.y << 32); last_power = r1.z | ((uint64_t)r1.w << 32);
    openings = r2.x; open_blocks = r2.y; hang_left = r2.z & 0xFFFFu; open = (r2.z >> 16) & 1u;
    const FmSetting st = a.set[oc];
    open_noise = st.open_noise; close_noise = st.close_noise;
    gains[t] = st.gain; deemph = (int)st.deemphasis; hang_blocks = (int)st.hang_blocks; hp_shift = (int)st.hp_shift;
  }
  __syncthreads();

  // the loads of (block b, pass p); rows past the last channel read the last channel's
  uint4 next_i, next_q;
  auto request = [&](int b, int p) {
    const int64_t off = ((int64_t)min(c0 + 16 * p + sub, last_c) * a.in_stride_blocks + b) * 128 + 8 * piece;
    next_i = *(const uint4 *)(a.i + off);
    next_q = *(const uint4 *)(a.q + off);
  };
  request(0, 0);
  const int from = (lane & ~15) | ((piece + 15) & 15);        // the lane of the piece before this one (of the last, for the first)

  for (int b = 0; b < a.n_blocks; b++) {
#pragma unroll 1
    for (int p = 0; p < PASSES; p++) {
      const int r = 16 * p + sub;
      const uint4 wi = next_i, wq = next_q;
      if (p + 1 < PASSES) request(b, p + 1);
      else if (b + 1 < a.n_blocks) request(b + 1, 0);
      const uint32_t iw[4] = {wi.x, wi.y, wi.z, wi.w}, qw[4] = {wq.x, wq.y, wq.z, wq.w};
      const uint32_t gain = gains[r];
      // the sample before this piece: the neighbour's last, or the row's carry
      const uint32_t mine = (iw[3] >> 16) | (qw[3] & 0xFFFF0000u);
      const uint32_t before = (uint32_t)__shfl((int)(piece == 15 ? carry_iq[r] : mine), from);
      int Ip = (int)(int16_t)(before & 0xFFFFu), Qp = (int)before >> 16;
      int v[8];
      uint64_t P = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint32_t wI = iw[j >> 1], wQ = qw[j >> 1];
        const int I = (j & 1) ? (int)wI >> 16 : (int)(int16_t)(wI & 0xFFFFu), Q = (j & 1) ? (int)wQ >> 16 : (int)(int16_t)(wQ & 0xFFFFu);
        v[j] = fm_discriminate(I, Q, Ip, Qp, gain);
        P += (uint32_t)(I * I) + (uint64_t)(uint32_t)(Q * Q);   // each square <= 2^30
        Ip = I; Qp = Q;
      }
      // the two v before this piece, likewise
      const uint32_t mine_v = ((uint32_t)v[6] & 0xFFFFu) | ((uint32_t)v[7] << 16);
      const uint32_t before_v = (uint32_t)__shfl((int)(piece == 15 ? carry_v[r] : mine_v), from);
      int v2 = (int)(int16_t)(before_v & 0xFFFFu), v1 = (int)before_v >> 16;
      uint64_t N = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int w = v[j] - 2 * v1 + v2;                     // |w| <= 2^17
        N += (uint64_t)((int64_t)w * w);
        v2 = v1; v1 = v[j];
      }
      if (piece == 15) { carry_iq[r] = mine; carry_v[r] = mine_v; }
      uint32_t *d = vbuf + r * ASDR_FM_PITCH + 4 * piece;
#pragma unroll
      for (int k = 0; k < 4; k++) d[k] = ((uint32_t)v[2 * k] & 0xFFFFu) | ((uint32_t)v[2 * k + 1] << 16);
      N = row_sum(N); P = row_sum(P);
      if (piece == 0) { nbuf[r] = N; pbuf[r] = P; }
    }
    __syncthreads();

    if (owner) {
      const uint64_t N = nbuf[t];
      if (N <= open_noise) { openings += open ^ 1u; open = 1; hang_left = (uint32_t)hang_blocks; }
      else if (open && N <= close_noise) hang_left = (uint32_t)hang_blocks;
      else if (open && hang_left > 0) hang_left--;
      else open = 0;
      open_blocks += open;
      last_noise = N; last_power = pbuf[t];
      const uint32_t keep = open ? 0xFFFFFFFFu : 0u;
      uint32_t *x = vbuf + t * ASDR_FM_PITCH;
#pragma unroll 1
      for (int g = 0; g < 64; g += 8) {
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = x[g + k];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int y0 = fm_filter((int)(int16_t)(w[k] & 0xFFFFu), hp_shift, deemph, m, s);
          const int y1 = fm_filter((int)w[k] >> 16, hp_shift, deemph, m, s);
          w[k] = (((uint32_t)y0 & 0xFFFFu) | ((uint32_t)y1 << 16)) & keep;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) x[g + k] = w[k];
      }
    }
    __syncthreads();

#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const int r = 16 * p + sub, c = c0 + r;
      const uint32_t *d = vbuf + r * ASDR_FM_PITCH + 4 * piece;
      const uint4 y = make_uint4(d[0], d[1], d[2], d[3]);
      if (c <= last_c) *(uint4 *)(a.out + (((int64_t)c * a.out_stride_blocks + b) * 128 + 8 * piece)) = y;
    }
  }

  // the carries were last written before the last block's first barrier
  if (live) {
    uint4 *rec = (uint4 *)(a.state + oc);
    const uint32_t cv = carry_v[t];
    rec[0] = make_uint4(carry_iq[t], (cv >> 16) | (cv << 16), (uint32_t)s, (uint32_t)m);
    rec[1] = make_uint4((uint32_t)last_noise, (uint32_t)(last_noise >> 32), (uint32_t)last_power, (uint32_t)(last_power >> 32));
    rec[2] = make_uint4(openings, open_blocks, hang_left | (open << 16), 0u);
  }
}

extern "C" int asdr_launch_fm(const FmArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0 || a->n_blocks <= 0) return 0;
  if (a->n_channels >= ASDR_FM_WIDE_CHANNELS) {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_FM_ROWS - 1) / ASDR_FM_ROWS);
    hipLaunchKernelGGL(asdr_fm_kernel<ASDR_FM_ROWS>, grid, dim3(ASDR_FM_THREADS), 0, stream, *a);
  } else {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_FM_NARROW_ROWS - 1) / ASDR_FM_NARROW_ROWS);
    hipLaunchKernelGGL(asdr_fm_kernel<ASDR_FM_NARROW_ROWS>, grid, dim3(ASDR_FM_THREADS), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
