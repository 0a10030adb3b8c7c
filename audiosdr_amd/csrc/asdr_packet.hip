// asdr_packet.hip -- the packet decoder's kernels (include/asdr_packet.h): 1200-baud AFSK demodulation and AX.25 framing on the int16
// audio rows the FM demodulator writes, and the ascending compact delivery of the decoded frames.  A deployment that creates no packet
// decoder launches nothing from this file.
//
// Form of the pass, after the DCS squelch's.  A workgroup of four waves owns ROWS channels -- 64 in a bank of
// ASDR_PACKET_WIDE_CHANNELS channels or more, 16 in a smaller one, which so fills more of the chip -- and walks their rows one
// 128-sample block at a time:
//  * Staging: a lane takes one 16-byte piece (8 samples) of a row, the 16 lanes of a row its 16 pieces, the workgroup 16 rows a
//    pass, ROWS / 16 passes.  A row lives in LDS as a ring of two blocks (128 words + 1, odd): block b goes to half b & 1, so the 6
//    samples before it (the other half's tail; hist of the record before the first block) are in place without a move.  The next
//    block's loads are issued before the current block's work.
//  * Decimator (step 1), lanes across outputs with neighbouring lanes on neighbouring rows: one d_k per lane from 5 word reads and 10
//    multiply-adds into the row's ring of the last 64 d (block b at (b & 1) * 32; dhist of the record in front of the first block).
//  * Correlators (step 2), lanes across outputs with the 32 lanes of a wave's half on the 32 values of one row: four 9-tap dot
//    products and e in int64 per lane; only e's sign goes on, as two ballot words a row (e > 0, e < 0).
//  * Slicer, clock, NRZI and HDLC (steps 3 to 5), a lane of wave 0 per channel: 32 short steps on the row's two words, and under
//    them, on the bits the clock takes, the framing.  A byte of the frame under way is stored to the record's buf as it completes;
//    a completed frame (step 6) is copied by its lane from buf to its ring slot, 16 bytes at a time.
//  * State: the first 80 bytes of a record are read once before the first block and written once behind the last, in 16-byte
//    accesses; so is the channel's ring bookkeeping.
// Rows past n_channels in the last workgroup read channel n_channels - 1 again and write nothing.
//
// Form of the collect (after the gate's tile-count, index and packet passes): count sums the frames waiting in each tile of 256
// channels; index gives every channel its position in the ascending order (the tiles before it, then a scan inside the tile), cuts
// at max_frames, lists the ring slots of the delivered frames, advances taken and writes the count; copy moves the listed slots, a
// lane a 16-byte piece.  Every entry of the list has one writer that depends on nothing but the bookkeeping.
#include <hip/hip_runtime.h>

#include "asdr_packet_device.h"

namespace {

constexpr int kH[10] = {1, 3, 6, 10, 12, 12, 10, 6, 3, 1};      // the coefficients of (1 + z + z^2 + z^3)^3

__device__ inline int lo16(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ inline int hi16(uint32_t w) { return (int)w >> 16; }
__device__ inline uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

// the bytes of a word at byte offset `at` of a payload of n bytes that belong to it: the rest zero
__device__ inline uint32_t payload_word(uint32_t w, int at, int n) {
  const int keep = n - at;
  return keep >= 4 ? w : (keep <= 0 ? 0u : w & ((1u << (8 * keep)) - 1u));
}

// the sum over the workgroup's four waves of a per-lane value, and the sum over the waves below this one (every thread calls it)
__device__ inline void wave_totals(uint32_t wave_sum, uint32_t &below, uint32_t &total) {
  __shared__ uint32_t sums[ASDR_PACKET_TILE / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sums[wave] = wave_sum;
  __syncthreads();
  below = 0; total = 0;
#pragma unroll
  for (int w = 0; w < ASDR_PACKET_TILE / 64; w++) {
    if (w < wave) below += sums[w];
    total += sums[w];
  }
}

}  // namespace

// grid ceil(n_channels / ROWS), 256 lanes
template <int ROWS>
__global__ __launch_bounds__(ASDR_PACKET_THREADS) void asdr_packet_kernel(PacketArgs a) {
  constexpr int PASSES = ROWS / 16;
  __shared__ uint32_t ring[ROWS * ASDR_PACKET_RING_PITCH];    // [ROWS][129]: two blocks of x as int16 pairs
  __shared__ int dring[ROWS * ASDR_PACKET_D_PITCH];           // [ROWS][65]: the last 64 d
  __shared__ uint32_t sign[2 * ROWS];                         // [ROWS][2]: bit k of word 0 is e_k > 0, of word 1 e_k < 0
  __shared__ uint32_t boost[ROWS];
  const int t = threadIdx.x, piece = t & 15, sub = t >> 4;    // in pass p the lane takes piece `piece` of row 16 p + sub
  const int c0 = blockIdx.x * ROWS, last_c = a.n_channels - 1;

  // hist: 16 bytes into the tail of ring half 1; dhist: 16 bytes in front of block 0's place
  for (int i = t; i < 2 * ROWS; i += ASDR_PACKET_THREADS) {
    const int r = i >> 1, q = i & 1;
    const uint4 h = ((const uint4 *)(a.state + min(c0 + r, last_c)))[q];
    if (q == 0) {
      uint32_t *d = ring + r * ASDR_PACKET_RING_PITCH + 124;
      d[0] = h.x; d[1] = h.y; d[2] = h.z; d[3] = h.w;
    } else {
      int *d = dring + r * ASDR_PACKET_D_PITCH + 56;
      d[0] = lo16(h.x); d[1] = hi16(h.x); d[2] = lo16(h.y); d[3] = hi16(h.y);
      d[4] = lo16(h.z); d[5] = hi16(h.z); d[6] = lo16(h.w); d[7] = hi16(h.w);
    }
  }

  // the sequential part's channel: wave 0, lane t
  const bool owner = t < ROWS, live = owner && c0 + t <= last_c;
  const int oc = min(c0 + t, last_c);
  uint32_t bits = 0, edges = 0, flags = 0, frames = 0, crc_errors = 0, aborts = 0, clk = 0, len = 0, crc = 0xFFFFu;
  uint32_t bit = 0, prev = 0, sr = 0, cur = 0, nb = 0, in_frame = 0, head = 0, taken = 0, lost = 0;
  if (owner) {
    const uint4 *rec = (const uint4 *)(a.state + oc);
    const uint4 r2 = rec[2], r3 = rec[3], r4 = rec[4];
    bits = r2.x; edges = r2.y; flags = r2.z; frames = r2.w;
    crc_errors = r3.x; aborts = r3.y; clk = r3.z & 0xFFFFu; len = r3.z >> 16;
    crc = r3.w & 0xFFFFu; bit = (r3.w >> 16) & 1u; prev = (r3.w >> 24) & 1u;
    sr = r4.x & 0xFFu; cur = (r4.x >> 8) & 0xFFu; nb = (r4.x >> 16) & 0xFFu; in_frame = (r4.x >> 24) & 1u;
    const uint4 g = *(const uint4 *)(a.rings + oc);
    head = g.x; taken = g.y; lost = g.z;
    boost[t] = a.boost[oc];
  }

  uint4 next_x[PASSES];
  auto request = [&](int b) {
#pragma unroll
    for (int p = 0; p < PASSES; p++)
      next_x[p] = *(const uint4 *)(a.in + (((int64_t)min(c0 + 16 * p + sub, last_c) * a.in_stride_blocks + b) * 128 + 8 * piece));
  };
  request(0);

  for (int b = 0; b < a.n_blocks; b++) {
    const int half = b & 1;
    uint4 x[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) x[p] = next_x[p];
    if (b + 1 < a.n_blocks) request(b + 1);
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      uint32_t *d = ring + (16 * p + sub) * ASDR_PACKET_RING_PITCH + 64 * half + 4 * piece;
      d[0] = x[p].x; d[1] = x[p].y; d[2] = x[p].z; d[3] = x[p].w;
    }
    __syncthreads();

    // step 1: d_k of row r from the words 2 k - 3 .. 2 k + 1 of the block (word m of them holds the samples of taps 9 - 2 m and 8 - 2 m)
#pragma unroll
    for (int i = t; i < 32 * ROWS; i += ASDR_PACKET_THREADS) {
      const int r = i % ROWS, k = i / ROWS;
      const uint32_t *xr = ring + r * ASDR_PACKET_RING_PITCH;
      const int base = 64 * half + 2 * k - 3;
      int s = 32;
#pragma unroll
      for (int m = 0; m < 5; m++) {
        const uint32_t w = xr[(base + m) & 127];
        s += kH[9 - 2 * m] * lo16(w) + kH[8 - 2 * m] * hi16(w);   // |s| <= 2^21 + 32
      }
      dring[r * ASDR_PACKET_D_PITCH + 32 * half + k] = s >> 6;
    }
    __syncthreads();

    // step 2: the sign of e_k; a wave's half is the 32 values of one row
#pragma unroll
    for (int i = t; i < 32 * ROWS; i += ASDR_PACKET_THREADS) {
      const int r = i >> 5, k = i & 31;
      const int *dr = dring + r * ASDR_PACKET_D_PITCH;
      int i1 = 0, q1 = 0, i2 = 0, q2 = 0;                      // |sum| <= 9 * 2^15 * 2^8 < 2^27
#pragma unroll
      for (int j = 0; j < 9; j++) {
        const int d = dr[(32 * half + k - j) & 63];
        i1 += d * ASDR_PACKET_C1200[j]; q1 += d * ASDR_PACKET_S1200[j];
        i2 += d * ASDR_PACKET_C2200[j]; q2 += d * ASDR_PACKET_S2200[j];
      }
      i1 >>= 8; q1 >>= 8; i2 >>= 8; q2 >>= 8;                  // < 2^19: a square below 2^38, e below 2^51
      const int64_t mark = (int64_t)i1 * i1 + (int64_t)q1 * q1, space = (int64_t)i2 * i2 + (int64_t)q2 * q2;
      const int64_t e = mark * 256 - space * (int64_t)boost[r];
      const uint64_t pos = __ballot(e > 0), neg = __ballot(e < 0);
      if (k == 0) {
        const int sh = (t & 32) ? 32 : 0;
        sign[2 * r] = (uint32_t)(pos >> sh);
        sign[2 * r + 1] = (uint32_t)(neg >> sh);
      }
    }
    __syncthreads();

    // steps 3 to 6
    if (live) {
      const uint32_t pos = sign[2 * t], neg = sign[2 * t + 1];
      asdr_packet_state_t *rec = a.state + oc;
      for (int k = 0; k < 32; k++) {
        const uint32_t nbit = (pos >> k) & 1u ? 1u : ((neg >> k) & 1u ? 0u : bit);
        const bool edge = nbit != bit;
        const int r = clk < ASDR_PACKET_HALF ? (int)clk : (int)clk - ASDR_PACKET_CLOCK;
        int moved = (int)clk - (r >> 2);                       // 0 .. 147
        moved = moved >= ASDR_PACKET_CLOCK ? moved - ASDR_PACKET_CLOCK : moved;
        clk = edge ? (uint32_t)moved : clk;
        edges += edge ? 1u : 0u;
        bit = nbit;
        const uint32_t p = clk;
        clk += 16;
        const bool take = p < ASDR_PACKET_HALF && clk >= ASDR_PACKET_HALF;
        clk = clk >= ASDR_PACKET_CLOCK ? clk - ASDR_PACKET_CLOCK : clk;
        if (!take) continue;
        const uint32_t v = bit == prev ? 1u : 0u;              // step 4
        prev = bit;
        bits++;
        sr = (sr >> 1) | (v << 7);                             // step 5
        if (sr == 0x7Eu) {
          flags++;
          if (in_frame && nb == 7 && len >= ASDR_PACKET_MIN_LEN) {
            if (crc == 0xF0B8u) {                              // step 6
              const int n = (int)len - 2;
              if (head - taken == a.ring) { taken++; lost++; }
              uint4 *dst = (uint4 *)(a.slots + (size_t)oc * a.ring + head % a.ring);
              const uint4 *src = (const uint4 *)rec->buf;
              dst[0] = make_uint4((uint32_t)oc, frames, a.block0 + (uint32_t)b, (uint32_t)n);
              for (int q = 0; q < (int)sizeof(rec->buf) / 16; q++) {
                const uint4 w = src[q];
                dst[1 + q] = make_uint4(payload_word(w.x, 16 * q, n), payload_word(w.y, 16 * q + 4, n), payload_word(w.z, 16 * q + 8, n),
                                        payload_word(w.w, 16 * q + 12, n));
              }
              frames++; head++;
            } else {
              crc_errors++;
            }
          }
          in_frame = 1; nb = 0; cur = 0; len = 0; crc = 0xFFFFu;
        } else if (sr == 0xFEu) {
          if (in_frame && len > 0) aborts++;
          in_frame = 0;
        } else if ((sr & 0xFCu) == 0x7Cu) {
        } else if (in_frame) {
          cur |= v << nb;
          nb++;
          if (nb == 8) {
            if (len == ASDR_PACKET_MAX_LEN) {
              in_frame = 0;
            } else {
              rec->buf[len++] = (uint8_t)cur;
#pragma unroll
              for (int s = 0; s < 8; s++) crc = (crc >> 1) ^ (((crc ^ (cur >> s)) & 1u) ? 0x8408u : 0u);
            }
            cur = 0; nb = 0;
          }
        }
      }
    }
  }

  // the last block's half of the ring was complete before that block's first barrier, its d before the second
  const int last_half = (a.n_blocks - 1) & 1;
  for (int i = t; i < 2 * ROWS; i += ASDR_PACKET_THREADS) {
    const int r = i >> 1, q = i & 1;
    if (c0 + r > last_c) continue;
    uint4 v;
    if (q == 0) {
      const uint32_t *d = ring + r * ASDR_PACKET_RING_PITCH + 64 * last_half + 60;
      v = make_uint4(d[0], d[1], d[2], d[3]);
    } else {
      const int *d = dring + r * ASDR_PACKET_D_PITCH + 32 * last_half + 24;
      v = make_uint4(pack16(d[0], d[1]), pack16(d[2], d[3]), pack16(d[4], d[5]), pack16(d[6], d[7]));
    }
    ((uint4 *)(a.state + c0 + r))[q] = v;
  }
  if (live) {
    uint4 *rec = (uint4 *)(a.state + oc);
    rec[2] = make_uint4(bits, edges, flags, frames);
    rec[3] = make_uint4(crc_errors, aborts, clk | (len << 16), crc | (bit << 16) | (prev << 24));
    rec[4] = make_uint4(sr | (cur << 8) | (nb << 16) | (in_frame << 24), 0u, 0u, 0u);
    const uint32_t turns = taken / a.ring * a.ring;           // kept reduced: the same slots, taken below ring
    *(uint4 *)(a.rings + oc) = make_uint4(head - turns, taken - turns, lost, 0u);
  }
}

// grid n_tiles: lane = channel
__global__ __launch_bounds__(ASDR_PACKET_TILE) void asdr_packet_count_kernel(PacketCollectArgs a) {
  const int c = blockIdx.x * ASDR_PACKET_TILE + threadIdx.x;
  uint32_t s = 0;
  if (c < a.n_channels) {
    const uint4 g = *(const uint4 *)(a.rings + c);
    s = g.x - g.y;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  uint32_t below, total;
  wave_totals(s, below, total);
  if (threadIdx.x == 0) a.tile_count[blockIdx.x] = total;
}

// grid n_tiles: lane = channel
__global__ __launch_bounds__(ASDR_PACKET_TILE) void asdr_packet_index_kernel(PacketCollectArgs a) {
  __shared__ uint32_t before[ASDR_PACKET_TILE / 64];
  const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = tile * ASDR_PACKET_TILE + threadIdx.x;
  uint32_t s = 0;
  for (int k = threadIdx.x; k < tile; k += ASDR_PACKET_TILE) s += a.tile_count[k];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  if (lane == 0) before[wave] = s;
  uint32_t head = 0, taken = 0, lost = 0, pending = 0;
  if (c < a.n_channels) {
    const uint4 g = *(const uint4 *)(a.rings + c);
    head = g.x; taken = g.y; lost = g.z; pending = g.x - g.y;
  }
  uint32_t scan = pending;                                     // the wave's inclusive scan
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = __shfl_up(scan, d);
    if (lane >= d) scan += up;
  }
  uint32_t below, total;
  wave_totals(__shfl(scan, 63), below, total);                 // its barrier covers `before` too
  const uint64_t first = (uint64_t)before[0] + before[1] + before[2] + before[3];
  const uint64_t pos = first + below + (scan - pending), limit = (uint64_t)a.max_frames;
  const uint32_t deliver = pos >= limit ? 0u : (uint32_t)min((uint64_t)pending, limit - pos);
  for (uint32_t j = 0; j < deliver; j++) a.index[pos + j] = (uint32_t)c * a.ring + (taken + j) % a.ring;
  if (deliver) {
    const uint32_t turns = (taken + deliver) / a.ring * a.ring;   // kept reduced: the same slots, taken below ring
    *(uint4 *)(a.rings + c) = make_uint4(head - turns, taken + deliver - turns, lost, 0u);
  }
  if (tile == (int)gridDim.x - 1 && threadIdx.x == 0) *a.count = (uint32_t)min(first + total, limit);
}

// grid ceil(min(max_frames, n_channels * ring) / 11): a workgroup moves 11 slots, a lane one 16-byte piece of one
__global__ __launch_bounds__(ASDR_PACKET_TILE) void asdr_packet_copy_kernel(PacketCollectArgs a) {
  const uint32_t s = threadIdx.x / ASDR_PACKET_SLOT_PIECES, k = threadIdx.x - s * ASDR_PACKET_SLOT_PIECES;
  if (s >= ASDR_PACKET_SLOTS_PER_GROUP) return;
  const uint64_t row = (uint64_t)blockIdx.x * ASDR_PACKET_SLOTS_PER_GROUP + s;
  if (row >= *a.count) return;
  const uint4 *src = (const uint4 *)(a.slots + a.index[row]);
  ((uint4 *)(a.frames + row))[k] = src[k];
}

// grid ceil(n_channels / 256): lane = channel; what asdr_packet_clear zeroes
__global__ __launch_bounds__(ASDR_PACKET_TILE) void asdr_packet_clear_kernel(asdr_packet_state_t *state, PacketRing *rings, int32_t n_channels) {
  const int c = blockIdx.x * ASDR_PACKET_TILE + threadIdx.x;
  if (c >= n_channels) return;
  asdr_packet_state_t *s = state + c;
  s->bits = 0; s->edges = 0; s->flags = 0; s->crc_errors = 0; s->aborts = 0;
  rings[c].lost = 0;
}

extern "C" int asdr_launch_packet(const PacketArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0 || a->n_blocks <= 0) return 0;
  if (a->n_channels >= ASDR_PACKET_WIDE_CHANNELS) {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_PACKET_ROWS - 1) / ASDR_PACKET_ROWS);
    hipLaunchKernelGGL(asdr_packet_kernel<ASDR_PACKET_ROWS>, grid, dim3(ASDR_PACKET_THREADS), 0, stream, *a);
  } else {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_PACKET_NARROW_ROWS - 1) / ASDR_PACKET_NARROW_ROWS);
    hipLaunchKernelGGL(asdr_packet_kernel<ASDR_PACKET_NARROW_ROWS>, grid, dim3(ASDR_PACKET_THREADS), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_packet_collect(const PacketCollectArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0) return 0;
  const uint32_t n_tiles = ((uint32_t)a->n_channels + ASDR_PACKET_TILE - 1) / ASDR_PACKET_TILE;
  hipLaunchKernelGGL(asdr_packet_count_kernel, dim3(n_tiles), dim3(ASDR_PACKET_TILE), 0, stream, *a);
  hipLaunchKernelGGL(asdr_packet_index_kernel, dim3(n_tiles), dim3(ASDR_PACKET_TILE), 0, stream, *a);
  const uint64_t most = (uint64_t)a->n_channels * a->ring, rows = (uint64_t)a->max_frames < most ? (uint64_t)a->max_frames : most;
  if (rows > 0) {
    const dim3 grid((uint32_t)((rows + ASDR_PACKET_SLOTS_PER_GROUP - 1) / ASDR_PACKET_SLOTS_PER_GROUP));
    hipLaunchKernelGGL(asdr_packet_copy_kernel, grid, dim3(ASDR_PACKET_TILE), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_packet_clear(asdr_packet_state_t *state, PacketRing *rings, int32_t n_channels, void *stream_) {
  if (n_channels <= 0) return 0;
  const uint32_t n_tiles = ((uint32_t)n_channels + ASDR_PACKET_TILE - 1) / ASDR_PACKET_TILE;
  hipLaunchKernelGGL(asdr_packet_clear_kernel, dim3(n_tiles), dim3(ASDR_PACKET_TILE), 0, (hipStream_t)stream_, state, rings, n_channels);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
