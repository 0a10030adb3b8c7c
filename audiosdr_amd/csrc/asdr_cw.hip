// asdr_cw.hip -- the CW decoder's kernels (include/asdr_cw.h): the mixer to the pitch, the envelope, the key with its glitch filter,
// the dot / dash decision with the speed tracker, the gaps and the Morse table on int16 audio rows, and the ascending compact
// delivery of the decoded characters.  A deployment that creates no CW decoder launches nothing from this file.
//
// Form of the pass, after the packet decoder's.  A workgroup of four waves owns ROWS channels -- 64 in a bank of
// ASDR_CW_WIDE_CHANNELS channels or more, 16 in a smaller one, which so fills more of the chip -- and walks their rows one
// 128-sample block at a time:
//  * Mixer (step 1), lanes across samples: a lane takes one 16-byte piece (8 samples) of a row, the 16 lanes of a row its 16 pieces,
//    the workgroup 16 rows a pass, ROWS / 16 passes.  A lane keeps the phase of its first sample per pass (the row's ph + 8 piece
//    pitch_step, + 128 pitch_step a block) and steps it 8 times; a table word (LDS, 4 KiB: C[j] and C[(j - 256) & 1023] in one word)
//    gives both products of a sample.  The four lanes of a sub-block add their sums over the quad (two DPP moves); the quad's first
//    lane writes aI, aQ to the row's four places of the block.  The next block's loads are issued before the current block's work.
//  * Steps 2 to 7, a lane of wave 0 per channel: four short steps a block on the row's four (aI, aQ).  The places are double
//    buffered by the block's parity, so a block costs one barrier.  An event is written to its ring slot by its lane, 16 bytes.
//  * State: the first 64 bytes of a record are read once before the first block and written once behind the last, in 16-byte
//    accesses; so are the channel's settings and ring bookkeeping.
// Rows past n_channels in the last workgroup read channel n_channels - 1 again and write nothing.
//
// Form of the collect (the packet decoder's): count sums the events waiting in each tile of 256 channels; index gives every channel
// its position in the ascending order (the tiles before it, then a scan inside the tile), cuts at max_events, lists the ring slots
// of the delivered events, advances taken and writes the count; copy moves the listed slots, a lane an event.
#include <hip/hip_runtime.h>

#include "asdr_cw_device.h"

namespace {

__device__ inline int lo16(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ inline int hi16(uint32_t w) { return (int)w >> 16; }

// v + the v of the three other lanes of the quad
__device__ inline int quad_sum(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  return v;
}

// the sum over the workgroup's four waves of a per-lane value, and the sum over the waves below this one (every thread calls it)
__device__ inline void wave_totals(uint32_t wave_sum, uint32_t &below, uint32_t &total) {
  __shared__ uint32_t sums[ASDR_CW_TILE / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sums[wave] = wave_sum;
  __syncthreads();
  below = 0; total = 0;
#pragma unroll
  for (int w = 0; w < ASDR_CW_TILE / 64; w++) {
    if (w < wave) below += sums[w];
    total += sums[w];
  }
}

}  // namespace

// grid ceil(n_channels / ROWS), 256 lanes
template <int ROWS>
__global__ __launch_bounds__(ASDR_CW_THREADS) void asdr_cw_kernel(CwArgs a) {
  constexpr int PASSES = ROWS / 16;
  __shared__ __align__(16) uint32_t table[ASDR_CW_TABLE_WORDS];
  __shared__ uint32_t row_ph[ROWS], row_step[ROWS];
  __shared__ __align__(16) int2 part[2][ROWS * 4];                           // [block & 1][row][sub-block]: aI, aQ
  const int t = threadIdx.x, piece = t & 15, sub = t >> 4;     // in pass p the lane takes piece `piece` of row 16 p + sub
  const int c0 = blockIdx.x * ROWS, last_c = a.n_channels - 1;

  ((uint4 *)table)[t] = ((const uint4 *)a.table)[t];

  // steps 2 to 7's channel: wave 0, lane t
  const bool owner = t < ROWS, live = owner && c0 + t <= last_c;
  const int oc = min(c0 + t, last_c);
  uint32_t ph = 0, hi = 0, lo = 0, D = ASDR_CW_MIN_D, run = 0, marks = 0, chars = 0, unknown = 0, glitches = 0, cnt = 0, key = 0, sym = 1, gap = 0;
  uint32_t step = 0, min_power = 0, glitch = 1, track = 0, head = 0, taken = 0, lost = 0;
  int pi0 = 0, pi1 = 0, pi2 = 0, pq0 = 0, pq1 = 0, pq2 = 0;    // the last three aI and aQ, the newest last
  if (owner) {
    const uint4 *rec = (const uint4 *)(a.state + oc);
    const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    ph = r0.x; pi0 = (int)r0.y; pi1 = (int)r0.z; pi2 = (int)r0.w;
    pq0 = (int)r1.x; pq1 = (int)r1.y; pq2 = (int)r1.z; hi = r1.w;
    lo = r2.x; D = r2.y; run = r2.z; marks = r2.w;
    chars = r3.x; unknown = r3.y; glitches = r3.z;
    cnt = r3.w & 0xFFu; key = (r3.w >> 8) & 1u; sym = (r3.w >> 16) & 0xFFu; gap = (r3.w >> 24) & 1u;
    const uint4 s = *(const uint4 *)(a.set + oc);
    step = s.x; min_power = s.y; glitch = s.z; track = s.w;
    const uint4 g = *(const uint4 *)(a.rings + oc);
    head = g.x; taken = g.y; lost = g.z;
    row_ph[t] = ph; row_step[t] = step;
  }
  __syncthreads();

  uint32_t lane_ph[PASSES], lane_step[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; p++) {
    lane_step[p] = row_step[16 * p + sub];
    lane_ph[p] = row_ph[16 * p + sub] + 8u * (uint32_t)piece * lane_step[p];
  }

  uint4 next_x[PASSES];
  auto request = [&](int b) {
#pragma unroll
    for (int p = 0; p < PASSES; p++)
      next_x[p] = *(const uint4 *)(a.in + (((int64_t)min(c0 + 16 * p + sub, last_c) * a.in_stride_blocks + b) * 128 + 8 * piece));
  };
  request(0);

  asdr_cw_event_t *const slots = a.slots + (size_t)oc * a.ring;
  for (int b = 0; b < a.n_blocks; b++) {
    uint4 x[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; p++) x[p] = next_x[p];
    if (b + 1 < a.n_blocks) request(b + 1);

    // step 1
#pragma unroll
    for (int p = 0; p < PASSES; p++) {
      const uint32_t w[4] = {x[p].x, x[p].y, x[p].z, x[p].w};
      uint32_t phase = lane_ph[p];
      int si = 0, sq = 0;                                      // |sum| <= 32 * 2^15 * 2^10 = 2^30 over the quad
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int xv = (i & 1) ? hi16(w[i >> 1]) : lo16(w[i >> 1]);
        const uint32_t cs = table[phase >> 22];
        si += xv * lo16(cs); sq += xv * hi16(cs);
        phase += lane_step[p];
      }
      lane_ph[p] += 128u * lane_step[p];
      si = quad_sum(si); sq = quad_sum(sq);
      if ((piece & 3) == 0) part[b & 1][(16 * p + sub) * 4 + (piece >> 2)] = make_int2(si >> 10, sq >> 10);
    }
    __syncthreads();

    // steps 2 to 7
    if (live) {
      const int4 *pp = (const int4 *)&part[b & 1][4 * t];
      const int4 p01 = pp[0], p23 = pp[1];
      const int ai[4] = {p01.x, p01.z, p23.x, p23.z}, aq[4] = {p01.y, p01.w, p23.y, p23.w};
      auto emit = [&](uint32_t ch, uint32_t sym_field, uint32_t flags) {
        if (head - taken == a.ring) { taken++; lost++; }
        const uint32_t wpm = (ASDR_CW_DIT_UNITS + D / 2) / D;
        *(uint4 *)(slots + head % a.ring) = make_uint4((uint32_t)oc, chars, a.block0 + (uint32_t)b, ch | (wpm << 8) | (sym_field << 16) | (flags << 24));
        chars++; head++;
      };
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int iw = ai[q] + pi0 + pi1 + pi2, qw = aq[q] + pq0 + pq1 + pq2;          // |.| <= 2^22
        pi0 = pi1; pi1 = pi2; pi2 = ai[q]; pq0 = pq1; pq1 = pq2; pq2 = aq[q];
        const uint32_t P = (uint32_t)(((int64_t)iw * iw + (int64_t)qw * qw) >> 14);   // <= 2^31
        hi = P > hi ? hi + ((P - hi) >> ASDR_CW_FAST_SHIFT) : hi - ((hi - P) >> ASDR_CW_SLOW_SHIFT);     // step 3
        lo = P < lo ? lo - ((lo - P) >> ASDR_CW_FAST_SHIFT) : lo + ((P - lo) >> ASDR_CW_SLOW_SHIFT);
        const uint32_t span = hi > lo ? hi - lo : 0u;
        const uint32_t r = span > 0 && P >= min_power && P > lo + (span >> (key ? 3 : 2)) ? 1u : 0u;
        run++;                                                                         // step 4
        if (r != key) {
          cnt++;
        } else {
          glitches += cnt > 0 ? 1u : 0u;
          cnt = 0;
        }
        if (cnt == glitch) {
          const uint32_t L = run - glitch, old = key;
          key = r; run = glitch; cnt = 0;
          if (old == 1) {                                                              // step 5
            marks++;
            const int64_t l16 = (int64_t)L * 16;
            const bool dash = l16 >= 2 * (int64_t)D;
            sym = (sym >= 128 || sym == 0) ? 0u : 2 * sym + (dash ? 1u : 0u);
            if (track) {
              const int64_t d = (int64_t)D + (((dash ? l16 / 3 : l16) - (int64_t)D) >> 3);
              D = (uint32_t)min(max(d, (int64_t)ASDR_CW_MIN_D), (int64_t)ASDR_CW_MAX_D);
            }
          }
        }
        if (key == 0) {                                                                // step 6
          const uint64_t s16 = (uint64_t)run * 16;
          if (sym != 1 && s16 >= 2 * (uint64_t)D) {
            const uint32_t ch = ASDR_CW_TABLE[sym];                                    // step 7
            if (ch == 0) { unknown++; emit('?', sym, ASDR_CW_FLAG_UNKNOWN); }
            else emit(ch, sym, 0);
            sym = 1; gap = 1;
          }
          if (gap == 1 && s16 >= 5 * (uint64_t)D) {
            emit(' ', 1, 0);
            gap = 0;
          }
        }
      }
    }
  }

  if (live) {
    uint4 *rec = (uint4 *)(a.state + oc);
    rec[0] = make_uint4(ph + 128u * (uint32_t)a.n_blocks * step, (uint32_t)pi0, (uint32_t)pi1, (uint32_t)pi2);
    rec[1] = make_uint4((uint32_t)pq0, (uint32_t)pq1, (uint32_t)pq2, hi);
    rec[2] = make_uint4(lo, D, run, marks);
    rec[3] = make_uint4(chars, unknown, glitches, cnt | (key << 8) | (sym << 16) | (gap << 24));
    const uint32_t turns = taken / a.ring * a.ring;           // kept reduced: the same slots, taken below ring
    *(uint4 *)(a.rings + oc) = make_uint4(head - turns, taken - turns, lost, 0u);
  }
}

// grid n_tiles: lane = channel
__global__ __launch_bounds__(ASDR_CW_TILE) void asdr_cw_count_kernel(CwCollectArgs a) {
  const int c = blockIdx.x * ASDR_CW_TILE + threadIdx.x;
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
__global__ __launch_bounds__(ASDR_CW_TILE) void asdr_cw_index_kernel(CwCollectArgs a) {
  __shared__ uint32_t before[ASDR_CW_TILE / 64];
  const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = tile * ASDR_CW_TILE + threadIdx.x;
  uint32_t s = 0;
  for (int k = threadIdx.x; k < tile; k += ASDR_CW_TILE) s += a.tile_count[k];
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
  const uint64_t pos = first + below + (scan - pending), limit = (uint64_t)a.max_events;
  const uint32_t deliver = pos >= limit ? 0u : (uint32_t)min((uint64_t)pending, limit - pos);
  for (uint32_t j = 0; j < deliver; j++) a.index[pos + j] = (uint32_t)c * a.ring + (taken + j) % a.ring;
  if (deliver) {
    const uint32_t turns = (taken + deliver) / a.ring * a.ring;   // kept reduced: the same slots, taken below ring
    *(uint4 *)(a.rings + c) = make_uint4(head - turns, taken + deliver - turns, lost, 0u);
  }
  if (tile == (int)gridDim.x - 1 && threadIdx.x == 0) *a.count = (uint32_t)min(first + total, limit);
}

// grid ceil(min(max_events, n_channels * ring) / 256): a lane moves one 16-byte event
__global__ __launch_bounds__(ASDR_CW_TILE) void asdr_cw_copy_kernel(CwCollectArgs a) {
  const uint64_t row = (uint64_t)blockIdx.x * ASDR_CW_TILE + threadIdx.x;
  if (row >= *a.count) return;
  *(uint4 *)(a.events + row) = *(const uint4 *)(a.slots + a.index[row]);
}

// grid ceil(n_channels / 256): lane = channel; what asdr_cw_clear zeroes
__global__ __launch_bounds__(ASDR_CW_TILE) void asdr_cw_clear_kernel(asdr_cw_state_t *state, CwRing *rings, int32_t n_channels) {
  const int c = blockIdx.x * ASDR_CW_TILE + threadIdx.x;
  if (c >= n_channels) return;
  asdr_cw_state_t *s = state + c;
  s->marks = 0; s->unknown = 0; s->glitches = 0;
  rings[c].lost = 0;
}

extern "C" int asdr_launch_cw(const CwArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0 || a->n_blocks <= 0) return 0;
  if (a->n_channels >= ASDR_CW_WIDE_CHANNELS) {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_CW_ROWS - 1) / ASDR_CW_ROWS);
    hipLaunchKernelGGL(asdr_cw_kernel<ASDR_CW_ROWS>, grid, dim3(ASDR_CW_THREADS), 0, stream, *a);
  } else {
    const dim3 grid(((uint32_t)a->n_channels + ASDR_CW_NARROW_ROWS - 1) / ASDR_CW_NARROW_ROWS);
    hipLaunchKernelGGL(asdr_cw_kernel<ASDR_CW_NARROW_ROWS>, grid, dim3(ASDR_CW_THREADS), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_cw_collect(const CwCollectArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->n_channels <= 0) return 0;
  const uint32_t n_tiles = ((uint32_t)a->n_channels + ASDR_CW_TILE - 1) / ASDR_CW_TILE;
  hipLaunchKernelGGL(asdr_cw_count_kernel, dim3(n_tiles), dim3(ASDR_CW_TILE), 0, stream, *a);
  hipLaunchKernelGGL(asdr_cw_index_kernel, dim3(n_tiles), dim3(ASDR_CW_TILE), 0, stream, *a);
  const uint64_t most = (uint64_t)a->n_channels * a->ring, rows = (uint64_t)a->max_events < most ? (uint64_t)a->max_events : most;
  if (rows > 0) {
    const dim3 grid((uint32_t)((rows + ASDR_CW_TILE - 1) / ASDR_CW_TILE));
    hipLaunchKernelGGL(asdr_cw_copy_kernel, grid, dim3(ASDR_CW_TILE), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_cw_clear(asdr_cw_state_t *state, CwRing *rings, int32_t n_channels, void *stream_) {
  if (n_channels <= 0) return 0;
  const uint32_t n_tiles = ((uint32_t)n_channels + ASDR_CW_TILE - 1) / ASDR_CW_TILE;
  hipLaunchKernelGGL(asdr_cw_clear_kernel, dim3(n_tiles), dim3(ASDR_CW_TILE), 0, (hipStream_t)stream_, state, rings, n_channels);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
