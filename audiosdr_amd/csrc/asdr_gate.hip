// asdr_gate.hip -- the audio gate's kernels (include/asdr_gate.h): block energy and peak of every receiver's audio, the squelch
// recurrence, the ascending list of the channels a call delivers, and the packet of their rows.  A deployment that creates no gate
// launches nothing from this file.
//
// Form:
//  * energy: parallel over (channel, block).  A workgroup of four waves owns a tile of 256 channels of one block.  A wave walks its
//    64 channels in eight steps of 8 channels; in a step the 8 lanes of a channel sit on adjacent 16-byte pieces of its 256-byte
//    block (the row access rule of DESIGN.md 2), two 16-byte loads per lane.  A lane squares its 16 samples two at a time into a
//    uint32 (two squares are at most 2^31) and adds those in 64 bits; the 8-lane sum and maximum go through three DPP steps inside
//    the row.  Lane j of a group keeps the result of step j, so after the eight steps every lane holds E and P of one channel (a
//    fixed permutation of the wave's 64) and writes them as one word, P << 48 | E, to the scratch [block][channel].  No LDS, no
//    atomics, plain loads: the chain has just written these rows.
//  * fold: one lane per channel walks the call's blocks in order over the scratch (coalesced), 16 loads in flight at a time (8 for
//    the tail) so that a long call is not one round trip per block, updates the 32-byte state row and writes the channel's
//    delivered flag; the workgroup's number of delivered channels goes to tile_count.  With n_blocks == 1 the energy kernel folds
//    in place (every lane already holds its channel's E and P) and no scratch is touched.
//  * index: workgroup t adds tile_count[0 .. t - 1] (its offset), ranks its own tile's flags (ballot and mbcnt in the wave, four
//    wave totals through LDS) and writes the channel numbers; the last workgroup writes count.  Every slot of index has exactly
//    one writer that depends on nothing but the flags: the same list on every run.
//  * packet: the grid is sized on the host for min(n_channels, capacity_rows) rows; a lane reads count and leaves when its row is
//    past it, else moves one 16-byte piece, neighbouring lanes neighbouring pieces of one row.
#include <hip/hip_runtime.h>

#include "asdr_gate_device.h"

namespace {

// v of another lane of the same row of 16 by a DPP control: quad_perm [1,0,3,2] (lane ^ 1), quad_perm [2,3,0,1] (lane ^ 2),
// row_half_mirror (7 - lane within 8)
constexpr int kQuadXor1 = 0xb1, kQuadXor2 = 0x4e, kHalfMirror = 0x141;

template <int CTRL>
__device__ inline uint32_t dpp32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ inline uint64_t dpp64(uint64_t v) {
  return ((uint64_t)dpp32<CTRL>((uint32_t)(v >> 32)) << 32) | dpp32<CTRL>((uint32_t)v);
}

// Sum / maximum over the aligned group of 8 lanes, left in every lane.  After the two quad steps a quad's lanes agree, so the
// half mirror pairs each lane with one of the other quad.  Every lane of the wave must be active.
__device__ inline uint64_t sum8(uint64_t v) {
  v += dpp64<kQuadXor1>(v);
  v += dpp64<kQuadXor2>(v);
  v += dpp64<kHalfMirror>(v);
  return v;
}
__device__ inline int max8(int v) {
  v = max(v, (int)dpp32<kQuadXor1>((uint32_t)v));
  v = max(v, (int)dpp32<kQuadXor2>((uint32_t)v));
  v = max(v, (int)dpp32<kHalfMirror>((uint32_t)v));
  return v;
}

// the two samples of a word: their squares' sum (at most 2 * 2^30 = 2^31: no carry out of 32 bits) and the larger magnitude
__device__ inline void word(uint32_t w, uint64_t &e, int &p) {
  const int lo = (int)(int16_t)(w & 0xffffu), hi = (int)w >> 16;
  e += (uint64_t)((uint32_t)(lo * lo) + (uint32_t)(hi * hi));
  p = max(p, max(abs(lo), abs(hi)));
}
__device__ inline void piece(uint4 v, uint64_t &e, int &p) {
  word(v.x, e, p); word(v.y, e, p); word(v.z, e, p); word(v.w, e, p);
}

// A channel's state row in registers (asdr_gate_state_t as two 16-byte words).
struct Row {
  uint64_t energy, last;
  int32_t peak;
  uint32_t openings, open_blocks, hang, open;
};
__device__ inline Row load_row(const asdr_gate_state_t *s) {
  const uint4 a = ((const uint4 *)s)[0], b = ((const uint4 *)s)[1];
  Row r;
  r.energy = ((uint64_t)a.y << 32) | a.x; r.last = ((uint64_t)a.w << 32) | a.z;
  r.peak = (int32_t)b.x; r.openings = b.y; r.open_blocks = b.z; r.hang = b.w & 0xffffu; r.open = (b.w >> 16) & 0xffu;
  return r;
}
__device__ inline void store_row(asdr_gate_state_t *s, const Row &r) {
  ((uint4 *)s)[0] = make_uint4((uint32_t)r.energy, (uint32_t)(r.energy >> 32), (uint32_t)r.last, (uint32_t)(r.last >> 32));
  ((uint4 *)s)[1] = make_uint4((uint32_t)r.peak, r.openings, r.open_blocks, r.hang | (r.open << 16));   // reserved byte 0
}

// one block of the recurrence (include/asdr_gate.h); returns open after the block
__device__ inline uint32_t step(Row &r, const GateSetting &t, uint64_t E, int P) {
  if (E >= t.open_energy) {
    r.openings += r.open ^ 1u; r.open = 1u; r.hang = t.hang_blocks;
  } else if (r.open) {
    if (E >= t.close_energy) r.hang = t.hang_blocks;
    else if (r.hang > 0) r.hang--;
    else r.open = 0u;
  }
  r.open_blocks += r.open; r.energy += E; r.last = E; r.peak = max(r.peak, P);
  return r.open;
}

// Blocks b0 .. b0 + live - 1 (live <= K) of one channel: K loads of the scratch in flight, then the steps in block order.  The loads
// past `live` re-read the last live word (no branch between the loads); their steps are skipped.  A lane's chain of dependent
// round trips to the scratch is n_blocks / K long instead of n_blocks.
template <int K>
__device__ inline uint32_t fold_batch(Row &r, const GateSetting &t, const uint64_t *w, int n_channels, int b0, int live) {
  uint64_t v[K];
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = w[(size_t)(b0 + min(k, live - 1)) * n_channels];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < K; k++)
    if (k < live) any |= step(r, t, v[k] & ((1ULL << 48) - 1), (int)(v[k] >> 48));
  return any;
}

// the workgroup's number of lanes with `any` set, to tile_count[tile] (four waves; every thread calls it)
__device__ inline void count_tile(uint32_t any, int32_t *tile_count, int tile) {
  __shared__ int32_t wave_count[ASDR_GATE_TILE / 64];
  const int n = __popcll(__ballot(any != 0));
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[tile] = wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
}

}  // namespace

// grid (n_tiles, n_blocks); FUSED (n_blocks == 1) folds in place.
template <bool FUSED>
__global__ __launch_bounds__(ASDR_GATE_TILE) void asdr_gate_energy_kernel(GateArgs a) {
  const int lane = threadIdx.x & 63, g = lane >> 3, j = lane & 7;
  const int c0 = blockIdx.x * ASDR_GATE_TILE + (threadIdx.x >> 6) * 64;   // the wave's first channel
  const int b = blockIdx.y;
  uint4 v[8][2];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = c0 + 8 * i + g;
    v[i][0] = v[i][1] = make_uint4(0, 0, 0, 0);
    if (c < a.n_channels) {
      const uint4 *p = (const uint4 *)(a.audio + ((int64_t)c * a.stride_blocks + b) * 128);
      v[i][0] = p[j]; v[i][1] = p[j + 8];
    }
  }
  uint64_t E = 0;
  int P = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t e = 0;
    int p = 0;
    piece(v[i][0], e, p); piece(v[i][1], e, p);
    e = sum8(e); p = max8(p);
    if (i == j) { E = e; P = p; }
  }
  const int c = c0 + 8 * j + g;   // the channel whose step this lane kept
  if (FUSED) {
    uint32_t any = 0;
    if (c < a.n_channels) {
      Row r = load_row(a.state + c);
      any = step(r, a.set[c], E, P);
      store_row(a.state + c, r);
      a.flag[c] = (uint8_t)any;
    }
    count_tile(any, a.tile_count, blockIdx.x);
  } else if (c < a.n_channels) {
    a.scr[(size_t)b * a.n_channels + c] = ((uint64_t)P << 48) | E;   // E <= 2^37, P <= 2^15: one word
  }
}

// grid n_tiles: lane = channel
__global__ __launch_bounds__(ASDR_GATE_TILE) void asdr_gate_fold_kernel(GateArgs a) {
  const int c = blockIdx.x * ASDR_GATE_TILE + threadIdx.x;
  uint32_t any = 0;
  if (c < a.n_channels) {
    Row r = load_row(a.state + c);
    const GateSetting t = a.set[c];
    const uint64_t *w = a.scr + c;
    int b = 0;
    for (; b + 16 <= a.n_blocks; b += 16) any |= fold_batch<16>(r, t, w, a.n_channels, b, 16);
    for (; b + 8 <= a.n_blocks; b += 8) any |= fold_batch<8>(r, t, w, a.n_channels, b, 8);
    if (b < a.n_blocks) any |= fold_batch<8>(r, t, w, a.n_channels, b, a.n_blocks - b);
    store_row(a.state + c, r);
    a.flag[c] = (uint8_t)any;
  }
  count_tile(any, a.tile_count, blockIdx.x);
}

// grid n_tiles
__global__ __launch_bounds__(ASDR_GATE_TILE) void asdr_gate_index_kernel(GateArgs a) {
  __shared__ int32_t before[ASDR_GATE_TILE / 64], mine[ASDR_GATE_TILE / 64];
  const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = tile * ASDR_GATE_TILE + threadIdx.x;
  int s = 0;
  for (int k = threadIdx.x; k < tile; k += ASDR_GATE_TILE) s += a.tile_count[k];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
  const bool f = c < a.n_channels && a.flag[c] != 0;
  const uint64_t m = __ballot(f);
  const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  if (lane == 0) { before[wave] = s; mine[wave] = __popcll(m); }
  __syncthreads();
  int offset = before[0] + before[1] + before[2] + before[3], total = 0;
#pragma unroll
  for (int w = 0; w < ASDR_GATE_TILE / 64; w++) {
    if (w < wave) offset += mine[w];
    total += mine[w];
  }
  if (f) a.index[offset + rank] = c;
  if (tile == (int)gridDim.x - 1 && threadIdx.x == 0) *a.count = before[0] + before[1] + before[2] + before[3] + total;
}

// grid (ceil(grid_rows / rows_per_wg), ceil(pieces / 256)): pieces = 16 n_blocks 16-byte pieces per row; a workgroup holds
// rows_per_wg = max(1, 256 / pieces) rows.
__global__ __launch_bounds__(256) void asdr_gate_packet_kernel(GateArgs a, uint32_t pieces, uint32_t rows_per_wg) {
  const uint32_t r = threadIdx.x / pieces, k = threadIdx.x - r * pieces + blockIdx.y * 256u;
  const int64_t row = (int64_t)blockIdx.x * rows_per_wg + r;
  if (r >= rows_per_wg || k >= pieces) return;
  const int32_t n = min(*a.count, a.capacity_rows);
  if (row >= n) return;
  const int32_t c = a.index[row];
  const uint4 *src = (const uint4 *)(a.audio + (int64_t)c * a.stride_blocks * 128);
  uint4 *dst = (uint4 *)a.rows + row * pieces;
  dst[k] = src[k];
}

extern "C" int asdr_launch_gate_pass(const GateArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int n_tiles = (a->n_channels + ASDR_GATE_TILE - 1) / ASDR_GATE_TILE;
  if (a->n_blocks == 1) {
    hipLaunchKernelGGL(asdr_gate_energy_kernel<true>, dim3(n_tiles, 1), dim3(ASDR_GATE_TILE), 0, stream, *a);
  } else {
    hipLaunchKernelGGL(asdr_gate_energy_kernel<false>, dim3(n_tiles, a->n_blocks), dim3(ASDR_GATE_TILE), 0, stream, *a);
    hipLaunchKernelGGL(asdr_gate_fold_kernel, dim3(n_tiles), dim3(ASDR_GATE_TILE), 0, stream, *a);
  }
  hipLaunchKernelGGL(asdr_gate_index_kernel, dim3(n_tiles), dim3(ASDR_GATE_TILE), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_gate_packet(const GateArgs *a, int grid_rows, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (grid_rows <= 0) return 0;
  const uint32_t pieces = 16u * (uint32_t)a->n_blocks, rows_per_wg = pieces >= 256u ? 1u : 256u / pieces;
  const dim3 grid(((uint32_t)grid_rows + rows_per_wg - 1) / rows_per_wg, (pieces + 255u) / 256u);
  hipLaunchKernelGGL(asdr_gate_packet_kernel, grid, dim3(256), 0, stream, *a, pieces, rows_per_wg);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
