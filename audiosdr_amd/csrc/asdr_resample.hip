// asdr_resample.hip -- the audio resampler's kernels (include/asdr_resample.h): the polyphase sums of every delivered row and the
// new carry of every channel.  A deployment that creates no resampler launches nothing from this file.
//
// Form:
//  * The bank is in lockstep, so output j of every row has the same b and the same phase.  A lane owns a ROW and a wave forms one
//    output of 64 rows at a time: the phase's taps are the same in every lane, so they are scalar loads (16 words at once) into
//    SGPRs and the dot instruction takes them as its scalar operand; only the samples come through LDS.
//  * A workgroup is 64 rows x one tile of tile_out outputs; its four waves take outputs w, w + 4, ... of the tile.  The host sizes
//    the tile so that the rows' windows fill at most 64 KiB of LDS (98 outputs at 12 kHz, a whole call when it is shorter), and
//    gives the call's first b and phase and the tile's steps in 64-bit arithmetic; a wave steps from output to output by adding
//    (q4, r4) with a compare, in scalar registers.  The one division (a tile's first phase, 32 bits) is scalar and once per wave.
//  * Staging: each row's window -- `reach` samples of history and the tile's input span -- goes to LDS in aligned 16-byte pieces,
//    neighbouring lanes on neighbouring pieces of one row (the row access rule of DESIGN.md 2); a piece lies wholly in the carry,
//    in the call's blocks, or outside both (zero).  A row takes 4 * pieces + 1 words: with an odd stride the 64 lanes' reads of one
//    offset fall into 64 different banks.
//  * The sums use sdot2 on the aligned words of the window: a word holds x[e], x[e + 1] with e even.  For odd b the words pair
//    (x[b - 2k - 1], x[b - 2k]) and meet table 0, (h[2k + 1], h[2k]); for even b they pair (x[b - 2k], x[b - 2k + 1]) and meet
//    table 1, (h[2k], h[2k - 1]) with h[-1] = 0: a second table, not a second copy of the window.  Both are stored
//    [table][phase][pairs], zero filled to a multiple of 16 words.
//  * carry: a lane moves one 16-byte piece of the new records of four channels, read from the old record or from the call's last
//    two blocks, written to the other half of the double buffer; nothing reads what the same call overwrites.
#include <hip/hip_runtime.h>

#include "asdr_resample_device.h"

namespace {

typedef short short2_t __attribute__((ext_vector_type(2)));

__device__ inline int dot2(uint32_t x, uint32_t h, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, x), __builtin_bit_cast(short2_t, h), acc, false);
}

__device__ inline int sat16(int v) { return min(max(v, -32768), 32767); }

}  // namespace

// grid (tiles, row groups (low 15 bits), row groups (high bits)); dynamic LDS 64 * row_words * 4 bytes
__global__ __launch_bounds__(ASDR_RESAMPLE_THREADS) void asdr_resample_kernel(ResampleArgs a) {
  extern __shared__ uint32_t win[];   // [64][row_words]
  const int tile = blockIdx.x;
  const int row0 = (int)(blockIdx.z * 32768u + blockIdx.y) * ASDR_RESAMPLE_ROWS;
  int rows = a.grid_rows;
  if (a.index) rows = min(rows, min(*a.count, a.capacity_rows));
  if (row0 >= rows) return;                                   // the whole workgroup
  const uint32_t t0 = (uint32_t)a.phi0 + (uint32_t)tile * (uint32_t)a.tile_r;
  const uint32_t wrap0 = t0 / (uint32_t)a.up;                 // scalar
  const int lb = a.lb0 + tile * a.tile_q + (int)wrap0;        // b of the tile's first output, relative to the call's first sample
  const int base = (lb - a.reach) & ~7;                       // first staged sample: a multiple of 8
  const int n_in = a.n_blocks * 128;

  const int staged = ASDR_RESAMPLE_ROWS * a.pieces;
#pragma unroll 2
  for (int w = threadIdx.x; w < staged; w += ASDR_RESAMPLE_THREADS) {
    const int r = (int)__umulhi((uint32_t)w, a.pieces_magic), p = w - r * a.pieces;
    const int row = row0 + r, s = base + 8 * p;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < rows) {
      const int c = a.index ? a.index[row] : row;
      if ((uint32_t)c < (uint32_t)a.n_channels) {
        if (s >= 0) {
          if (s < n_in) v = *(const uint4 *)(a.audio + ((int64_t)c * a.stride_blocks * 128 + s));
        } else if (s >= -256) {
          v = *(const uint4 *)(a.carry + ((int64_t)c * 256 + 256 + s));
        }
      }
    }
    uint32_t *d = win + r * a.row_words + 4 * p;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();

  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int row = row0 + lane;
  const int first = tile * a.tile_out;                        // relative to the call's first output
  const int live = min(a.tile_out, a.n_out - first);
  int phi = (int)(t0 - wrap0 * (uint32_t)a.up), b = lb - base;   // of the wave's output; b as an index into the window, >= reach
  for (int s = 0; s < wave; s++) {
    phi += a.r1; b += a.q1;
    if (phi >= a.up) { phi -= a.up; b++; }
  }
  const uint32_t *x0 = win + lane * a.row_words;
  int16_t *o = a.out + ((int64_t)row * a.out_stride + first);
  for (int i = wave; i < live; i += ASDR_RESAMPLE_WAVES) {
    const uint32_t *t = a.taps + (size_t)(((b & 1) ? 0 : a.up) + phi) * a.pairs;   // the same in every lane
    const uint32_t *x = x0 + (b >> 1);
    int acc = 0;
    for (int k0 = 0; k0 < a.pairs; k0 += ASDR_RESAMPLE_PAIR_BATCH) {
      uint32_t h[ASDR_RESAMPLE_PAIR_BATCH], v[ASDR_RESAMPLE_PAIR_BATCH];
#pragma unroll
      for (int u = 0; u < ASDR_RESAMPLE_PAIR_BATCH; u++) { h[u] = t[k0 + u]; v[u] = x[-(k0 + u)]; }
#pragma unroll
      for (int u = 0; u < ASDR_RESAMPLE_PAIR_BATCH; u++) acc = dot2(v[u], h[u], acc);
    }
    if (row < rows) o[i] = (int16_t)sat16((acc + a.round) >> a.shift);
    phi += a.r4; b += a.q4;
    if (phi >= a.up) { phi -= a.up; b++; }
  }
}

// grid ceil(32 ceil(n_channels / 4) / 256): a lane moves one 16-byte piece of the new records of four neighbouring channels, the four
// loads issued before the first store
__global__ __launch_bounds__(ASDR_RESAMPLE_THREADS) void asdr_resample_carry_kernel(ResampleArgs a) {
  const int64_t w = (int64_t)blockIdx.x * ASDR_RESAMPLE_THREADS + threadIdx.x;
  const int64_t c0 = (w >> 5) * ASDR_RESAMPLE_CARRY_CHANNELS;
  const int p = (int)(w & 31);
  const int s = a.n_blocks * 128 - 256 + 8 * p;               // >= -128: n_blocks >= 1
  uint4 v[ASDR_RESAMPLE_CARRY_CHANNELS];
#pragma unroll
  for (int u = 0; u < ASDR_RESAMPLE_CARRY_CHANNELS; u++) {
    const int64_t c = c0 + u;
    v[u] = make_uint4(0, 0, 0, 0);
    if (c < a.n_channels)
      v[u] = s >= 0 ? *(const uint4 *)(a.audio + (c * a.stride_blocks * 128 + s)) : *(const uint4 *)(a.carry + (c * 256 + 256 + s));
  }
#pragma unroll
  for (int u = 0; u < ASDR_RESAMPLE_CARRY_CHANNELS; u++) {
    const int64_t c = c0 + u;
    if (c < a.n_channels) *(uint4 *)(a.carry_next + (c * 256 + 8 * p)) = v[u];
  }
}

extern "C" int asdr_launch_resample(const ResampleArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->grid_rows <= 0 || a->n_out <= 0) return 0;
  const uint32_t tiles = ((uint32_t)a->n_out + a->tile_out - 1) / a->tile_out;
  const uint32_t groups = ((uint32_t)a->grid_rows + ASDR_RESAMPLE_ROWS - 1) / ASDR_RESAMPLE_ROWS;
  const dim3 grid(tiles, groups < 32768u ? groups : 32768u, (groups + 32767u) / 32768u);
  const size_t lds = (size_t)ASDR_RESAMPLE_ROWS * a->row_words * 4;
  hipLaunchKernelGGL(asdr_resample_kernel, grid, dim3(ASDR_RESAMPLE_THREADS), lds, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_resample_carry(const ResampleArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t groups = ((int64_t)a->n_channels + ASDR_RESAMPLE_CARRY_CHANNELS - 1) / ASDR_RESAMPLE_CARRY_CHANNELS;
  const uint32_t grid = (uint32_t)((groups * 32 + ASDR_RESAMPLE_THREADS - 1) / ASDR_RESAMPLE_THREADS);
  hipLaunchKernelGGL(asdr_resample_carry_kernel, dim3(grid), dim3(ASDR_RESAMPLE_THREADS), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
