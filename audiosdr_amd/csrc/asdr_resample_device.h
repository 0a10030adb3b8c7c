// asdr_resample_device.h -- what asdr_resample_host.cpp and asdr_resample.hip share: the kernels' argument block and launch entries.
#ifndef ASDR_RESAMPLE_DEVICE_H_
#define ASDR_RESAMPLE_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_resample.h"

#define ASDR_RESAMPLE_THREADS 256      // lanes per workgroup of both kernels
#define ASDR_RESAMPLE_ROWS 64          // rows per workgroup of the pass: a lane of every wave owns one row
#define ASDR_RESAMPLE_WAVES 4          // the waves of a workgroup share its outputs: wave w forms outputs w, w + 4, ... of the tile
#define ASDR_RESAMPLE_PAIR_BATCH 16    // tap words per phase are padded to a multiple of this: one scalar load of 16 words
#define ASDR_RESAMPLE_MAX_LDS 65536    // bytes of windows per workgroup
#define ASDR_RESAMPLE_CARRY_CHANNELS 4 // channels per lane of the carry kernel

struct ResampleArgs {
  const int16_t *audio;        // [n_channels][stride_blocks][128]
  int64_t stride_blocks;
  const int16_t *carry;        // [n_channels][256]: the last 256 samples before this call
  int16_t *carry_next;         // the other half of the double buffer
  int16_t *out;                // [rows][out_stride]
  int64_t out_stride;
  const int32_t *index;        // NULL: row c is channel c
  const int32_t *count;
  const uint32_t *taps;        // [2][up][pairs]: the two pair tables (asdr_resample.hip)
  int32_t n_channels, n_blocks, grid_rows, capacity_rows;
  int32_t up, pairs, shift, round;   // pairs: words per phase, a multiple of ASDR_RESAMPLE_PAIR_BATCH
  int32_t n_out;               // outputs of this call per row
  int32_t phi0, lb0;           // phase of the call's first output, and its b relative to the call's first sample (>= 0)
  int32_t tile_out;            // outputs of a tile
  int32_t tile_q, tile_r;      // tile_out * down = tile_q * up + tile_r
  int32_t q1, r1, q4, r4;      // down = q1 * up + r1, 4 * down = q4 * up + r4: one output on, and one output of the same wave on
  int32_t reach;               // samples behind b that the padded words reach: 2 * pairs + 1
  int32_t pieces;              // 16-byte pieces of a row's window in LDS
  uint32_t pieces_magic;       // ceil(2^32 / pieces): item / pieces = umulhi(item, magic) for item < 65536
  int32_t row_words;           // 4 * pieces + 1: odd, so the 64 rows' words at one offset lie in 64 different banks
};

// the resampling pass over grid_rows rows; dynamic LDS = 64 * row_words * 4 bytes
extern "C" int asdr_launch_resample(const ResampleArgs *a, void *stream);
// every channel's new carry into carry_next
extern "C" int asdr_launch_resample_carry(const ResampleArgs *a, void *stream);

#endif
