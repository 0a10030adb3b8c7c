// asdr_codec_device.h -- what asdr_codec_host.cpp and asdr_codec.hip share: the kernels' argument block, the launch entries and the
// IMA step table (the kernel's copy goes to LDS, the host's serves asdr_codec_decode).
#ifndef ASDR_CODEC_DEVICE_H_
#define ASDR_CODEC_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_codec.h"

#define ASDR_CODEC_THREADS 256         // lanes per workgroup of the G.711 pass: a lane takes one 16-byte piece, 8 samples
#define ASDR_CODEC_ROWS 64             // rows per workgroup of the ADPCM pass: one wave, a lane owns a row
#define ASDR_CODEC_CHUNK 64            // samples of a row staged at a time: 8 lanes of a row on 8 adjacent 16-byte pieces
#define ASDR_CODEC_ROW_WORDS 33        // LDS words per staged row: 32 + 1, odd, so 64 lanes reading one offset hit different banks
#define ASDR_CODEC_STEPS 89
#define ASDR_CODEC_GROUP 2             // dwords of nibbles (16 samples) the chain forms between two stores: 4 spills SGPRs

#define ASDR_CODEC_STEP_TABLE                                                                                                              \
  7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157,   \
      173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,  \
      1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635,    \
      13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767

struct CodecArgs {
  const int16_t *rows;         // [..][row_stride] samples
  int64_t row_stride;
  uint8_t *out;                // [..][out_stride] bytes, 4-byte aligned
  int64_t out_stride;          // a multiple of 4
  const int32_t *index;        // NULL: row c is channel c
  const int32_t *count;
  asdr_codec_state_t *state;   // [n_channels]; the ADPCM pass only
  int32_t n_channels, n_samples, grid_rows, capacity_rows;
  int32_t rows_compact;        // with an index: input row i (1) or input row index[i] (0)
  int32_t kind;
  int32_t aligned;             // rows 16-byte aligned and row_stride a multiple of 8: whole pieces are 16-byte loads
  int32_t pieces;              // ceil(n_samples / 8)
};

// mu-law / A-law: grid_rows * pieces lanes
extern "C" int asdr_launch_codec_g711(const CodecArgs *a, void *stream);
// IMA ADPCM: ceil(grid_rows / 64) waves
extern "C" int asdr_launch_codec_adpcm(const CodecArgs *a, void *stream);

#endif
