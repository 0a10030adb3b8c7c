// asdr_fm_device.h -- what asdr_fm_host.cpp and asdr_fm.hip share: the kernel's argument block and launch entry.
#ifndef ASDR_FM_DEVICE_H_
#define ASDR_FM_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_fm.h"

#define ASDR_FM_THREADS 256      // four waves: the pointwise part's lanes
#define ASDR_FM_ROWS 64          // channels per workgroup: one lane of wave 0 each in the recurrence part
#define ASDR_FM_NARROW_ROWS 16   // ... of a bank below ASDR_FM_WIDE_CHANNELS channels: four times the workgroups
#define ASDR_FM_WIDE_CHANNELS 32768   // 512 workgroups of 64 channels: two per CU
#define ASDR_FM_CHUNK_BLOCKS 1   // blocks of a row staged in LDS at a time
#define ASDR_FM_PITCH 65         // words per staged row: 64 (128 int16) + 1, odd, so the 64 rows' words of one offset fall into different banks
#define ASDR_FM_CORDIC_ITERS 20

struct FmSetting {   // one channel's settings, 32 bytes
  uint64_t open_noise, close_noise;
  uint32_t gain, deemphasis;
  uint32_t hang_blocks, hp_shift;
};

struct FmArgs {
  const int16_t *i, *q;        // [n_channels][in_stride_blocks][128]
  int16_t *out;                // [n_channels][out_stride_blocks][128]
  int64_t in_stride_blocks, out_stride_blocks;
  int32_t n_channels, n_blocks;
  const FmSetting *set;        // [n_channels]
  asdr_fm_state_t *state;      // [n_channels]
};

extern "C" int asdr_launch_fm(const FmArgs *a, void *stream);

#endif
