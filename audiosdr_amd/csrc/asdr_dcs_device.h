// asdr_dcs_device.h -- what asdr_dcs_host.cpp and asdr_dcs.hip share: the kernel's argument block and launch entry.
#ifndef ASDR_DCS_DEVICE_H_
#define ASDR_DCS_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_dcs.h"

#define ASDR_DCS_THREADS 256          // four waves
#define ASDR_DCS_ROWS 64              // channels per workgroup: one lane of wave 0 each in the slicer, clock and register
#define ASDR_DCS_NARROW_ROWS 16       // ... of a bank below ASDR_DCS_WIDE_CHANNELS channels: four times the workgroups
#define ASDR_DCS_WIDE_CHANNELS 32768  // 512 workgroups of 64 channels: two per CU
#define ASDR_DCS_RING_PITCH 129       // words per row of the sample ring: two blocks (128 words) + 1, odd
#define ASDR_DCS_D_PITCH 33           // words per row of the ring of decimated values: four blocks (32) + 1, odd
#define ASDR_DCS_S_PITCH 9            // words per row of a block's bit-filter outputs: 8 + 1, odd
#define ASDR_DCS_HALF 1312            // a bit is taken where clk passes it; an edge below it pulls the clock back, from it on forward

struct DcsSetting {   // one channel's settings, 8 bytes
  int32_t want;
  uint32_t hysteresis;
};

struct DcsArgs {
  const int16_t *in;           // [n_channels][in_stride_blocks][128]
  int16_t *out;                // [n_channels][out_stride_blocks][128]
  int64_t in_stride_blocks, out_stride_blocks;
  int32_t n_channels, n_blocks;
  int32_t n_codes, max_errors, confirm, hold_bits;
  const uint32_t *table;       // [128]: the words, 0 from n_codes on
  const DcsSetting *set;       // [n_channels]
  asdr_dcs_state_t *state;     // [n_channels]
};

extern "C" int asdr_launch_dcs(const DcsArgs *a, void *stream);

#endif
