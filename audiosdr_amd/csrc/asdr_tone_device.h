// asdr_tone_device.h -- what asdr_tone_host.cpp and asdr_tone.hip share: the kernel's argument block and launch entry.
#ifndef ASDR_TONE_DEVICE_H_
#define ASDR_TONE_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_tone.h"

#define ASDR_TONE_THREADS 256     // four waves
#define ASDR_TONE_ROWS 16         // channels per workgroup: 16 lanes of a row's 16-byte pieces each; a lane of wave 0 each in the recurrence
#define ASDR_TONE_WAVE_ROWS 4     // channels per wave in the correlation: lanes across the 64 table slots
#define ASDR_TONE_RING_PITCH 129  // words per row of the sample ring: two blocks (128 words) + 1, odd
#define ASDR_TONE_OUT_PITCH 65    // words per staged output row: 64 + 1, odd
#define ASDR_TONE_TABLE 1024      // entries of the cosine table

struct ToneSetting {   // one channel's settings, 16 bytes
  uint64_t min_power;
  int32_t want;
  uint32_t hang_windows;
};

struct ToneArgs {
  const int16_t *in;           // [n_channels][in_stride_blocks][128]
  int16_t *out;                // [n_channels][out_stride_blocks][128]
  int64_t in_stride_blocks, out_stride_blocks;
  int32_t n_channels, n_blocks;
  int32_t n_tones, window, dominance, sections;
  int32_t coef[ASDR_TONE_MAX_SECTIONS][5];   // b0, b1, b2, a1, a2 in Q28
  const uint32_t *steps;       // [64]: the phase steps, 0 from n_tones on
  const uint32_t *table;       // [1024]: C[j] & 0xFFFF | C[(j - 256) & 1023] << 16
  const ToneSetting *set;      // [n_channels]
  asdr_tone_state_t *state;    // [n_channels]
};

extern "C" int asdr_launch_tone(const ToneArgs *a, void *stream);

#endif
