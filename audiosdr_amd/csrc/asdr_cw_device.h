// asdr_cw_device.h -- what asdr_cw_host.cpp and asdr_cw.hip share: the kernels' argument blocks and launch entries.
#ifndef ASDR_CW_DEVICE_H_
#define ASDR_CW_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_cw.h"

#define ASDR_CW_THREADS 256          // four waves
#define ASDR_CW_ROWS 64              // channels per workgroup: one lane of wave 0 each in steps 2 to 7
#define ASDR_CW_NARROW_ROWS 16       // ... of a bank below ASDR_CW_WIDE_CHANNELS channels: four times the workgroups
#define ASDR_CW_WIDE_CHANNELS 32768  // 512 workgroups of 64 channels: two per CU
#define ASDR_CW_TABLE_WORDS 1024     // the mixer's table: word j holds C[j] (low half) and C[(j - 256) & 1023] (high half)
#define ASDR_CW_LOADED_BYTES 64      // of a record, what a call loads and stores: everything in front of the reserved fields
#define ASDR_CW_TILE 256             // channels per workgroup of the collect passes; events per workgroup of the copy pass

struct CwRing {   // one channel's ring bookkeeping, 16 bytes: slot k of the channel holds the event whose head was k mod ring.
  uint32_t head, taken, lost, reserved;   // Kept reduced: taken < ring and head - taken <= ring, so neither ever wraps
};

struct CwSetting {   // one channel's settings, 16 bytes
  uint32_t pitch_step, min_power, glitch, track;
};

struct CwArgs {
  const int16_t *in;             // [n_channels][in_stride_blocks][128]
  int64_t in_stride_blocks;
  int32_t n_channels, n_blocks;
  uint32_t ring, block0;         // slots per channel; the low 32 bits of the handle's block count before the call
  const CwSetting *set;          // [n_channels]
  const uint32_t *table;         // [ASDR_CW_TABLE_WORDS], 16-byte aligned
  asdr_cw_state_t *state;        // [n_channels]
  CwRing *rings;                 // [n_channels]
  asdr_cw_event_t *slots;        // [n_channels][ring]
};

struct CwCollectArgs {
  int32_t n_channels, max_events;
  uint32_t ring;
  CwRing *rings;
  const asdr_cw_event_t *slots;
  uint32_t *tile_count;          // [ceil(n_channels / ASDR_CW_TILE)]: the events waiting in a tile
  uint32_t *index;               // [min(max_events, n_channels * ring)]: the slot (channel * ring + k) of every delivered event
  uint32_t *count;               // the caller's
  asdr_cw_event_t *events;       // the caller's
};

extern "C" int asdr_launch_cw(const CwArgs *a, void *stream);
extern "C" int asdr_launch_cw_collect(const CwCollectArgs *a, void *stream);
extern "C" int asdr_launch_cw_clear(asdr_cw_state_t *state, CwRing *rings, int32_t n_channels, void *stream);

#endif
