// asdr_gate_device.h -- what asdr_gate_host.cpp and asdr_gate.hip share: the kernels' argument block and launch entries.
#ifndef ASDR_GATE_DEVICE_H_
#define ASDR_GATE_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_gate.h"

#define ASDR_GATE_TILE 256   // channels per workgroup of the energy, fold and index steps: the tile of the index step's scan

struct GateSetting {   // one channel's squelch, 24 bytes
  uint64_t open_energy, close_energy;
  uint32_t hang_blocks, pad;
};

struct GateArgs {
  const int16_t *audio;        // [n_channels][stride_blocks][128]
  int64_t stride_blocks;
  int32_t n_channels, n_blocks;
  const GateSetting *set;      // [n_channels]
  asdr_gate_state_t *state;    // [n_channels]
  uint64_t *scr;               // [n_blocks][n_channels]: P << 48 | E   (unused by the fused one-block form)
  uint8_t *flag;               // [n_channels]: delivered by this call
  int32_t *tile_count;         // [n_tiles]
  int32_t *count, *index;      // the result
  int16_t *rows;               // the packet, or NULL
  int32_t capacity_rows;
};

// energy (+ fold when n_blocks == 1), fold, index: the whole pass up to count and index
extern "C" int asdr_launch_gate_pass(const GateArgs *a, void *stream);
// the packet: rows 0 .. min(*count, capacity_rows) - 1; the grid is sized for grid_rows rows
extern "C" int asdr_launch_gate_packet(const GateArgs *a, int grid_rows, void *stream);

#endif
