// asdr_packet_device.h -- what asdr_packet_host.cpp and asdr_packet.hip share: the kernels' argument blocks and launch entries.
#ifndef ASDR_PACKET_DEVICE_H_
#define ASDR_PACKET_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_packet.h"

#define ASDR_PACKET_THREADS 256          // four waves
#define ASDR_PACKET_ROWS 64              // channels per workgroup: one lane of wave 0 each in the slicer, clock, NRZI and HDLC steps
#define ASDR_PACKET_NARROW_ROWS 16       // ... of a bank below ASDR_PACKET_WIDE_CHANNELS channels: four times the workgroups
#define ASDR_PACKET_WIDE_CHANNELS 32768  // 512 workgroups of 64 channels: two per CU
#define ASDR_PACKET_RING_PITCH 129       // words per row of the sample ring: two blocks (128 words) + 1, odd
#define ASDR_PACKET_D_PITCH 65           // words per row of the ring of decimated values: two blocks (64) + 1, odd
#define ASDR_PACKET_HALF 74              // a bit is taken where clk passes it; an edge below it pulls the clock back, from it on forward
#define ASDR_PACKET_LOADED_BYTES 80      // of a record, what a call loads and stores: everything in front of the reserved fields and buf
#define ASDR_PACKET_TILE 256             // channels per workgroup of the collect passes
#define ASDR_PACKET_SLOT_PIECES 22       // 16-byte pieces of a 352-byte slot
#define ASDR_PACKET_SLOTS_PER_GROUP 11   // slots a workgroup of the copy pass moves: 242 of its 256 lanes

struct PacketRing {   // one channel's ring bookkeeping, 16 bytes: slot k of the channel holds the frame whose head was k mod ring.
  uint32_t head, taken, lost, reserved;   // Kept reduced: taken < ring and head - taken <= ring, so neither ever wraps
};

struct PacketArgs {
  const int16_t *in;             // [n_channels][in_stride_blocks][128]
  int64_t in_stride_blocks;
  int32_t n_channels, n_blocks;
  uint32_t ring, block0;         // slots per channel; the low 32 bits of the handle's block count before the call
  const uint32_t *boost;         // [n_channels]
  asdr_packet_state_t *state;    // [n_channels]
  PacketRing *rings;             // [n_channels]
  asdr_packet_frame_t *slots;    // [n_channels][ring]
};

struct PacketCollectArgs {
  int32_t n_channels, max_frames;
  uint32_t ring;
  PacketRing *rings;
  const asdr_packet_frame_t *slots;
  uint32_t *tile_count;          // [ceil(n_channels / ASDR_PACKET_TILE)]: the frames waiting in a tile
  uint32_t *index;               // [min(max_frames, n_channels * ring)]: the slot (channel * ring + k) of every delivered frame
  uint32_t *count;               // the caller's
  asdr_packet_frame_t *frames;   // the caller's
};

extern "C" int asdr_launch_packet(const PacketArgs *a, void *stream);
extern "C" int asdr_launch_packet_collect(const PacketCollectArgs *a, void *stream);
extern "C" int asdr_launch_packet_clear(asdr_packet_state_t *state, PacketRing *rings, int32_t n_channels, void *stream);

#endif
