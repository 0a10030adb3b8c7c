/* asdr_packet.h -- C ABI of the packet decoder: 1200-baud Bell-202 AFSK carrying AX.25 frames (APRS, packet radio, digipeaters,
 * telemetry beacons) behind the FM demodulator.
 *
 * A stage of its own (libasdr_hip.so, asdr_packet.hip): it reads the int16 audio rows that asdr_fm_update_device writes (or a tone or
 * DCS squelch behind it) and writes no rows: it writes frames, the first stage whose output is decoded data.  A deployment that
 * creates none runs exactly as without this header.  Same conventions as asdr_dcs.h: `ch` = channel index or ASDR_ALL (-1) for the
 * per-channel setter, ASDR_NO_DEVICE for a control-plane-only handle whose signal calls fail, 0 / -1 return codes with
 * asdr_last_error(); a refused call changes nothing.
 *
 * Statement (integers only; tests/packet_ref.py is the independent numpy restatement, and the kernel is held to it bit for bit).
 * ">>" is an arithmetic shift (floor).
 *
 *   Input:  dIn int16 [n_channels][in_stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.  Channel c reads row c.
 *
 *   Per-channel setting (from the next call):
 *     space_boost   uint32 in 64 .. 4096, creation 256: the weight of the 2200 Hz energy against 256 for the 1200 Hz energy.  It
 *                   makes up for a de-emphasised 2200 Hz; FM's a = 32768 (no de-emphasis) is advised for packet channels.
 *
 *   Per block of 128 input samples x, in block order:
 *
 *   1. Decimate by 4 to 11,025 Hz.  d_k = (sum_{j = 0 .. 9} h[j] x[4 k + 3 - j] + 32) >> 6 for k = 0 .. 31, h = 1 3 6 10 12 12 10 6
 *      3 1, the coefficients of (1 + z + z^2 + z^3)^3.  Negative sample indices reach into the channel's previous samples (hist, 6
 *      used, zeros at creation).  d fits int16 (-32768 only for a constant -32768 input).
 *
 *   2. Tone correlators over one bit.  A bit is 147 / 16 = 9.19 decimated samples.  With the tables ASDR_PACKET_C1200 / S1200 /
 *      C2200 / S2200 below (C_f[j] = floor(256 cos(2 pi f j / 11025) + 0.5), S_f likewise with sin, j = 0 .. 8):
 *          I_f = (sum_{j = 0 .. 8} d[n - j] C_f[j]) >> 8,  Q_f likewise with S_f          (the sums fit int32)
 *          e = (I_1200^2 + Q_1200^2) * 256 - (I_2200^2 + Q_2200^2) * space_boost          (int64)
 *      d[n - j] reaches into dhist, the channel's last 8 decimated values (zeros at creation).
 *
 *   3. Slicer and bit clock.  clk runs in 0 .. 146, 16 per decimated sample.  For each of the 32 values in order:
 *          nb = 1 if e > 0, 0 if e < 0, else b
 *          if nb != b:   r = clk if clk < 74 else clk - 147;   clk = (clk - (r >> 2)) mod 147, taken into 0 .. 146;
 *                        b = nb;  edges++
 *          p = clk;  clk += 16;  if p < 74 <= clk: a bit is taken (step 4, with b);  if clk >= 147: clk -= 147
 *      A block takes 3 or 4 bits on an undisturbed clock and at most 5 over every clk and every pattern of edges
 *      (tests/test_packet_ref.py goes through them); the kernel relies on no bound.
 *
 *   4. NRZI.  On a bit: v = (b == prev);  prev = b;  bits++.
 *
 *   5. HDLC, on v.
 *          sr = (sr >> 1) | (v << 7)
 *          if sr == 0x7E:                          flag
 *              flags++
 *              if in_frame and nb == 7 and len >= 17:
 *                  if crc == 0xF0B8: a frame completes (step 6)   else: crc_errors++
 *              in_frame = 1;  nb = 0;  cur = 0;  len = 0;  crc = 0xFFFF
 *          else if sr == 0xFE:                     abort
 *              if in_frame and len > 0: aborts++
 *              in_frame = 0
 *          else if (sr & 0xFC) == 0x7C:            a stuffed zero: nothing
 *          else if in_frame:
 *              cur |= v << nb;  nb++
 *              if nb == 8:
 *                  if len == 332: in_frame = 0
 *                  else: buf[len++] = cur;  crc = eight steps of crc = (crc >> 1) ^ (0x8408 if (crc ^ bit) & 1 else 0) over cur's
 *                        bits, the low bit first
 *                  cur = 0;  nb = 0
 *      (`nb` of step 5 is the record's bit count of the byte under way, not step 3's slicer value.)
 *
 *   6. A completed frame.  Its payload is buf[0 .. len - 3], without the FCS: 15 .. 330 bytes.  seq = frames, then frames++.  The
 *      frame goes into the ring of the handle's slot for that channel: `ring` slots a channel (a creation parameter, 1 .. 16), whose
 *      head and taken are kept on the handle's side, not in the record.  If head - taken == ring the oldest frame is dropped: taken++,
 *      lost++.  A ring slot is an asdr_packet_frame_t, 352 bytes:
 *          offset  0  uint32 channel    the channel of the ring
 *          offset  4  uint32 seq        the channel's frame number
 *          offset  8  uint32 block      low 32 bits of the handle's block count (asdr_packet_blocks) of the block in which the closing
 *                                       flag's last bit was taken: the count before the call + the block's index in it
 *          offset 12  uint16 length     payload bytes
 *          offset 14  uint16 flags      0
 *          offset 16  uint8  data[336]  the payload, the rest zero
 *
 *   Splitting a sequence of blocks into calls of any sizes leaves every frame, every slot byte and every state field unchanged.
 *
 *   Per-channel state: asdr_packet_state_t, 448 bytes, every field little-endian:
 *       offset   0  int16  hist[8]      the last 8 inputs, the newest last (6 are used)
 *       offset  16  int16  dhist[8]     the last 8 decimated values, the newest last
 *       offset  32  uint32 bits         offset  36  uint32 edges      offset  40  uint32 flags
 *       offset  44  uint32 frames       offset  48  uint32 crc_errors offset  52  uint32 aborts
 *       offset  56  uint16 clk          offset  58  uint16 len        offset  60  uint16 crc (0xFFFF at creation)
 *       offset  62  uint8  b            offset  63  uint8  prev       offset  64  uint8  sr       offset  65  uint8  cur
 *       offset  66  uint8  nb           offset  67  uint8  in_frame
 *       offset  68  uint32 reserved[11] 0
 *       offset 112  uint8  buf[336]     the bytes of the frame under way (332 are used)
 *   The setting and the ring are not in the record.  Frames decoded in slot c are delivered from slot c, whatever record is written
 *   there later.
 *
 * Delivery.  asdr_packet_collect_device writes, on `stream`, a uint32 count to dCount and that many 352-byte slots to dFrames,
 * ascending by channel and, in a channel, from the oldest frame on (ascending seq).  A frame is delivered if and only if its position in
 * that order is below max_frames; a channel's taken advances by its delivered frames only, and the rest stay for the next collect.
 * dFrames is 16-byte aligned, dCount 4-byte aligned; max_frames is 0 .. 2^24.  asdr_packet_deliver does a collect into buffers of
 * the handle, copies the count and only `count` slots to the host, and waits.  asdr_packet_ring_state reads, per channel, the frames
 * waiting (head - taken) and the frames lost to overruns; either array may be NULL.
 *
 * Calls.  asdr_packet_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_fm_update_device.  dIn must
 * be 16-byte aligned; n_blocks is 1 .. 65535 (0 does nothing); the stride is at least n_blocks.
 *
 * State.  read_state / write_state / clear / reset / ring_state wait for the handle's work first.  write_state checks every record on
 * the host before it writes one (clk < 147, len <= 332, nb < 8, b, prev and in_frame <= 1, reserved fields 0, channels in range).  clear
 * zeroes bits, edges, flags, crc_errors, aborts, lost and the count asdr_packet_blocks returns; it keeps frames and the rings.  reset
 * restores the creation state, empties the rings and keeps the setting.  Both are complete on return: a call on any stream may
 * follow.  An ASDR_NO_DEVICE handle keeps its records and settings on the host: every state call works on it, and update_device,
 * collect_device and deliver fail.
 */
#ifndef ASDR_PACKET_H_
#define ASDR_PACKET_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_PACKET_CLOCK 147           /* clk units per bit: 16 per decimated sample */
#define ASDR_PACKET_MIN_BOOST 64
#define ASDR_PACKET_MAX_BOOST 4096
#define ASDR_PACKET_MAX_RING 16
#define ASDR_PACKET_MAX_LEN 332         /* frame bytes with the FCS */
#define ASDR_PACKET_MIN_LEN 17
#define ASDR_PACKET_MAX_FRAMES (1 << 24)

static const int16_t ASDR_PACKET_C1200[9] = {256, 198, 52, -118, -235, -246, -146, 19, 176};
static const int16_t ASDR_PACKET_S1200[9] = {0, 162, 251, 227, 101, -70, -210, -255, -186};
static const int16_t ASDR_PACKET_C2200[9] = {256, 80, -206, -208, 76, 256, 83, -204, -210};
static const int16_t ASDR_PACKET_S2200[9] = {0, 243, 152, -149, -244, -4, 242, 155, -146};

typedef struct asdr_packet asdr_packet_t;

typedef struct {
  int16_t hist[8];
  int16_t dhist[8];
  uint32_t bits, edges, flags, frames, crc_errors, aborts;
  uint16_t clk, len, crc;
  uint8_t b, prev, sr, cur, nb, in_frame;
  uint32_t reserved[11];
  uint8_t buf[336];
} asdr_packet_state_t;

typedef struct {
  uint32_t channel, seq, block;
  uint16_t length, flags;
  uint8_t data[336];
} asdr_packet_frame_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576, ring in 1 .. 16 */
asdr_packet_t *asdr_packet_create(int n_channels, int ring, int device);
void asdr_packet_destroy(asdr_packet_t *t);
int asdr_packet_n_channels(const asdr_packet_t *t);

/* helpers, no device.  fcs: the AX.25 frame check sequence of n bytes (0x906E for "123456789"); a frame's FCS follows its payload,
 * the low byte first.  format_address: the address field of a payload as "SRC>DST,PATH" text ("N0CALL-7>APRS,WIDE1-1*,WIDE2-2": the
 * SSID when not 0, a '*' behind a digipeater that has repeated the frame), NUL-terminated into out; returns the text's length, -1
 * with asdr_last_error for a field that is not one (shorter than 14 bytes, no end mark within 10 addresses, a byte that is no
 * shifted printable character) or for an out_size too small */
uint16_t asdr_packet_fcs(const uint8_t *bytes, size_t n);
int asdr_packet_format_address(const uint8_t *frame, int length, char *out, int out_size);

/* per-channel setting */
int asdr_packet_set_space_boost(asdr_packet_t *t, int ch, uint32_t space_boost);
int asdr_packet_get_space_boost(const asdr_packet_t *t, int ch, uint32_t *space_boost);

/* the pass */
int asdr_packet_update_device(asdr_packet_t *t, const int16_t *dIn, long in_stride_blocks, int n_blocks, void *stream);

/* delivery */
int asdr_packet_collect_device(asdr_packet_t *t, uint32_t *dCount, asdr_packet_frame_t *dFrames, int max_frames, void *stream);
int asdr_packet_deliver(asdr_packet_t *t, uint32_t *count, asdr_packet_frame_t *host_frames, int max_frames);
int asdr_packet_ring_state(asdr_packet_t *t, uint32_t *pending /* [n_channels] or NULL */, uint32_t *lost /* [n_channels] or NULL */);

/* state */
int asdr_packet_read_state(asdr_packet_t *t, asdr_packet_state_t *dst /* [n_channels] */);
int asdr_packet_write_state(asdr_packet_t *t, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_packet_state_t *src /* [n] */);
int asdr_packet_clear(asdr_packet_t *t);
int asdr_packet_reset(asdr_packet_t *t);
long long asdr_packet_blocks(const asdr_packet_t *t); /* blocks seen since creation / clear / reset; -1 for a NULL handle */
int asdr_packet_synchronize(asdr_packet_t *t);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_PACKET_H_ */
