/* asdr_cw.h -- C ABI of the CW decoder: Morse text from a CW receiver's audio (the chain's CW_USBmode / CW_LSBmode behind the audioCW
 * filter, centre 774 Hz), the decoder of a CW skimmer's channels.
 *
 * A stage of its own (libasdr_hip.so, asdr_cw.hip): it reads int16 audio rows at 44.1 kHz (the chain's, or a capture sink's) and
 * writes no rows: it writes one event per decoded character.  A deployment that creates none runs exactly as without this header.
 * Same conventions as asdr_packet.h: `ch` = channel index or ASDR_ALL (-1) for the per-channel setters, ASDR_NO_DEVICE for a
 * control-plane-only handle whose signal calls fail, 0 / -1 return codes with asdr_last_error(); a refused call changes nothing.
 *
 * Statement (integers only; tests/cw_ref.py is the independent numpy restatement, and the kernel is held to it bit for bit).
 * ">>" is an arithmetic shift (floor).
 *
 *   Input:  dIn int16 [n_channels][in_stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.  Channel c reads row c.
 *
 *   Per-channel settings (from the next call):
 *     pitch_step  uint32, creation asdr_cw_pitch_step(774): the mixer's phase step per sample, floor(f 2^32 / 44100 + 0.5)
 *     min_power   uint32, creation 16: the key can be down only when P >= min_power
 *     glitch      1 .. 16, creation 4: the envelope samples a key change must last
 *     track       0 / 1, creation 1: whether D follows the marks
 *   asdr_cw_set_speed(wpm), 5 .. 60, writes the record's D = (26460 + wpm / 2) / wpm (1323 at creation: 20 WPM).  It is the one
 *   setter that writes state, not a setting: it waits for the handle's work first.
 *
 *   1. Mixer and partial sums.  C[j] = floor(1024 cos(2 pi j / 1024) + 0.5), j = 0 .. 1023 (asdr_cw_cos).  Sample n of the call,
 *      counted from 0, has phase (ph + n pitch_step) mod 2^32 and table index j = phase >> 22.  Per sub-block of 32 samples (four a
 *      block):  aI = (sum x C[j]) >> 10,  aQ = (sum x C[(j - 256) & 1023]) >> 10.  The sums fit int32 and |a| <= 2^20.  Behind the
 *      call ph += 128 n_blocks pitch_step (mod 2^32).
 *
 *   2. Envelope at 44100 / 32 = 1378.125 Hz.  I_w = this aI + the previous three (prev_i of the record, zeros at creation), Q_w
 *      likewise; P = (I_w^2 + Q_w^2) >> 14, the sum in 64 bits; P < 2^31.  The window is 128 samples; a tone of amplitude A at the
 *      pitch gives P ~ A^2 / 4.
 *
 *   3. Level trackers and raw key, per envelope sample.
 *          hi:  if P > hi: hi += (P - hi) >> 2    else: hi -= (hi - P) >> 10
 *          lo:  if P < lo: lo -= (lo - P) >> 2    else: lo += (P - lo) >> 10
 *          span = hi - lo, 0 if hi <= lo
 *          r = span > 0 and P >= min_power and P > lo + (span >> (2 if key == 0 else 3))
 *
 *   4. Glitch filter and runs.  run++ (mod 2^32).  If r != key: cnt++.  Otherwise: if cnt > 0: glitches++; then cnt = 0.
 *      If cnt == glitch:  L = run - glitch (mod 2^32);  old = key;  key = r;  run = glitch;  cnt = 0;  if old == 1 a mark of length
 *      L ends (step 5).
 *
 *   5. A mark of length L.  marks++;  dash = (16 L >= 2 D).  sym is a uint8 register, 1 = empty, 0 = overflowed:
 *          if sym >= 128 or sym == 0: sym = 0    else: sym = 2 sym + dash
 *      If track:  a dot: D += (16 L - D) >> 3;  a dash: D += (16 L / 3 - D) >> 3 (floor division of a non-negative value);  then D is
 *      clamped to 441 .. 5292 (60 .. 5 WPM).  D is the dit in sixteenths of an envelope sample; wpm = (26460 + D / 2) / D.  Products
 *      of L and of run are taken in 64 bits.
 *
 *   6. Gaps: on every envelope sample with key == 0 after step 4, with s = run.
 *          if sym != 1 and 16 s >= 2 D:    emit the character of sym (step 7);  sym = 1;  gap = 1
 *          if gap == 1 and 16 s >= 5 D:    emit ' ' (its sym field is 1: no elements; flags 0);  gap = 0
 *      A key change is known `glitch` samples after it happened and run starts from `glitch` then, so a gap is measured from its true
 *      start; but a gap that ends is still counted while the new mark's first `glitch` samples pass: a gap looks up to `glitch`
 *      samples long at its end, and a gap within that of a threshold may be taken for the longer kind.
 *
 *   7. A character.  ASDR_CW_TABLE[256] below maps sym (a leading 1, then 0 = dot and 1 = dash, the first element highest) to
 *      ASCII, 0 = no such code.  An unknown or overflowed sym emits '?' with flag bit 0 set, and unknown++.  seq = chars, then
 *      chars++.  The event goes into the channel's ring of `ring` slots (a creation parameter, 1 .. 64); head, taken and lost are
 *      on the handle's side, not in the record.  A full ring drops its oldest event: taken++, lost++.  A slot is an
 *      asdr_cw_event_t, 16 bytes:
 *          offset  0  uint32 channel    the channel of the ring
 *          offset  4  uint32 seq        the channel's character number
 *          offset  8  uint32 block      low 32 bits of the handle's block count (asdr_cw_blocks) of the block the event fell in: the
 *                                       count before the call + the block's index in it
 *          offset 12  uint8  ch         the ASCII character
 *          offset 13  uint8  wpm        the speed from D at emission
 *          offset 14  uint8  sym        the symbol register
 *          offset 15  uint8  flags      bit 0: an unknown or overflowed sym
 *
 *   Splitting a sequence of blocks into calls of any sizes leaves every event byte and every state field unchanged.
 *
 *   Per-channel state: asdr_cw_state_t, 80 bytes, every field little-endian:
 *       offset  0  uint32 ph            offset  4  int32  prev_i[3]   the last three aI, the newest last
 *       offset 16  int32  prev_q[3]     offset 28  uint32 hi          offset 32  uint32 lo        offset 36  uint32 D
 *       offset 40  uint32 run           offset 44  uint32 marks       offset 48  uint32 chars     offset 52  uint32 unknown
 *       offset 56  uint32 glitches      offset 60  uint8  cnt         offset 61  uint8  key       offset 62  uint8  sym
 *       offset 63  uint8  gap           offset 64  uint32 reserved[4] 0
 *   The settings and the ring are not in the record.  Events decoded in slot c are delivered from slot c, whatever record is written
 *   there later.
 *
 * The starting constants stand.  min_power 16, glitch 4 and the trackers' slow shift 10 were starting values, to be changed only if
 * the restatement decoded the designed messages of tests/test_cw_ref.py worse with them than with another value.  It decodes the
 * keyed messages at 12, 20 and 35 WPM, with jitter and in noise, with them; a sweep of the slow shift over 6 .. 11 found no value
 * better than 10 on any message and shifts below 9 much worse in noise.  None was changed.
 *
 * Delivery.  asdr_cw_collect_device writes, on `stream`, a uint32 count to dCount and that many 16-byte events to dEvents, ascending
 * by channel and, in a channel, from the oldest event on (ascending seq).  An event is delivered if and only if its position in that
 * order is below max_events; a channel's taken advances by its delivered events only, and the rest stay for the next collect.
 * dEvents is 16-byte aligned, dCount 4-byte aligned; max_events is 0 .. 2^26.  asdr_cw_deliver does a collect into buffers of the
 * handle, copies the count and only `count` events to the host, and waits.  asdr_cw_ring_state reads, per channel, the events waiting
 * (head - taken) and the events lost to overruns; either array may be NULL.
 *
 * Calls.  asdr_cw_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_fm_update_device.  dIn must be
 * 16-byte aligned; n_blocks is 1 .. 65535 (0 does nothing); the stride is at least n_blocks.
 *
 * State.  read_state / write_state / set_speed / clear / reset / ring_state wait for the handle's work first.  write_state checks
 * every record on the host before it writes one (D in 441 .. 5292, key and gap <= 1, cnt <= 16, prev_i and prev_q within step 1's
 * bound of +-2^20, on which P < 2^31 rests, reserved fields 0, channels in range).
 * clear zeroes marks, unknown, glitches, lost and the count asdr_cw_blocks returns; it keeps chars, the source of seq (so that the
 * events waiting in a ring stay ascending), and the rings.  reset restores the creation state, empties the rings and keeps the
 * settings.  Both are complete on return: a call on any stream may follow.  An ASDR_NO_DEVICE handle keeps its records and settings
 * on the host: every state call works on it, and update_device, collect_device and deliver fail.
 */
#ifndef ASDR_CW_H_
#define ASDR_CW_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_CW_PITCH_HZ 774            /* the centre of the chain's audioCW filter */
#define ASDR_CW_MIN_POWER 16
#define ASDR_CW_GLITCH 4
#define ASDR_CW_MAX_GLITCH 16
#define ASDR_CW_SLOW_SHIFT 10           /* the trackers' release */
#define ASDR_CW_FAST_SHIFT 2            /* the trackers' attack */
#define ASDR_CW_WPM 20
#define ASDR_CW_MIN_WPM 5
#define ASDR_CW_MAX_WPM 60
#define ASDR_CW_DIT_UNITS 26460         /* D wpm: 1.2 s x 1378.125 Hz x 16 */
#define ASDR_CW_MIN_D 441               /* 60 WPM */
#define ASDR_CW_MAX_D 5292              /* 5 WPM */
#define ASDR_CW_MAX_RING 64
#define ASDR_CW_RING 16
#define ASDR_CW_MAX_EVENTS (1 << 26)
#define ASDR_CW_FLAG_UNKNOWN 1

static const uint8_t ASDR_CW_TABLE[256] = {
    0,   0,  69,  84,  73,  65,  78,  77,  83,  85,  82,  87,  68,  75,  71,  79,
   72,  86,  70,   0,  76,   0,  80,  74,  66,  88,  67,  89,  90,  81,   0,   0,
   53,  52,   0,  51,   0,   0,   0,  50,  38,   0,  43,   0,   0,   0,   0,  49,
   54,  61,  47,   0,   0,   0,  40,   0,  55,   0,   0,   0,  56,   0,  57,  48,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,  63,  95,   0,   0,
    0,   0,  34,   0,   0,  46,   0,   0,   0,   0,  64,   0,   0,   0,  39,   0,
    0,  45,   0,   0,   0,   0,   0,   0,   0,   0,  59,  33,   0,  41,   0,   0,
    0,   0,   0,  44,   0,   0,   0,   0,  58,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,  36,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
    0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,   0,
};

typedef struct asdr_cw asdr_cw_t;

typedef struct {
  uint32_t ph;
  int32_t prev_i[3], prev_q[3];
  uint32_t hi, lo, D, run, marks, chars, unknown, glitches;
  uint8_t cnt, key, sym, gap;
  uint32_t reserved[4];
} asdr_cw_state_t;

typedef struct {
  uint32_t channel, seq, block;
  uint8_t ch, wpm, sym, flags;
} asdr_cw_event_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576, ring in 1 .. 64 */
asdr_cw_t *asdr_cw_create(int n_channels, int ring, int device);
void asdr_cw_destroy(asdr_cw_t *t);
int asdr_cw_n_channels(const asdr_cw_t *t);

/* helpers, no device.  pitch_step: floor(hz 2^32 / 44100 + 0.5) for hz in 100 .. 3000, 0 with asdr_last_error outside;  cos: C[j & 1023] */
uint32_t asdr_cw_pitch_step(double hz);
int asdr_cw_cos(int j);

/* per-channel settings */
int asdr_cw_set_pitch_step(asdr_cw_t *t, int ch, uint32_t pitch_step);
int asdr_cw_set_min_power(asdr_cw_t *t, int ch, uint32_t min_power);
int asdr_cw_set_glitch(asdr_cw_t *t, int ch, int glitch);
int asdr_cw_set_track(asdr_cw_t *t, int ch, int track);
int asdr_cw_get_settings(const asdr_cw_t *t, int ch, uint32_t *pitch_step, uint32_t *min_power, int *glitch, int *track);
int asdr_cw_set_speed(asdr_cw_t *t, int ch, int wpm);

/* the pass */
int asdr_cw_update_device(asdr_cw_t *t, const int16_t *dIn, long in_stride_blocks, int n_blocks, void *stream);

/* delivery */
int asdr_cw_collect_device(asdr_cw_t *t, uint32_t *dCount, asdr_cw_event_t *dEvents, int max_events, void *stream);
int asdr_cw_deliver(asdr_cw_t *t, uint32_t *count, asdr_cw_event_t *host_events, int max_events);
int asdr_cw_ring_state(asdr_cw_t *t, uint32_t *pending /* [n_channels] or NULL */, uint32_t *lost /* [n_channels] or NULL */);

/* state */
int asdr_cw_read_state(asdr_cw_t *t, asdr_cw_state_t *dst /* [n_channels] */);
int asdr_cw_write_state(asdr_cw_t *t, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_cw_state_t *src /* [n] */);
int asdr_cw_clear(asdr_cw_t *t);
int asdr_cw_reset(asdr_cw_t *t);
long long asdr_cw_blocks(const asdr_cw_t *t); /* blocks seen since creation / clear / reset; -1 for a NULL handle */
int asdr_cw_synchronize(asdr_cw_t *t);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_CW_H_ */
