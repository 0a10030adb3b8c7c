/* asdr_fm.h -- C ABI of the FM demodulator: narrow-band FM audio from a tuner bank's I/Q rows, with a noise squelch.
 *
 * A stage of its own beside the AM / SAM / SSB / CW chain (libasdr_hip.so, asdr_fm.hip): it reads the 44.1 kHz int16 dI / dQ rows
 * that asdr_tuner_update_device writes and writes int16 audio rows of the shape the chain writes, so the gate, the resampler, the
 * codec and the spectrogram follow it unchanged.  A deployment that creates none runs exactly as without this header.  Same
 * conventions as asdr_gate.h: `ch` = channel index or ASDR_ALL (-1) for the setters, ASDR_NO_DEVICE for a control-plane-only
 * handle whose signal call fails, 0 / -1 return codes with asdr_last_error(); a refused setter changes nothing.
 *
 * Statement (integers only; tests/fm_ref.py is the independent numpy restatement, and the kernel is held to it bit for bit).
 * ">>" is an arithmetic shift (floor), int32 arithmetic wraps mod 2^32, clamp is to -32768 .. 32767.
 *
 *   Input:  dI, dQ int16 [n_channels][in_stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.
 *   Output: dOut   int16 [n_channels][out_stride_blocks][128].  Channel c reads row c and writes row c; a contiguous sub-range of a
 *           tuner bank is addressed by offsetting the pointers.
 *
 *   Per sample (I, Q), with (Ip, Qp) the channel's previous sample, (0, 0) at creation:
 *
 *   1. Conjugate product.  re = I Ip + Q Qp, im = Q Ip - I Qp, exact (|.| <= 2^31: four operands of -32768 give re = 2^31).
 *
 *   2. Angle theta, an int32 with 2^31 = pi, by a 20-iteration integer CORDIC in vectoring mode.  re == im == 0 gives theta = 0.
 *      Otherwise, with L the bit length of max(|re|, |im|), both are shifted by 29 - L (left; an arithmetic right shift for
 *      L > 29); if re < 0 both are negated and theta starts from 2^31, else from 0.  Then for k = 0 .. 19:
 *          if im >= 0:  (re, im, theta) <- (re + (im >> k), im - (re >> k), theta + A[k])
 *          else:        (re, im, theta) <- (re - (im >> k), im + (re >> k), theta - A[k])
 *      with A[k] = floor(atan(2^-k) / (2 pi) * 2^32 + 0.5).  theta accumulates mod 2^32 and is read as int32.  The registers
 *      stay below 2^30.22, so int32 holds them.  The error against atan2 is at most atan(2^-19) + 21 sqrt(2) 2^-28 = 2.02e-6 rad.
 *
 *   3. Gain.  v = clamp(((int64)theta * G) >> 31).  G is per channel, 1 .. 2^24.
 *      asdr_fm_gain_from_deviation(hz) = floor(32767 * 44100 / (2 hz) + 0.5): that deviation gives full scale (5 kHz: 144502).
 *
 *   4. Noise probe.  w = v - 2 v1 + v2, with v1, v2 the two previous v (0 at creation): the double difference, which weighs the
 *      discriminator's output by f^2 and so reads what lies above the voice band.  Per block N_b = sum of w^2 (exact in uint64, at
 *      most 2^41) and P_b = sum of I^2 + Q^2 (uint64): the carrier level.
 *
 *   5. DC removal.  hp_shift is per channel, 0 .. 15; 0 means off: x = v and m is untouched.  Otherwise, m an int32 in Q15:
 *          m += ((v << 15) - m) >> hp_shift;   x = clamp(v - ((m + 2^14) >> 15))
 *      m doubles as the tuning-offset meter: m / 2^15 is the mean of v, and v = 32767 at the deviation G was set for.
 *
 *   6. De-emphasis.  a is per channel, 1 .. 32768, Q15; s is an int32:
 *          s += (((x << 15) - s) * a) >> 15   (the product in 64 bits);   y = clamp((s + 2^14) >> 15)
 *      a = 32768 is an exact bypass, y = x.
 *      asdr_fm_deemphasis_from_tau_us(t) = floor(32768 * (1 - exp(-1e6 / (44100 t))) + 0.5) (750 us: 976, 75 us: 8550).
 *
 *   Per block, in block order, the noise squelch.  Per-channel settings open_noise <= close_noise (uint64, <= 2^41) and
 *   hang_blocks (0 .. 65535); creation values 2^41, 2^41, 0: that squelch is open for every block.
 *       if   N <= open_noise:             if !open: openings++;   open = 1; hang_left = hang_blocks
 *       elif open and N <= close_noise:   hang_left = hang_blocks
 *       elif open and hang_left > 0:      hang_left--
 *       elif open:                        open = 0
 *       open_blocks += open;  last_noise = N;  last_power = P
 *   It is asdr_gate.h's rule with the inequality mirrored: noise 9,0,9,9,9,9 with thresholds 0 / 5 and hang 2 gives
 *   open = 0,1,1,1,0,0; noise 1,0,1,6,6 with hang 0 gives 0,1,1,0,0.  A block whose open is 0 after the rule is written as 128
 *   zeros; m, s, v1, v2 and the previous sample advance regardless, so unmuting has no transient.  The block's own noise decides,
 *   so no look-back is needed.  An unsquelched FM channel without a carrier is full-scale noise, which an energy squelch opens on:
 *   a plain gate behind this stage with open_energy >= 1 delivers only the channels that hear a carrier.
 *   Splitting a sequence of blocks into calls of any sizes leaves every output and every state field unchanged.
 *
 *   Per-channel state: asdr_fm_state_t, 48 bytes, every field little-endian:
 *       offset  0  int16  prev_i        offset 16  uint64 last_noise     offset 40  uint16 hang_left
 *       offset  2  int16  prev_q        offset 24  uint64 last_power     offset 42  uint8  open
 *       offset  4  int16  v1            offset 32  uint32 openings       offset 43  uint8  reserved   0
 *       offset  6  int16  v2            offset 36  uint32 open_blocks    offset 44  uint32 reserved2  0
 *       offset  8  int32  s
 *       offset 12  int32  m
 *
 * Calls.  asdr_fm_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_gate_update_device: a call
 * on another stream than the previous one first waits (on the device) for the previous call's work.  dI, dQ and dOut must be
 * 16-byte aligned; n_blocks is 1 .. 65535 (0 does nothing); both strides are at least n_blocks; the output span must not overlap
 * either input span.  Settings take effect with the next call.
 *
 * State.  read_state / write_state / clear / reset wait for the handle's work first.  write_state checks every record on the host
 * before it writes one (open <= 1, reserved fields 0, channels in range).  clear zeroes openings and open_blocks (and the count
 * asdr_fm_blocks returns); reset restores the creation state and keeps the settings.  An ASDR_NO_DEVICE handle keeps its state
 * records on the host: every state call works on it, and update_device fails.
 */
#ifndef ASDR_FM_H_
#define ASDR_FM_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_FM_MAX_GAIN (1u << 24)
#define ASDR_FM_MAX_DEEMPHASIS 32768u   /* Q15 one: the bypass */
#define ASDR_FM_MAX_DC_SHIFT 15
#define ASDR_FM_MAX_HANG 65535
#define ASDR_FM_MAX_NOISE (1ULL << 41)  /* of one block: 128 * (4 * 32768)^2 */

typedef struct asdr_fm asdr_fm_t;

typedef struct {
  int16_t prev_i, prev_q;
  int16_t v1, v2;
  int32_t s;
  int32_t m;
  uint64_t last_noise;
  uint64_t last_power;
  uint32_t openings;
  uint32_t open_blocks;
  uint16_t hang_left;
  uint8_t open;
  uint8_t reserved;
  uint32_t reserved2;
} asdr_fm_state_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576.  Creation settings: the gain of 5 kHz deviation,
 * a = 32768, hp_shift = 0, the squelch always open */
asdr_fm_t *asdr_fm_create(int n_channels, int device);
void asdr_fm_destroy(asdr_fm_t *f);
int asdr_fm_n_channels(const asdr_fm_t *f);

/* settings: take effect with the next call.  A refused call changes nothing */
int asdr_fm_set_gain(asdr_fm_t *f, int ch, uint32_t gain);
int asdr_fm_get_gain(const asdr_fm_t *f, int ch, uint32_t *gain);
int asdr_fm_set_deemphasis(asdr_fm_t *f, int ch, uint32_t a);
int asdr_fm_get_deemphasis(const asdr_fm_t *f, int ch, uint32_t *a);
int asdr_fm_set_dc_shift(asdr_fm_t *f, int ch, int hp_shift);
int asdr_fm_get_dc_shift(const asdr_fm_t *f, int ch, int *hp_shift);
int asdr_fm_set_squelch(asdr_fm_t *f, int ch, uint64_t open_noise, uint64_t close_noise, int hang_blocks);
int asdr_fm_get_squelch(const asdr_fm_t *f, int ch, uint64_t *open_noise, uint64_t *close_noise, int *hang_blocks);
uint32_t asdr_fm_gain_from_deviation(double hz);    /* 0 (and asdr_last_error) where the result is outside 1 .. 2^24 */
uint32_t asdr_fm_deemphasis_from_tau_us(double t);  /* 0 (and asdr_last_error) where the result is outside 1 .. 32768 */

/* the pass */
int asdr_fm_update_device(asdr_fm_t *f, const int16_t *dI, const int16_t *dQ, long in_stride_blocks, int16_t *dOut, long out_stride_blocks,
                          int n_blocks, void *stream);

/* state */
int asdr_fm_read_state(asdr_fm_t *f, asdr_fm_state_t *dst /* [n_channels] */);
int asdr_fm_write_state(asdr_fm_t *f, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_fm_state_t *src /* [n] */);
int asdr_fm_clear(asdr_fm_t *f);
int asdr_fm_reset(asdr_fm_t *f);
long long asdr_fm_blocks(const asdr_fm_t *f); /* blocks seen since creation / clear / reset; -1 for a NULL handle */
int asdr_fm_synchronize(asdr_fm_t *f);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_FM_H_ */
