/* asdr_tone.h -- C ABI of the tone squelch: CTCSS decode, tone squelch and a sub-audible high-pass behind the FM demodulator.
 *
 * A stage of its own (libasdr_hip.so, asdr_tone.hip): it reads the int16 audio rows that asdr_fm_update_device writes (with FM's
 * hp_shift 12 or more, or 0, the sub-audible tone is in them) and writes int16 audio rows of the same shape, so the gate, the
 * resampler, the codec and the spectrogram follow it unchanged.  A deployment that creates none runs exactly as without this header.
 * Same conventions as asdr_fm.h: `ch` = channel index or ASDR_ALL (-1) for the per-channel setters, ASDR_NO_DEVICE for a
 * control-plane-only handle whose signal call fails, 0 / -1 return codes with asdr_last_error(); a refused call changes nothing.
 *
 * Statement (integers only; tests/tone_ref.py is the independent numpy restatement, and the kernel is held to it bit for bit).
 * ">>" is an arithmetic shift (floor), int32 and int64 arithmetic wraps, clamp is to -32768 .. 32767.
 *
 *   Input:  dIn  int16 [n_channels][in_stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.
 *   Output: dOut int16 [n_channels][out_stride_blocks][128].  Channel c reads row c and writes row c.
 *
 *   Bank-wide settings (from the next call):
 *     tone table   n_tones in 1 .. 64 frequencies in Hz, strictly ascending, each below 1,378 Hz, held as uint32 phase steps
 *                  floor(f * 16 * 2^32 / 44100 + 0.5) that must ascend strictly too.  Creation: the 50 CTCSS tones, ASDR_CTCSS_TONES.
 *     window       W blocks, 16 .. 128; creation 64 (186 ms).
 *                  Setting the table or W zeroes every channel's accumulators and window_block; open, detected and the counters stay.
 *     dominance    Q4, 16 .. 1024; creation 64: the best tone carries 4 x the power of the strongest tone that is not its neighbour.
 *     high-pass    0 .. 3 biquad sections (b0, b1, b2, a1, a2), int32 in Q28; creation 0 sections, an exact pass.
 *                  asdr_tone_highpass_design(fc, sections, out): the bilinear Butterworth high-pass of order 2 sections at 44.1 kHz.
 *                  With K = tan(pi fc / 44100) and, for section k, q = 2 sin(pi (2 k + 1) / (4 sections)):  n = 1 / (1 + q K + K^2),
 *                  b = (n, -2 n, n), a1 = 2 (K^2 - 1) n, a2 = (1 - q K + K^2) n, each rounded as floor(c 2^28 + 0.5).
 *   Per-channel settings:
 *     want         ASDR_TONE_PASS (-2, creation): never muted, decode only.  ASDR_TONE_ANY (-1): any detected tone opens.
 *                  0 .. n_tones - 1: only that tone opens.
 *     min_power    uint64, creation 0.  asdr_tone_min_power(amplitude, W) = floor((128 amplitude W)^2 / 4).
 *     hang_windows 0 .. 255, creation 0.
 *
 *   Per block of 128 input samples x, in block order:
 *
 *   1. Decimate by 16.  d_k = (sum_{j = 0 .. 45} h[j] x[16 k + 15 - j] + 2048) >> 12 for k = 0 .. 7, h the 46 coefficients of
 *      (1 + z + ... + z^15)^3 (their sum is 4096).  Negative sample indices reach into the channel's previous samples (hist, zeros at
 *      creation).  |d| <= 32767.  A third-order CIC: nulls on the multiples of 2,756.25 Hz, 0.36 dB of droop at 254.1 Hz.
 *
 *   2. Correlate.  p = 8 window_block + k is the sample's place in the window; C[j] = floor(16384 cos(2 pi j / 1024) + 0.5).  For tone
 *      t: phi = (step_t p) mod 2^32, i = phi >> 22; the block's exact sums R = sum_k d_k C[i] and S = sum_k d_k C[(i - 256) & 1023]
 *      (each at most 2^32 in magnitude); re_t += R >> 9, im_t += S >> 9, both int32.  They stay within W 2^23 <= 2^30.
 *
 *   3. High-pass, on x at the full rate.  u = x << 8; per section, direct form I on int32 states (x1, x2, y1, y2):
 *          acc = b0 u + b1 x1 + b2 x2 - a1 y1 - a2 y2   (int64);   o = clamp30((acc + 2^27) >> 28), clamp30 to -2^30 .. 2^30 - 1;
 *          (x2, x1, y2, y1) <- (x1, u, y1, o);   u = o
 *      y = clamp((u + 128) >> 8).  With 0 sections y = x.
 *
 *   4. Output.  The block leaves as y, or as 128 zeros if want != PASS and open == 0.  open is read before step 5, so a window's
 *      verdict acts from the next block on.  hist, the filter states and the accumulators advance regardless, so unmuting has no
 *      transient.  open_blocks counts the blocks that left unmuted.
 *
 *   5. Window end.  window_block += 1; when it reaches W:
 *          P_t = re_t^2 + im_t^2 (uint64);  best = the lowest index of the maximum;  other = max P_t over |t - best| >= 2, else 0
 *          detected = best if P_best >= min_power and 16 (P_best >> 8) >= dominance (other >> 8), else -1
 *          match = 1 for PASS, (detected >= 0) for ANY, (detected == want) otherwise
 *          if match:                     if !open: openings++;   open = 1; hang_left = hang_windows
 *          elif open and hang_left > 0:  hang_left--
 *          elif open:                    open = 0
 *          windows++; matches += match; last_best = best; last_power = P_best; last_other = other
 *          the accumulators are zeroed and window_block = 0
 *   Splitting a sequence of blocks into calls of any sizes leaves every output and every state field unchanged.
 *
 *   Per-channel state: asdr_tone_state_t, 704 bytes, every field little-endian:
 *       offset   0  int16  hist[48]       the last 48 inputs, the newest last (45 are used)
 *       offset  96  int32  hp[3][4]       per section x1, x2, y1, y2
 *       offset 144  uint64 last_power     offset 152  uint64 last_other
 *       offset 160  uint32 windows        offset 164  uint32 matches      offset 168  uint32 openings    offset 172  uint32 open_blocks
 *       offset 176  int16  detected       offset 178  int16  last_best    (both -1 at creation)
 *       offset 180  uint16 window_block   offset 182  uint8  hang_left    offset 183  uint8  open
 *       offset 184  uint32 reserved[2]    0
 *       offset 192  int32  acc[64][2]     re, im of tone t
 *   The settings are not in the record.
 *
 * Calls.  asdr_tone_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_fm_update_device.  dIn and
 * dOut must be 16-byte aligned; n_blocks is 1 .. 65535 (0 does nothing); both strides are at least n_blocks; the output span must
 * not overlap the input span.
 *
 * State.  read_state / write_state / clear / reset wait for the handle's work first.  write_state checks every record on the host
 * before it writes one (open <= 1, window_block < W, detected and last_best in -1 .. n_tones - 1, reserved fields 0, acc zero from
 * n_tones on, channels in range).  Channels whose window_block differ work in one call.  clear zeroes windows, matches, openings and
 * open_blocks (and the count asdr_tone_blocks returns); reset restores the creation state and keeps the settings.  An
 * ASDR_NO_DEVICE handle keeps its state records on the host: every state call works on it, and update_device fails.
 */
#ifndef ASDR_TONE_H_
#define ASDR_TONE_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_TONE_PASS (-2)
#define ASDR_TONE_ANY (-1)
#define ASDR_TONE_MAX_TONES 64
#define ASDR_TONE_MAX_HZ 1378.0        /* tones lie below it: half the decimated rate, 44100 / 32 */
#define ASDR_TONE_MIN_WINDOW 16
#define ASDR_TONE_MAX_WINDOW 128
#define ASDR_TONE_MIN_DOMINANCE 16
#define ASDR_TONE_MAX_DOMINANCE 1024
#define ASDR_TONE_MAX_SECTIONS 3
#define ASDR_TONE_MAX_HANG 255
#define ASDR_CTCSS_COUNT 50

/* the 50 standard CTCSS tones in Hz: the creation table */
static const double ASDR_CTCSS_TONES[ASDR_CTCSS_COUNT] = {
    67.0,  69.3,  71.9,  74.4,  77.0,  79.7,  82.5,  85.4,  88.5,  91.5,  94.8,  97.4,  100.0, 103.5, 107.2, 110.9, 114.8,
    118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
    183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1};

typedef struct asdr_tone asdr_tone_t;

typedef struct {
  int16_t hist[48];
  int32_t hp[3][4];
  uint64_t last_power, last_other;
  uint32_t windows, matches, openings, open_blocks;
  int16_t detected, last_best;
  uint16_t window_block;
  uint8_t hang_left, open;
  uint32_t reserved[2];
  int32_t acc[64][2];
} asdr_tone_state_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576 */
asdr_tone_t *asdr_tone_create(int n_channels, int device);
void asdr_tone_destroy(asdr_tone_t *t);
int asdr_tone_n_channels(const asdr_tone_t *t);

/* bank-wide settings.  get_tones fills hz and steps (either may be NULL), at most ASDR_TONE_MAX_TONES entries, and returns n_tones */
int asdr_tone_set_tones(asdr_tone_t *t, const double *hz, int n_tones);
int asdr_tone_get_tones(const asdr_tone_t *t, double *hz, uint32_t *steps);
int asdr_tone_set_window(asdr_tone_t *t, int window_blocks);
int asdr_tone_get_window(const asdr_tone_t *t);
int asdr_tone_set_dominance(asdr_tone_t *t, int dominance_q4);
int asdr_tone_get_dominance(const asdr_tone_t *t);
int asdr_tone_set_highpass(asdr_tone_t *t, const int32_t *coefficients /* [sections][5] */, int sections);
int asdr_tone_get_highpass(const asdr_tone_t *t, int32_t *coefficients /* [3][5], may be NULL */); /* returns the sections */
int asdr_tone_highpass_design(double fc_hz, int sections, int32_t *out /* [sections][5] */);
uint64_t asdr_tone_min_power(double amplitude, int window_blocks); /* floor((128 amplitude W)^2 / 4); 0 and asdr_last_error if refused */

/* per-channel settings */
int asdr_tone_set_want(asdr_tone_t *t, int ch, int want);
int asdr_tone_get_want(const asdr_tone_t *t, int ch, int *want);
int asdr_tone_set_min_power(asdr_tone_t *t, int ch, uint64_t min_power);
int asdr_tone_get_min_power(const asdr_tone_t *t, int ch, uint64_t *min_power);
int asdr_tone_set_hang(asdr_tone_t *t, int ch, int hang_windows);
int asdr_tone_get_hang(const asdr_tone_t *t, int ch, int *hang_windows);

/* the pass */
int asdr_tone_update_device(asdr_tone_t *t, const int16_t *dIn, long in_stride_blocks, int16_t *dOut, long out_stride_blocks, int n_blocks,
                            void *stream);

/* state */
int asdr_tone_read_state(asdr_tone_t *t, asdr_tone_state_t *dst /* [n_channels] */);
int asdr_tone_write_state(asdr_tone_t *t, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_tone_state_t *src /* [n] */);
int asdr_tone_clear(asdr_tone_t *t);
int asdr_tone_reset(asdr_tone_t *t);
long long asdr_tone_blocks(const asdr_tone_t *t); /* blocks seen since creation / clear / reset; -1 for a NULL handle */
int asdr_tone_synchronize(asdr_tone_t *t);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_TONE_H_ */
