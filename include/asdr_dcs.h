/* asdr_dcs.h -- C ABI of the DCS squelch: digital coded squelch (134.4 bit/s, 23-bit Golay words) behind the FM demodulator.
 *
 * A stage of its own (libasdr_hip.so, asdr_dcs.hip): it reads the int16 audio rows that asdr_fm_update_device writes (with FM's
 * hp_shift 12 or more, or 0, the code is in them) and writes int16 audio rows of the same shape, so the gate, the tone squelch, the
 * resampler, the codec and the spectrogram follow it unchanged.  Code search: it names the code a channel carries.  Code squelch: it
 * mutes, in the rows it writes, the channels whose code is not the wanted one.  A deployment that creates none runs exactly as
 * without this header.  Same conventions as asdr_tone.h: `ch` = channel index or ASDR_ALL (-1) for the per-channel setters,
 * ASDR_NO_DEVICE for a control-plane-only handle whose signal call fails, 0 / -1 return codes with asdr_last_error(); a refused call
 * changes nothing.
 *
 * Words.  A code is three octal digits c (9 bits).  Its 12 data bits are d = 0x800 | c (the fixed bits are 100), its 11 parity bits
 * p = (d x^11) mod g over GF(2) with g = 0xC75, the word is w = p << 12 | d, sent bit 0 first and repeated without a gap.  Code 023
 * gives 0x763813.  The 104 codes of ASDR_DCS_CODES fall into 104 different rotation classes; the complement of every rotation of
 * every one of them is a rotation of another of them (the complement of 023 is a rotation of 047: "023 inverted" and "047 normal"
 * are one signal), so the stage has no "invert" setting: polarity is a matter of which table entry is wanted, and asdr_dcs_find
 * does the lookup.  Any two different words among their 2,392 rotations differ in at least 7 bits.
 *
 * Statement (integers only; tests/dcs_ref.py is the independent numpy restatement, and the kernel is held to it bit for bit).
 * ">>" is an arithmetic shift (floor), clamp is to -32768 .. 32767.
 *
 *   Input:  dIn  int16 [n_channels][in_stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.
 *   Output: dOut int16 [n_channels][out_stride_blocks][128].  Channel c reads row c and writes row c.
 *
 *   Bank-wide settings (from the next call):
 *     code table   n_codes in 1 .. 128 words T[i] of 23 bits, set as octal codes.  Refused unless every pair of table words differs
 *                  in at least 2 max_errors + 1 bits.  Creation: the 104 codes of ASDR_DCS_CODES.  Setting it restores sr, cand, age,
 *                  run, detected and quiet of every channel to their creation values; open and the counters stay.
 *     max_errors   0 .. 3, creation 0.  Refused if the table's distance does not allow it.
 *     confirm      1 .. 8, creation 2: the words in a row, 23 bits apart, that make a detection.
 *     hold_bits    23 .. 1023, creation 46: the bits without a confirmed word after which a detection lapses.
 *   Per-channel settings:
 *     want         ASDR_DCS_PASS (-2, creation): never muted, search only.  ASDR_DCS_ANY (-1): any detected code opens.
 *                  0 .. n_codes - 1: only that table entry opens.
 *     hysteresis   uint32, creation 0, on the scale of s below: a code of amplitude A gives |s| of about 20 A.
 *
 *   Per block of 128 input samples x, in block order:
 *
 *   1. Decimate by 16, exactly as step 1 of asdr_tone.h.  d_k = (sum_{j = 0 .. 45} h[j] x[16 k + 15 - j] + 2048) >> 12 for
 *      k = 0 .. 7, h the 46 coefficients of (1 + z + ... + z^15)^3.  Negative sample indices reach into the channel's previous
 *      samples (hist, zeros at creation).  |d| <= 32767.
 *
 *   2. Bit filter.  s = sum_{j = 0 .. 19} d[n - j] in int32, |s| <= 20 * 32768; it reaches into dhist, the channel's last decimated
 *      values (zeros at creation).  A bit is 2625 / 128 = 20.51 decimated samples: 44100 / 134.4 = 2625 / 8 exactly.
 *
 *   3. Slicer and clock.  clk counts a bit's time in 0 .. 2624, 128 per decimated sample.  For each of the 8 values in order:
 *          nb = 1 if s > hysteresis, 0 if s < -hysteresis, else b
 *          if nb != b:   e = clk if clk < 1312 else clk - 2625;   clk = (clk - (e >> 2)) mod 2625, taken into 0 .. 2624;
 *                        b = nb;  edges++
 *          p = clk;  clk += 128;  if p < 1312 <= clk: a bit is taken (step 4, with b);  if clk >= 2625: clk -= 2625
 *      At most one bit is taken per block: over every clk and every pattern of edges in a block (tests/test_dcs_ref.py goes through
 *      them), because an edge at clk >= 1312, behind a bit's middle, only ever moves the clock forward.
 *
 *   4. On a bit.
 *          sr = (sr >> 1) | (b << 22);  bits++;  age = min(age + 1, 255);  quiet = min(quiet + 1, 65535)
 *          dist_i = popcount(sr ^ T[i]);  best = the lowest index of the minimum
 *          if dist_best <= max_errors:
 *              hits++;  run = min(run + 1, 255) if best == cand and age == 23, else 1;  cand = best;  age = 0
 *              if run >= confirm:   if detected != best: detections++;   detected = best;  quiet = 0
 *          if detected >= 0 and quiet > hold_bits:  detected = -1
 *          match = 1 for PASS, (detected >= 0) for ANY, (detected == want) otherwise
 *          if match and !open: openings++;   open = match
 *
 *   5. Output.  The block leaves as x, or as 128 zeros if want != PASS and open == 0.  open is read before the block's step 3, so a
 *      verdict acts from the next block on.  Every state advances regardless.  open_blocks counts the blocks that left unmuted.
 *
 *   Splitting a sequence of blocks into calls of any sizes leaves every output and every state field unchanged.  A row of zeros (FM's
 *   closed noise squelch writes such rows) moves nothing but the clock: s = 0, b holds, bits are taken from the held b, and a
 *   constant register matches no table word.
 *
 *   Per-channel state: asdr_dcs_state_t, 192 bytes, every field little-endian:
 *       offset   0  int16  hist[48]     the last 48 inputs, the newest last (45 are used)
 *       offset  96  int16  dhist[24]    the last 24 decimated values, the newest last (19 are used)
 *       offset 144  uint32 sr           offset 148  uint32 bits         offset 152  uint32 hits       offset 156  uint32 detections
 *       offset 160  uint32 openings     offset 164  uint32 open_blocks  offset 168  uint32 edges
 *       offset 172  int16  detected     offset 174  int16  cand         (both -1 at creation)
 *       offset 176  uint16 clk          offset 178  uint16 quiet
 *       offset 180  uint8  age (255 at creation)   offset 181  uint8  run   offset 182  uint8  b   offset 183  uint8  open
 *       offset 184  uint32 reserved[2]  0
 *   The settings are not in the record.
 *
 * Calls.  asdr_dcs_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_fm_update_device.  dIn and
 * dOut must be 16-byte aligned; n_blocks is 1 .. 65535 (0 does nothing); both strides are at least n_blocks; the output span must
 * not overlap the input span.
 *
 * State.  read_state / write_state / clear / reset wait for the handle's work first.  write_state checks every record on the host
 * before it writes one (clk < 2625, sr < 2^23, b and open <= 1, detected and cand in -1 .. n_codes - 1, reserved fields 0, channels
 * in range).  clear zeroes bits, hits, detections, openings, open_blocks and edges (and the count asdr_dcs_blocks returns); reset
 * restores the creation state and keeps the settings.  An ASDR_NO_DEVICE handle keeps its state records on the host: every state
 * call works on it, and update_device fails.
 */
#ifndef ASDR_DCS_H_
#define ASDR_DCS_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_DCS_PASS (-2)
#define ASDR_DCS_ANY (-1)
#define ASDR_DCS_MAX_CODES 128
#define ASDR_DCS_MAX_CODE 0777
#define ASDR_DCS_MAX_ERRORS 3
#define ASDR_DCS_MAX_CONFIRM 8
#define ASDR_DCS_MIN_HOLD 23
#define ASDR_DCS_MAX_HOLD 1023
#define ASDR_DCS_CLOCK 2625           /* clk units per bit: 128 per decimated sample */
#define ASDR_DCS_COUNT 104

/* the 104 standard DCS codes: the creation table */
static const uint16_t ASDR_DCS_CODES[ASDR_DCS_COUNT] = {
    0023, 0025, 0026, 0031, 0032, 0036, 0043, 0047, 0051, 0053, 0054, 0065, 0071, 0072, 0073, 0074, 0114, 0115, 0116, 0122, 0125,
    0131, 0132, 0134, 0143, 0145, 0152, 0155, 0156, 0162, 0165, 0172, 0174, 0205, 0212, 0223, 0225, 0226, 0243, 0244, 0245, 0246,
    0251, 0252, 0255, 0261, 0263, 0265, 0266, 0271, 0274, 0306, 0311, 0315, 0325, 0331, 0332, 0343, 0346, 0351, 0356, 0364, 0365,
    0371, 0411, 0412, 0413, 0423, 0431, 0432, 0445, 0446, 0452, 0454, 0455, 0462, 0464, 0465, 0466, 0503, 0506, 0516, 0523, 0526,
    0532, 0546, 0565, 0606, 0612, 0624, 0627, 0631, 0632, 0654, 0662, 0664, 0703, 0712, 0723, 0731, 0732, 0734, 0743, 0754};

typedef struct asdr_dcs asdr_dcs_t;

typedef struct {
  int16_t hist[48];
  int16_t dhist[24];
  uint32_t sr, bits, hits, detections, openings, open_blocks, edges;
  int16_t detected, cand;
  uint16_t clk, quiet;
  uint8_t age, run, b, open;
  uint32_t reserved[2];
} asdr_dcs_state_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576 */
asdr_dcs_t *asdr_dcs_create(int n_channels, int device);
void asdr_dcs_destroy(asdr_dcs_t *t);
int asdr_dcs_n_channels(const asdr_dcs_t *t);

/* helpers.  word: 0 and asdr_last_error for a code above 0777.  find: the lowest table index whose word is a rotation of the code's
 * word (of its complement when `inverted` is not 0), -1 if none is (and for a refused code or handle, with asdr_last_error) */
uint32_t asdr_dcs_word(int code);
int asdr_dcs_find(const asdr_dcs_t *t, int code, int inverted);

/* bank-wide settings.  get_codes fills codes and words (either may be NULL), at most ASDR_DCS_MAX_CODES entries, and returns n_codes */
int asdr_dcs_set_codes(asdr_dcs_t *t, const int *codes, int n_codes);
int asdr_dcs_get_codes(const asdr_dcs_t *t, int *codes, uint32_t *words);
int asdr_dcs_set_max_errors(asdr_dcs_t *t, int max_errors);
int asdr_dcs_get_max_errors(const asdr_dcs_t *t);
int asdr_dcs_set_confirm(asdr_dcs_t *t, int confirm);
int asdr_dcs_get_confirm(const asdr_dcs_t *t);
int asdr_dcs_set_hold_bits(asdr_dcs_t *t, int hold_bits);
int asdr_dcs_get_hold_bits(const asdr_dcs_t *t);

/* per-channel settings */
int asdr_dcs_set_want(asdr_dcs_t *t, int ch, int want);
int asdr_dcs_get_want(const asdr_dcs_t *t, int ch, int *want);
int asdr_dcs_set_hysteresis(asdr_dcs_t *t, int ch, uint32_t hysteresis);
int asdr_dcs_get_hysteresis(const asdr_dcs_t *t, int ch, uint32_t *hysteresis);

/* the pass */
int asdr_dcs_update_device(asdr_dcs_t *t, const int16_t *dIn, long in_stride_blocks, int16_t *dOut, long out_stride_blocks, int n_blocks,
                           void *stream);

/* state */
int asdr_dcs_read_state(asdr_dcs_t *t, asdr_dcs_state_t *dst /* [n_channels] */);
int asdr_dcs_write_state(asdr_dcs_t *t, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_dcs_state_t *src /* [n] */);
int asdr_dcs_clear(asdr_dcs_t *t);
int asdr_dcs_reset(asdr_dcs_t *t);
long long asdr_dcs_blocks(const asdr_dcs_t *t); /* blocks seen since creation / clear / reset; -1 for a NULL handle */
int asdr_dcs_synchronize(asdr_dcs_t *t);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_DCS_H_ */
