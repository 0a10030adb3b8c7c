/* asdr_resample.h -- C ABI of the audio resampler: the receivers' 44.1 kHz audio rows at a decoder's rate (8, 12, 16 kHz ...).
 *
 * An after-pass over the int16 audio rows that asdr_update_device_strided wrote, or over the capture sink's rows
 * (asdr_capture_device_ptr with stride_blocks = capacity).  It writes int16 rows at Fs_out = 44100 U / M on the device, for every
 * channel or for the channels a gate (asdr_gate.h) delivered, so that a service behind a large bank moves 12 kHz rows of the
 * receivers that hear something over PCIe instead of 44.1 kHz rows of all of them.  A resampler is an object of its own
 * (libasdr_hip.so, asdr_resample.hip); it changes no chain, tuner or gate kernel, and a deployment that creates none runs exactly
 * as without this header.  Same conventions as asdr_gate.h: ASDR_NO_DEVICE for a control-plane-only resampler whose signal calls
 * fail, 0 / -1 return codes with asdr_last_error(), and a refused call changes nothing.
 *
 * Statement (integers only; tests/resample_ref.py is the independent numpy restatement, and the kernels are held to it bit for bit).
 *
 *   Rate.    g = gcd(Fs_out, 44100), U = Fs_out / g, M = 44100 / g.  Accepted: 1 <= U <= 512 and U <= M <= 16 U.  Interpolation
 *            (U > M) is refused.  U = M = 1 with the filter {16384}, shift 14, is the identity (a tap of 32768 does not fit
 *            int16): (16384 x + 8192) >> 14 = x.
 *
 *   Filter.  K taps per phase, 1 <= K <= 256, int16, given as h[k U + phi] (k = 0 .. K - 1, phi = 0 .. U - 1), with a shift s in
 *            0 .. 15 and round = s ? 1 << (s - 1) : 0.  A filter is refused unless  sum over k of |h[k U + phi]| <= 65535  for every
 *            phase phi: then every partial sum below is exact in int32, in whatever order it is formed.
 *
 *   Output.  Output j >= 0 of every channel, with x[i < 0] = 0:
 *
 *                y[j] = sat16((sum over k = 0 .. K - 1 of h[k U + phi_j] x[b_j - k]  +  round) >> s),
 *                b_j = floor(j M / U),   phi_j = j M mod U
 *
 *            (>> is the arithmetic shift, sat16 clamps to -32768 .. 32767).
 *
 *   Timing.  The bank is in lockstep: N = input samples consumed so far (int64, one number for all channels).  Output j is written
 *            by the first call after which b_j <= N - 1: a call that takes N from N0 to N1 = N0 + 128 n_blocks writes outputs
 *            ceil(N0 U / M) .. ceil(N1 U / M) - 1 of every channel, as samples 0 .. of its rows of dOut, and returns their number,
 *            which the host knows without asking the device.  Splitting a block sequence into calls of any sizes leaves every
 *            output unchanged.  At 12 kHz a block gives 34 or 35 outputs, at 8 kHz 23 or 24, at 11.025 kHz 32.
 *
 *   State.   The per-channel state record is the channel's last 256 input samples, oldest first: int16[256], 512 bytes
 *            (ASDR_RESAMPLE_STATE_SAMPLES).  Samples before position 0 are zero.  The first output of a call has b_j >= N0, so it
 *            reaches at most K - 1 <= 255 samples behind the call.  The record depends neither on N nor on the rate: it moves
 *            between resamplers freely.
 *
 *   Defaults (asdr_resampler_create).  The prototype is a Kaiser-windowed sinc at U 44100 Hz with passband 0 .. 0.42 Fs_out and
 *            stop band from 0.58 Fs_out, so nothing folds into the passband:
 *                dw = 2 pi 0.16 Fs_out / (U 44100),   K = 2 ceil((80 - 7.95) / (2.285 dw) / (2 U)),   L = U K,
 *                h[i] = 2 fc sinc(2 fc (i - (L - 1) / 2)) kaiser(L, beta = 0.1102 (80 - 8.7)),   fc = 0.5 Fs_out / (U 44100)
 *            Each phase is scaled to sum 32768 and rounded to nearest; its tap of largest magnitude takes the residual, so the DC
 *            gain is exactly 1 in every phase (no spur at the resampling rate: the rate banks' rule, asdr_tuner.h).  s = 15.
 *            Fs_out = 44100 gives the identity.  The rounded taps:
 *                Fs_out   U / M     K    max sum |h|   stop band
 *                  8000   80 / 441  174    62268        74.7 dB
 *                 11025    1 / 4    126    62824        68.8 dB
 *                 12000   40 / 147  116    62420        75.2 dB
 *                 16000  160 / 441   88    62776        78.0 dB
 *                 22050    1 / 2     64    65500        72.3 dB
 *                 24000   80 / 147   58    62896        78.4 dB
 *                 32000  320 / 441   44    64454        79.8 dB
 *            The filter is causal; its delay of (L - 1) / (2 U) input samples is what asdr_resampler_delay returns (for a custom
 *            filter the same expression: the delay of a symmetric prototype).
 *
 * The pass.  asdr_resampler_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_gate_update_device:
 * a call on another stream than the previous one first waits (on the device) for the previous call's work.  dAudio: int16 rows
 * [n_channels][stride_blocks][128] of which blocks 0 .. n_blocks - 1 are new; n_blocks in 1 .. 65535 (0 does nothing and returns 0),
 * stride_blocks >= n_blocks, 16-byte aligned.  dOut: int16 rows [..][out_stride_samples], out_stride_samples at least the returned
 * count, 2-byte aligned, not overlapping the audio span.  It returns the per-row output count (asdr_resampler_out_samples(n_blocks)
 * says it beforehand), or -1.
 *     dIndex == NULL:  row c of dOut is channel c, for all n_channels (capacity_rows is ignored).
 *     otherwise:       dIndex / dCount are device addresses (int32 [..] and one int32), typically asdr_gate_index_device /
 *                      asdr_gate_count_device of a gate run earlier on the same stream over the same rows.  Row i of dOut is channel
 *                      dIndex[i] for i < min(*dCount, capacity_rows); rows past that are not written.  There is no host round trip.
 * Every channel's carry advances in every call, delivered or not, so a channel that opens later has the right history.  Samples of
 * a row past the returned count are not written.  There is no host-pointer entry: the consumer copies dOut.
 *
 * State.  read_state / write_state / reset / set_filter / set_position wait for the resampler's work first.  write_state is all or
 * nothing: every channel is range-checked before one record is written.  reset gives zero records and N = 0 and keeps the filter.
 * set_filter swaps the filter (same U and M) and keeps the records and N.  set_position(N) places a restored resampler: with
 * write_state it is the checkpoint / resume path (N in 0 .. 2^50).  An ASDR_NO_DEVICE resampler keeps its records on the host:
 * every call but update_device works on it.
 */
#ifndef ASDR_RESAMPLE_H_
#define ASDR_RESAMPLE_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_RESAMPLE_FS_IN 44100
#define ASDR_RESAMPLE_MAX_UP 512
#define ASDR_RESAMPLE_MAX_RATIO 16         /* M <= 16 U */
#define ASDR_RESAMPLE_MAX_TAPS 256         /* per phase */
#define ASDR_RESAMPLE_MAX_ABS_SUM 65535    /* of a phase's taps */
#define ASDR_RESAMPLE_STATE_SAMPLES 256
#define ASDR_RESAMPLE_MAX_POSITION (1LL << 50)

typedef struct asdr_resampler asdr_resampler_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576 */
asdr_resampler_t *asdr_resampler_create(int n_channels, int fs_out, int device);
asdr_resampler_t *asdr_resampler_create_custom(int n_channels, int up, int down, int taps_per_phase, const int16_t *taps /* [up * taps_per_phase] */,
                                               int shift, int device);
void asdr_resampler_destroy(asdr_resampler_t *r);
int asdr_resampler_n_channels(const asdr_resampler_t *r);

/* the rate and the filter */
int asdr_resampler_up(const asdr_resampler_t *r);
int asdr_resampler_down(const asdr_resampler_t *r);
int asdr_resampler_taps_per_phase(const asdr_resampler_t *r);
int asdr_resampler_get_taps(const asdr_resampler_t *r, int16_t *taps /* [up * taps_per_phase] */, int *shift);
double asdr_resampler_delay(const asdr_resampler_t *r); /* input samples; NaN for a NULL resampler */
int asdr_resampler_set_filter(asdr_resampler_t *r, int taps_per_phase, const int16_t *taps, int shift);

/* position */
long long asdr_resampler_position(const asdr_resampler_t *r);         /* N; -1 for a NULL resampler */
long long asdr_resampler_output_position(const asdr_resampler_t *r);  /* ceil(N U / M) */
long asdr_resampler_out_samples(const asdr_resampler_t *r, int n_blocks); /* what the next call of that size returns */
int asdr_resampler_set_position(asdr_resampler_t *r, long long n);

/* the pass */
long asdr_resampler_update_device(asdr_resampler_t *r, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dOut,
                                  long out_stride_samples, const int32_t *dIndex /* NULL: all channels */, const int32_t *dCount,
                                  int capacity_rows, void *stream);

/* state */
int asdr_resampler_read_state(asdr_resampler_t *r, int16_t *dst /* [n_channels][256] */);
int asdr_resampler_write_state(asdr_resampler_t *r, const int *channels /* NULL: 0 .. n - 1 */, int n, const int16_t *src /* [n][256] */);
int asdr_resampler_reset(asdr_resampler_t *r);
int asdr_resampler_synchronize(asdr_resampler_t *r);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_RESAMPLE_H_ */
