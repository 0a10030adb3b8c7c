/* asdr_spectrogram.h -- C ABI of the audio spectrogram: per-receiver STFT rows (a band of bins per frame) of int16 audio rows.
 *
 * An after-pass over int16 audio rows on the device: the chain's rows (asdr_update_device_strided), a capture sink's
 * (asdr_capture_device_ptr) or a resampler's dOut (asdr_resample.h) at a decoder's rate.  Every weak-signal decoder (WSPR, FT8 / FT4,
 * JS8), a CW skimmer and a per-receiver audio waterfall begin with it.  A spectrogram is an object of its own (libasdr_hip.so,
 * asdr_spectrogram.hip); it changes no chain, tuner, gate, resampler or codec kernel, and a deployment that creates none runs exactly
 * as without this header.  Same conventions as asdr_resample.h: ASDR_NO_DEVICE for a control-plane-only spectrogram whose signal call
 * fails, 0 / -1 return codes with asdr_last_error(), and a refused call changes nothing.
 *
 * Statement (float64; tests/spectrogram_ref.py is the independent numpy restatement, and the kernels, which work in float32, are
 * held to it within the tolerance of DESIGN.md 3.13).
 *
 *   Parameters (at creation).  N in {128, 256, 512, 1024, 2048, 4096, 8192}.  Hop H, any integer with N / 16 <= H <= N.  Band k0, B
 *            with 0 <= k0, 1 <= B, k0 + B <= N / 2 + 1.  Window w: rect (w[n] = 1), hann (w[n] = 0.5 - 0.5 cos(2 pi n / N), formed
 *            in float64 and rounded to float32), or custom float32 [N] (asdr_spectrogram_set_window; finite values only).  The
 *            window enters the statement as its float32 values.  Output kind: power or complex.
 *
 *   Frames.  With x the channel's whole sample sequence (x[i < 0] = 0) and frame f >= 0:
 *
 *                X_f[k] = (1 / N) sum over n = 0 .. N - 1 of w[n] x[f H + n] e^{-j 2 pi k n / N},   k = k0 .. k0 + B - 1
 *
 *            power writes |X_f[k]|^2 as float32; complex writes (re, im) as float32.  The scale is not window-corrected (as the
 *            fast-convolution bank's spectrum): a tone of amplitude A on a bin centre reads A^2 / 4 (rect) or
 *            A^2 / 16 (hann).  At 12 000 Hz N = 8192 is a WSPR symbol and its 1.4648 Hz tone spacing; at 12 800 Hz (a resampler
 *            with U / M = 128 / 441) N = 2048 is an FT8 symbol and its 6.25 Hz spacing.
 *
 *   Timing.  The bank is in lockstep: T = samples consumed so far (int64, one number for all channels).  F(T) = 0 for T < N, else
 *            floor((T - N) / H) + 1: the frames that lie wholly in the first T samples.  A call that takes T from T0 to
 *            T1 = T0 + n_samples writes frames F(T0) .. F(T1) - 1 of every channel as frames 0 .. of its output rows and returns
 *            their number, possibly 0, which the host knows beforehand (asdr_spectrogram_out_frames).  Splitting a sample sequence
 *            into calls of any sizes leaves every output bit-identical: a frame's arithmetic does not depend on where the call
 *            boundaries fall inside it.
 *
 *   State.   The per-channel record is the channel's last N input samples, oldest first, with zeros before position 0: int16[N].
 *            A frame that a call completes began at most N - 1 samples behind the call.  The record does not depend on T, H, the
 *            band, the window or the kind: it moves between spectrograms of one N freely.
 *
 * The pass.  asdr_spectrogram_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_gate_update_device:
 * a call on another stream than the previous one first waits (on the device) for the previous call's work.  dAudio: int16 rows
 * [n_channels][stride_samples] of which samples 0 .. n_samples - 1 are new; n_samples in 1 .. 2^24 (0 does nothing and returns 0),
 * stride_samples >= n_samples, 2-byte aligned (odd strides and odd offsets are fine).  dOut: float32 rows [..][out_stride_frames][B]
 * (power) or [..][out_stride_frames][B][2] (complex), out_stride_frames at least the returned count, 4-byte aligned, not overlapping
 * the audio span.  It returns the per-row frame count, or -1.
 *     dIndex == NULL:  row c of dOut is channel c, for all n_channels (capacity_rows is ignored).
 *     otherwise:       dIndex / dCount are device addresses (int32 [..] and one int32), exactly as in asdr_resampler_update_device:
 *                      a gate's list, or a list of the receivers somebody is watching.  Row i of dOut is channel dIndex[i] for
 *                      i < min(*dCount, capacity_rows); rows past that are not written.  There is no host round trip.
 * Every channel's carry advances in every call, written or not, so a channel that is watched later has the right history.  Frames
 * of a row past the returned count are not written.  The input rows are whole-bank rows (row c = channel c): the compact rows of a
 * resampler run behind an index are not an input.  There is no host-pointer entry: the consumer copies dOut.
 *
 * State calls.  read_state / write_state / reset / set_window / set_position wait for the spectrogram's work first.  write_state is
 * all or nothing: every channel is range-checked before one record is written.  reset gives zero records and T = 0 and keeps the
 * parameters and the window.  set_position(T) places a restored spectrogram (T in 0 .. 2^50): with write_state it is the
 * checkpoint / resume path.  An ASDR_NO_DEVICE spectrogram keeps its records on the host: every call but update_device works on it.
 */
#ifndef ASDR_SPECTROGRAM_H_
#define ASDR_SPECTROGRAM_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_SPECTROGRAM_MIN_N 128
#define ASDR_SPECTROGRAM_MAX_N 8192
#define ASDR_SPECTROGRAM_MAX_OVERLAP 16             /* H >= N / 16 */
#define ASDR_SPECTROGRAM_MAX_SAMPLES (1 << 24)      /* per call */
#define ASDR_SPECTROGRAM_MAX_POSITION (1LL << 50)

#define ASDR_SPECTROGRAM_RECT 0
#define ASDR_SPECTROGRAM_HANN 1
#define ASDR_SPECTROGRAM_CUSTOM 2                   /* what window_kind returns after set_window; not a creation value */

#define ASDR_SPECTROGRAM_POWER 0
#define ASDR_SPECTROGRAM_COMPLEX 1

typedef struct asdr_spectrogram asdr_spectrogram_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576; window RECT or HANN; kind POWER or COMPLEX */
asdr_spectrogram_t *asdr_spectrogram_create(int n_channels, int n_fft, int hop, int first_bin, int n_bins, int window, int kind, int device);
void asdr_spectrogram_destroy(asdr_spectrogram_t *s);
int asdr_spectrogram_n_channels(const asdr_spectrogram_t *s);

/* the parameters */
int asdr_spectrogram_n_fft(const asdr_spectrogram_t *s);
int asdr_spectrogram_hop(const asdr_spectrogram_t *s);
int asdr_spectrogram_first_bin(const asdr_spectrogram_t *s);
int asdr_spectrogram_n_bins(const asdr_spectrogram_t *s);
int asdr_spectrogram_window_kind(const asdr_spectrogram_t *s);
int asdr_spectrogram_output_kind(const asdr_spectrogram_t *s);
int asdr_spectrogram_get_window(const asdr_spectrogram_t *s, float *w /* [n_fft] */);
int asdr_spectrogram_set_window(asdr_spectrogram_t *s, const float *w /* [n_fft], finite */);

/* position */
long long asdr_spectrogram_position(const asdr_spectrogram_t *s);        /* T; -1 for a NULL spectrogram */
long long asdr_spectrogram_frame_position(const asdr_spectrogram_t *s);  /* F(T) */
long asdr_spectrogram_out_frames(const asdr_spectrogram_t *s, long n_samples); /* what the next call of that size returns */
int asdr_spectrogram_set_position(asdr_spectrogram_t *s, long long t);

/* the pass */
long asdr_spectrogram_update_device(asdr_spectrogram_t *s, const int16_t *dAudio, long stride_samples, long n_samples, float *dOut,
                                    long out_stride_frames, const int32_t *dIndex /* NULL: all channels */, const int32_t *dCount,
                                    int capacity_rows, void *stream);

/* state */
int asdr_spectrogram_read_state(asdr_spectrogram_t *s, int16_t *dst /* [n_channels][n_fft] */);
int asdr_spectrogram_write_state(asdr_spectrogram_t *s, const int *channels /* NULL: 0 .. n - 1 */, int n, const int16_t *src /* [n][n_fft] */);
int asdr_spectrogram_reset(asdr_spectrogram_t *s);
int asdr_spectrogram_synchronize(asdr_spectrogram_t *s);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_SPECTROGRAM_H_ */
