/* asdr_tuner.h -- C ABI of the digital tuner bank: per-receiver digital LO + decimating low-pass that turns shared wideband
 * CS16 I/Q into the 44.1 kHz int16 I and Q rows asdr_update_device / asdr_capture_update_device consume.  It stands in for the
 * reference's quadrature LO (EXTRAS/SI5351quad, tuned to `frequency - TuningOffset`, BareBonesWSPR.ino:102,116) and its codec.
 * Not a function of the reference library: the arithmetic is this project's own and is stated below, integer-only, so results
 * are bit-exact whatever the summation order.  Same library (libasdr_hip.so) and conventions as asdr.h / asdr_front.h: `ch` =
 * channel index or ASDR_ALL (-1) for setters, ASDR_NO_DEVICE for a control-plane-only bank whose update calls fail, errors
 * through asdr_last_error() (setters return 0 / -1).
 *
 * Arithmetic (all integer; sat16 clamps to [-32768, 32767]; >> is an arithmetic shift = floor):
 *   bank      n_channels channels, n_sources sources, one decimation D in [1, 64], one filter h[0..L-1] int16, L in [1, 1024],
 *             gain shift g in [0, 15].  Position P = input samples per source since creation / reset; x_s[m] = sample m of source s.
 *   NCO       C[k] = round(32767 cos(2 pi k / 4096)), S[k] = round(32767 sin(2 pi k / 4096)) (asdr_tuner_tables.h).
 *   channel   src, frequency word fw (uint32), anchor (pos_a, ph_a); theta(m) = ph_a + (m - pos_a) * fw mod 2^32 for m >= pos_a.
 *   mixer     k = theta(m) >> 20, x = x_src[m]:  zr = sat16((xr C[k] + xi S[k] + 16384) >> 15),
 *                                                zi = sat16((xi C[k] - xr S[k] + 16384) >> 15);   z[m] = 0 for m < pos_a.
 *   filter    s = 15 - g, r = s ? 1 << (s - 1) : 0:  I[n] = sat16((sum_{k<L} h[k] zr[nD + D - 1 - k] + r) >> s), Q[n] likewise on zi.
 *   retune    set_source / set_frequency / set_frequency_word / set_phase act at the current P: the channel is re-anchored
 *             (pos_a = P; ph_a = theta_old(P), or the given phase for set_phase) and its history flushed (z = 0 before P) -- even
 *             when the value does not change.  A new filter applies to outputs from P on; the sources' history is kept.
 *   creation  P = 0, every anchor (0, 0), fw 0, src 0, source history zeros.  Default filter: D = 1 -> h = {16384}, g = 1 (exact
 *             pass-through of z); D >= 2 -> a Kaiser low-pass of 12 D + 1 taps, g = 0 (DESIGN.md 3.8 gives its response).
 *
 * Rate banks (asdr_tuner_create_rate): wideband input at any integer rate Fs_in (Hz) that a decimation D in [1, 64] brings to
 * Fs_mid = Fs_in / D (Fs_in % D == 0) in [44100, 176400]; U / M = 44100 / Fs_mid in lowest terms, U <= 2048.  A plain bank is the
 * rate bank with Fs_in = D * 44100 (U = M = 1): the same defaults and the same output.
 *   stage 1   the arithmetic above, with Fs_in for the frequency word; it gives the channel's intermediate sequence u[i] (I and Q,
 *             int16) at Fs_mid.  N_u = P / D = u samples produced so far.
 *   stage 2   a polyphase rational resampler: prototype h2[0 .. U K - 1] int16, K taps per phase in [1, 64], gain shift g2 in
 *             [0, 15], every phase phi with sum_k |h2[k U + phi]| <= 65535.  Output j: b_j = floor(j M / U), phi_j = j M - b_j U,
 *             y[j] = sat16((sum_{k<K} h2[k U + phi_j] u[b_j - k] + r2) >> s2), s2 = 15 - g2, r2 = s2 ? 1 << (s2 - 1) : 0,
 *             u[i] = 0 for i < 0; I and Q separately.
 *   timing    a call consumes whole frames: 128 D input samples per source (128 new u samples).  Output block J (samples 128 J ..
 *             128 J + 127) is written by the first call after which b_{128 J + 127} <= N_u - 1, blocks in order: 0 .. n_frames + 1
 *             blocks per call, a count that depends on the positions only (asdr_tuner_out_blocks).
 *   state     a retune does not touch stage 2 (stage 1 flushes its own history as above); a new stage-2 filter applies to the
 *             outputs written from the next call on; reset zeroes P, the output position and the stage-2 history.  A stage 2
 *             with U = M = 1, K = 1 and h2 = {1 << s2} is a pass-through (the output is u) and keeps no history: the first call
 *             that runs another stage 2 after pass-through calls sees u[i] = 0 for every i before that call.
 *   defaults  Kaiser (beta 9) windowed sincs, 0 - 11.2 kHz passband, rejecting what would fold into 0 - 12 kHz at 44.1 kHz.
 *             Stage 1: Fs_mid = 44100 -> the plain default above; D = 1 -> {16384}, g = 1; otherwise stop band from
 *             Fs_mid - 12 kHz, cut-off midway between 11.2 kHz and that edge, L1 = 2 ceil(6 D Fs_mid 20900 / (44100 (Fs_mid -
 *             23200))) + 1 taps, g = 0.  Stage 2: U = M = 1 -> {16384}, g2 = 1; otherwise a prototype at U Fs_mid with cut-off
 *             21.65 kHz, K = 2 ceil(6 Fs_mid / 44100), each phase rounded to Q15 on its own and its largest tap corrected so the
 *             phase sums to exactly 32768, g2 = 0 (DESIGN.md 3.8 gives the responses).
 *
 * Fast-convolution banks (asdr_tuner_create_fastconv): stage 1 by overlap-save, one forward FFT per source and frame shared by all
 * of its channels, so a channel's cost follows its output rate, not Fs_in.  Floating point, unlike the integer-exact direct form:
 * the statement below is exact (float64); the kernels compute in float32 and agree with it within +-1 of u.
 *   bank      R a power of two in [2, 1024]; Fs_mid = Fs_in / R in [44100, 176400] (it may be fractional: Fs_in % R need not be
 *             0); U / M = 44100 R / Fs_in in lowest terms, U <= 2048 (2.4 MS/s, R = 16 -> 147 / 500; 20 MS/s, R = 128 -> 882 /
 *             3125; 61.44 MS/s, R = 512 -> 147 / 400).  decimation() returns R, rate() Fs_in.
 *   sizes     hop H = 128 R input samples, FFT size N = 2 H = 256 R (512 .. 262,144), q = 2^32 / N.
 *   frame b   counted from creation / reset; consumes input samples [b H, (b + 1) H) of every source.  Its window is
 *             x_s[(b - 1) H .. (b + 1) H - 1] (zeros before position 0), X = DFT_N(window), unnormalised, e^{-j 2 pi k n / N}.
 *   channel   src, fw, anchor (pos_a, ph_a) as above (the setters map Hz to fw as for rate banks).  Coarse bin
 *             k0 = floor(((int32) fw + q / 2) / q); residual rw = (int32)(fw - k0 q) in [-q / 2, q / 2).
 *   filter    real taps g[0 .. Lg - 1] (float), 1 <= Lg <= 129, at Fs_mid, one for the whole bank; its response
 *             G[m] = sum_n g[n] e^{-j 2 pi m n / 256}, m in [-128, 128), computed in float64 and rounded to float.
 *   output    y[n] = (1 / N) sum_{m=-128}^{127} X[(k0 + m) mod N] G[m] e^{+j 2 pi m n / 256} for n = 128 .. 255 (overlap-save: the
 *             first 128 are discarded); i = 128 b + n - 128 is the Fs_mid sample (input sample i R).  Times (-1)^{k0 (b - 1)}, so
 *             that the coarse shift is mixing by e^{-j 2 pi k0 m / N} at absolute input sample m; times e^{-j 2 pi theta_i / 2^32}
 *             with the fine NCO theta_i = ph_a + rw (i R - pos_a) mod 2^32 (evaluated from (int32) theta_i, |error| <= 2^-21);
 *             u[i] = sat16(rint(Re)), sat16(rint(Im)), round half to even.  The fine shift follows the filter: the filter acts at
 *             a tone's offset from the coarse bin (k0 Fs_in / N), at most Fs_mid / 512 from the tuned frequency; the one visible
 *             effect is a constant phase 2 pi (rw Fs_in / 2^32) tau_g on the channel (tau_g: the filter's group delay).
 *   stage 2   the rate-bank resampler, unchanged, with its timing and out_blocks rule: a call consumes whole frames (H input
 *             samples per source) and makes 128 new u samples per frame.  Fs_in = 44100 R defaults to a pass-through (output u).
 *   retune    set_source / set_frequency(_word) / set_phase act at the current P, always a frame boundary: pos_a = P, ph_a =
 *             theta_P of the fine NCO (continuous) or the given phase.  Unlike the direct form no history is flushed: a
 *             fast-convolution channel has none of its own.  Reset zeroes P, the output position, the sources' windows (the last
 *             H samples per source) and the stage-2 carry.
 *   defaults  channel filter: Kaiser (beta 7.857) windowed sinc, 129 taps, sum g = 1, cut-off 11.5 kHz + delta / 2 with delta =
 *             0.0392 Fs_mid (Kaiser's 80 dB transition width for 129 taps): flat over |f| <= 11.5 kHz (0 - 11.2 kHz after the
 *             fine shift), stop band from 11.5 kHz + delta to Fs_mid / 2.  Stage 2: the rate banks' rule at this Fs_mid, i.e.
 *             K = 2 ceil(6 Fs_in / (44100 R)), cut-off 21.65 kHz at U Fs_mid.
 *   ABI       every other function works as for rate banks, except set_filter / get_filter, which fail (use
 *             set_channel_filter / get_channel_filter), and update(_device), which need a pass-through stage 2.
 *
 * Input formats (asdr_tuner_set_input_format): a format says how one input sample is stored and how it becomes the x = (xr, xi)
 * (two int16) that every statement above starts from.  Everything after x is unchanged.
 *   format                            stored as       bytes / sample   x
 *   ASDR_TUNER_IN_CS16 = 0 (default)  int16 re, im    4                as stored
 *   ASDR_TUNER_IN_CU8                 uint8 re, im    2                256 a - 32640 per part ( = 128 (2 a - 255), the usual a - 127.5
 *                                                                      convention; range +-32640)
 *   ASDR_TUNER_IN_CS8                 int8 re, im     2                256 a per part
 *   ASDR_TUNER_IN_CF32                float re, im    8                sat16(rint(32768 a)) per part, round half to even, NaN -> 0,
 *                                                                      +-inf saturate (the product is exact, so this is one rounding)
 *   ASDR_TUNER_IN_RS16                int16, real     2                xr = a, xi = 0
 * A "sample" in in_stride_samples, in frame sizes (128 D, H = 128 R) and in P is one stored sample of the format (one pair, or one
 * real value).  The format applies to the rows of the next call; the history rows / windows kept across calls hold converted
 * samples (x), so a change of format between two calls is well defined by the above and needs no flush.  reset keeps the format.
 * The conversion happens in the loads of the kernels that read the caller's rows.  A fast-convolution bank
 * computes X of an RS16 window by a transform of N / 2 complex points on z[n] = w[2n] + j w[2n + 1] and the untangling step
 * X[k] = (Z[k] + conj Z[N/2 - k]) / 2 - (j / 2) W_N^k (Z[k] - conj Z[N/2 - k]), X[N - k] = conj X[k]: the same X in exact
 * arithmetic, so the statement of X above holds as it stands. *
 * Monitors (fast-convolution banks only; both off at creation).  They observe what stage 1 computes anyway and change nothing of
 * it: a bank that enables neither launches and allocates as before, and a bank with both on writes bit for bit the same I and Q.
 * The statements are exact (float64); the kernels compute |.|^2 and the sums inside one frame in float32 and accumulate frames in
 * float64 (DESIGN.md 3.8.4 gives the tolerance).
 *   spectrum  per source s and frame b, from the X of "frame b" above (so formats, RS16, history across calls and the zeros before
 *             position 0 are as stated there).  Window rect: W[k] = X[k].  Window hann: W[k] = X[k] / 2 - (X[(k - 1) mod N] +
 *             X[(k + 1) mod N]) / 4, the DFT of the window's samples times 0.5 - 0.5 cos(2 pi n / N); the frames overlap by half, so
 *             a hann sum is Welch's estimator at 50 % overlap.  p_b[k] = |W[k]|^2 / N^2: a complex tone of amplitude A on a bin
 *             centre reads A^2 with rect and A^2 / 4 with hann (not corrected).  B output bins, a power of two in [256, N],
 *             g = N / B: P_b[j] = sum_{k = j g}^{j g + g - 1} p_b[k], j in FFT order (j = 0 starts at the capture's centre
 *             frequency, bin width Fs_in / B; j >= B / 2 are the negative frequencies), as asdr_grab_spectrum orders its bins.
 *             Mode sum: acc[s][j] += P_b[j]; mode peak: acc[s][j] = max(acc[s][j], P_b[j]); frames in order; a bank-wide count of
 *             accumulated frames goes up by one per frame in both.  acc is float64.
 *   level     per channel c and frame b, with y[n], n = 128 .. 255, the "output" line's y (1 / N included) before the fine NCO,
 *             the rounding and the clamp (the NCO has unit modulus, the coarse sign too): e_b[c] = sum_n |y[n]|^2, in int16^2
 *             units; level[c] += e_b[c] in float64, with a bank-wide frame count of its own.  level[c] / (128 frames) is the mean
 *             power per Fs_mid sample; it is taken before the clamp, so it passes 32767^2 where the output saturates.  A retune
 *             does not clear a channel's level: clear after retuning.
 *   state     enable / disable / re-configuration clear that monitor's accumulators and count and apply from the next update call;
 *             asdr_tuner_reset clears both monitors and keeps their configuration; retunes, filter and format changes touch
 *             neither.  Direct-form and rate banks have no X: every monitor function fails on them (asdr_last_error).  An
 *             ASDR_NO_DEVICE bank takes the configuration calls and fails the reads, the clears and the device getters.
 *
 * Filter palette and gain (fast-convolution banks only; everything not named here is unchanged).  In the frequency domain another
 * filter for a channel is another row of a small table: a bank holds up to 64 responses and every channel names one, and a gain.
 *   palette   slots 0 .. 63 (ASDR_TUNER_FC_MAX_FILTERS).  Slot 0 is the bank's channel filter: the default, or what
 *             asdr_tuner_set_channel_filter set; only that function touches it.  Slots 1 .. 63 are undefined at creation.  A slot
 *             holds Lg taps, 1 <= Lg <= 129, at Fs_mid, real or complex (interleaved re, im floats); its response is
 *             G_s[m] = sum_n g[n] e^{-j 2 pi m n / 256}, m in [-128, 128), computed in float64 with each part rounded to float:
 *             the rule of "filter" above, with complex g.
 *   channel   a slot f_c and a gain a_c; 0 and 1.0 at creation.  a_c is a finite float with |a_c| <= 32768; negative values and
 *             zero are allowed.  In the "output" line G[m] becomes G_{f_c}[m]; after the 1 / N scale and the coarse sign y is
 *             multiplied by a_c; then the fine NCO, the rounding and the clamp follow as stated there.
 *   level     the level monitor takes y with G_{f_c} but without a_c: the level is the signal's, so a change of gain needs no
 *             recalibration.
 *   timing    setting a channel's slot, defining a slot, redefining a slot (every channel on it follows) and setting a gain apply
 *             to the frames of the next update call.  No history is flushed and no NCO re-anchored: overlap-save keeps no
 *             per-channel state.  asdr_tuner_reset puts every channel back to slot 0 and gain 1 (the creation state) and keeps the
 *             palette's slots, as it keeps the filter.
 *   place     as today the filter acts at a tone's offset from the coarse bin, at most Fs_mid / 512 from the tuned frequency: a
 *             passband meant for [lo, hi] about the tuned frequency should be Fs_mid / 512 wider on each side.
 *   sharpness 129 taps at Fs_mid set the transition width: 0.0392 Fs_mid for 80 dB, i.e. 1.7 kHz at Fs_mid = 44.1 kHz and 5.9 kHz
 *             at 150 kHz.  The palette chooses among bandwidths of a few kHz and up, and sidedness (a complex slot states a
 *             one-sided SSB passband, which real taps cannot); it is not a 100 Hz CW filter.  An R that puts Fs_mid near 44.1 -
 *             75 kHz gives the sharper filters.
 *   cost      a bank whose channels are all on slot 0 at gain 1 launches and allocates exactly as before; any other bank runs
 *             one other channel kernel in the old one's place.  A channel on slot 0 at gain 1 of such a bank
 *             is written bit for bit as before.
 *
 * Source conditioning (every bank kind; everything not named here is unchanged).  Zero-IF radios add a DC offset and an I/Q gain
 * and phase imbalance to what they deliver; a bank holds one correction per source, applied to x before anything else reads it, and
 * can measure x to find that correction.  All integer; >> is an arithmetic shift.
 *   correction per source s: (d_r, d_i, p, g) = (dc_re, dc_im, cross_q16, gain_q16), d_r, d_i in [-32768, 32767], p in [-32768,
 *             32768], g in [32768, 131072]; the identity (0, 0, 0, 65536) at creation.  With x = (xr, xi) the int16 pair of the
 *             "Input formats" table:
 *                 a = xr - d_r,  b = xi - d_i                       (not clamped: 18-bit values)
 *                 xr' = sat16(a)
 *                 xi' = sat16((p a + g b + 32768) >> 16)            (in int64: |g b| reaches 2^33)
 *             x' takes the place of x in every statement above, for all three bank kinds.  The identity gives x' = x exactly.  For
 *             RS16 only d_r acts: xr' = sat16(xr - d_r), xi' = 0.
 *   timing    a correction applies to the rows of the next update call; the history rows and overlap-save windows kept across
 *             calls hold x', so a change between two calls is well defined by the above and flushes nothing.  asdr_tuner_reset
 *             keeps the corrections, as it keeps the format.
 *   statistics  off at creation, bank-wide.  Per source, over every sample the bank consumes while they are on, taken of x
 *             (converted, before the correction): n, sum xr, sum xi, sum xr^2, sum xi^2, sum xr xi, and `clipped`, the number of
 *             stored samples with a part at the format's rail: CU8 a in {0, 255}, CS8 {-128, 127}, CS16 / RS16 {-32768, 32767}, CF32
 *             |a| >= 1 or not finite.  All seven are int64 and exact; they wrap modulo 2^64, sum xr^2 first: past 2^63 after 2^33
 *             samples at -32768 (7 minutes at 20 MS/s), so the caller reads or clears before then.  Being taken of x they make the
 *             estimate below absolute: tracking twice converges and does not compound.  For RS16 the three sums with xi are 0.
 *             Enabling, disabling and asdr_tuner_reset clear the statistics; retunes, filter, format and correction changes do not.
 *   estimator a pure host function in float64, every sum converted to double first, each operation rounded once (no contraction):
 *                 m_r = sum xr / n,  m_i = sum xi / n
 *                 v_rr = sum xr^2 / n - m_r m_r,  v_ii = sum xi^2 / n - m_i m_i,  v_ri = sum xr xi / n - m_r m_i
 *                 det = v_rr v_ii - v_ri v_ri,  gh = v_rr / sqrt(det),  ph = (-gh v_ri) / v_rr
 *                 d_r = rint(m_r),  d_i = rint(m_i),  p = rint(65536 ph),  g = rint(65536 gh)          (round half to even)
 *             the blind estimate that leaves the corrected Q uncorrelated with I and equal to it in power: right for signals that
 *             are circular about DC, which a band full of independent stations is.  It fails (output untouched) when n < 2, when
 *             v_rr <= 0, when det <= 0, or when a word falls outside its range.  Statistics whose three sums with xi are all zero
 *             (RS16) give d_r, d_i = 0 and the identity for p and g, and need only n >= 2 and d_r in range.
 *   cost      a bank with every correction at the identity and the statistics off launches and allocates exactly as before.  With
 *             the statistics on and every correction at the identity one more kernel reads the caller's rows and sums; the bank's
 *             kernels read the caller's rows as before.  With any correction off the identity that kernel also writes x' of every
 *             source (the identity ones: a converted copy) as CS16 (RS16 for an RS16 bank) to a scratch of the bank's, and the
 *             bank's unchanged kernels read the scratch.  An ASDR_NO_DEVICE bank takes the setters, enable and
 *             the estimator and fails the reads, the clear and track.
 *
 * State records (every bank kind; everything not named here is unchanged): what asdr.h's receiver state records are to a receiver,
 * for the tuner in front of it.  A bank's state leaves it in two parts: one variable-size BANK-STATE BLOB (everything that is
 * bank-wide or per source) and one fixed-size CHANNEL RECORD per channel.  A channel restored from both writes as its next output
 * the sample the uninterrupted bank would have written, bit for bit.  Both are little-endian, every pad byte is zero, every section
 * starts 16-byte aligned, and no byte depends on the bank's internal double-buffer parities: two banks that were given the same
 * samples in calls of different sizes export the same bytes.  An export changes nothing the bank computes; an import is a
 * transaction: everything is checked on the host before a word of the bank is written, and a refused import (-1, asdr_last_error
 * names the record or the section) leaves the bank computing exactly what it would have.
 *   channel   ASDR_TUNER_CHANNEL_RECORD_BYTES = 2560 bytes:
 *     0 ..   15  magic "ASTC" (u32 ASDR_TUNER_CHANNEL_MAGIC), version 1, bytes (2560), content bits
 *    16 ..   63  where the record was taken: kind i32 (0 direct / rate, 1 fast-convolution), D or R i32, Fs_in i64, U i32, M i32,
 *                P i64, output position i64, pad
 *    64 ..   95  src i32, fw u32, pos_a i64, ph_a u32, palette slot i32, gain f32, pad
 *    96 ..  103  level accumulator f64 (0 when the levels are off)
 *   104 ..  255  zero
 *   256 .. 2559  the stage-2 carry: 576 dwords, slot i = u sample N_u - 576 + i (I low, Q high); zeros when the carry is
 *                logically zero (before the first stage-2 call, after pass-through calls) or absent (a pass-through stage 2)
 *             content bits: ASDR_TUNER_REC_HAS_SIGNAL (1) the record came from a bank with a device; ASDR_TUNER_REC_HAS_CARRY (2)
 *             the carry section is stage-2 history (the bank had a real stage 2); ASDR_TUNER_REC_HAS_LEVEL (4) the level is valid.
 *             asdr_tuner_channel_record_field lists the head's fields.
 *   import    checks, all before any write: n >= 1; every index in range; no destination named twice (one RECORD may be named
 *             for many destinations: cloning); magic, version, bytes, content bits; kind, D / R, Fs_in, U, M equal to the
 *             destination's; P and the output position equal to the destination's NOW; 0 <= pos_a <= P; src below the
 *             destination's n_sources; slot a defined palette slot on a fast-convolution bank, 0 elsewhere; gain finite with
 *             |gain| <= 32768 (exactly 1 elsewhere).  The position rule makes an anchor and a carry mean in the destination what
 *             they meant in the origin; it holds between a bank and one restored from its blob, and between banks fed in lockstep
 *             from the same sources (the shards of one deployment).  Moving a channel between banks at different positions is not
 *             supported.  Then the channel's row (src, fw, anchor), slot and gain are replaced verbatim -- no re-anchoring and no
 *             flush: a direct-form channel's flushed history is already in pos_a -- the level is written when the destination has
 *             the levels on, and the carry row when it has a real stage 2 (allocated first if need be; if the pass-through calls
 *             before had left it stale the whole carry is first made the zeros it logically is, so the other channels still see
 *             zeros).  A pass-through destination ignores the carry section.  A record without HAS_SIGNAL configures the channel
 *             and gives it a zero carry and a zero level; an ASDR_NO_DEVICE bank exports and imports the head only.
 *   ordering  the host forms synchronise with the bank's work and return when done.  The device forms run on `stream` under the
 *             update calls' rule: `stream` first waits for the previous call's work if that ran on another stream, and the next
 *             call on any stream is ordered after them.  The device import first brings every record's head to the host (a
 *             strided copy and a wait on `stream`), validates, and only then launches.  Device records: 16-byte aligned, on the
 *             bank's device.
 *   blob      asdr_tuner_bank_state_bytes() bytes; it holds no channel count and nothing per channel.  A 256-byte header:
 *     0 ..   15  magic "ASTB" (u32 ASDR_TUNER_BANK_MAGIC), version 1, total bytes u64
 *    16 ..   31  content bits (ASDR_TUNER_BLOB_HAS_SIGNAL 1: the per-source device state is present; ASDR_TUNER_BLOB_CARRY_STALE 2:
 *                pass-through calls had left the stage-2 history stale), kind i32, D or R i32, n_sources i32
 *    32 ..   63  Fs_in i64, U i32, M i32, P i64, output position i64
 *    64 ..   87  input format i32, history dwords per source i32 (1024, or 128 R), stage-1 gain shift g i32 (0 for a
 *                fast-convolution bank), stage-1 taps i32 (L, or Lg), g2 i32, K i32
 *    88 ..  103  spectrum bins i32 (0: off), window i32, mode i32, levels on i32
 *   104 ..  127  spectrum frames i64, level frames i64, I/Q statistics on i32, pad
 *   128 ..  255  the directory: eight (offset u64, bytes u64) pairs, in this order and laid out back to back from byte 256, each
 *                section's size rounded up to 16: [0] the stage-1 filter (1024 int16 h, or 129 float g; unused taps zero), [1]
 *                the stage-2 prototype (U x 64 int16: h2[k U + phi] at word k U + phi, K taps per phase used), [2] the palette
 *                (fast-convolution banks: slots 1 .. 63, each Lg i32 (0: undefined), complex i32, pad, 258 floats), [3] the
 *                corrections (n_sources asdr_tuner_iq_t), [4] the statistics (n_sources asdr_tuner_iq_stats_t; only while on and
 *                HAS_SIGNAL), [5] the spectrum accumulators (n_sources x B f64; likewise), [6] the history rows (n_sources x
 *                history dwords, oldest sample first: converted, corrected samples, re low, im high; only with HAS_SIGNAL), [7]
 *                unused (0, 0)
 *             import: kind, D / R, Fs_in, U, M and n_sources must equal the destination's (n_channels is free); the whole blob is
 *             validated first (sizes, directory, filter limits as the setters have them, tap counts, gain shifts, correction
 *             words, monitor configuration, positions on a frame boundary); then it acts as asdr_tuner_reset followed by
 *             installing the blob: P, the output position, the format, the filters and the palette, the corrections, the
 *             statistics switch and sums, the monitors' configuration, accumulators and frame counts, the history rows.  Every
 *             channel is then in creation state at the new P, to be filled by asdr_tuner_import_channels; the level accumulators
 *             are per channel and travel in the channel records.  A blob whose stage 2 was stale or a pass-through restores that
 *             condition.  A blob without HAS_SIGNAL (from an ASDR_NO_DEVICE bank) carries the settings only: the histories stay
 *             the zeros of a reset.  Order of a whole restore: the bank's blob, then its channels, then the receivers' records
 *             (asdr_import_state) behind them.
 */
#ifndef ASDR_TUNER_H_
#define ASDR_TUNER_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_TUNER_MAX_DECIMATION 64
#define ASDR_TUNER_MAX_TAPS 1024
#define ASDR_TUNER_MAX_GAIN_SHIFT 15
#define ASDR_TUNER_HISTORY 1023 /* input samples per source kept across calls (L - 1 at most) */
#define ASDR_TUNER_MAX_UP 2048
#define ASDR_TUNER_MAX_RESAMPLER_TAPS 64 /* K, taps per phase */
#define ASDR_TUNER_FC_MAX_R 1024
#define ASDR_TUNER_FC_MAX_TAPS 129       /* Lg, channel filter taps of a fast-convolution bank */
#define ASDR_TUNER_FC_MAX_FILTERS 64     /* palette slots of a fast-convolution bank; slot 0 is the channel filter */
#define ASDR_TUNER_FC_MAX_GAIN 32768.0f  /* |a_c| at most */
#define ASDR_TUNER_IN_CS16 0             /* input formats (the table above) */
#define ASDR_TUNER_IN_CU8 1
#define ASDR_TUNER_IN_CS8 2
#define ASDR_TUNER_IN_CF32 3
#define ASDR_TUNER_IN_RS16 4

typedef struct asdr_tuner_bank asdr_tuner_t;

typedef struct {
  int32_t src;          /* source row */
  uint32_t fw;          /* frequency word: phase step per input sample, 2^32 = one turn */
  int64_t pos_a;        /* anchor position (input samples) */
  uint32_t ph_a;        /* NCO phase at pos_a */
  uint32_t reserved;
} asdr_tuner_state_t;

/* lifetime; NULL on failure (asdr_last_error) */
asdr_tuner_t *asdr_tuner_create(int n_channels, int n_sources, int decimation, int device);
void asdr_tuner_destroy(asdr_tuner_t *t);
int asdr_tuner_reset(asdr_tuner_t *t);            /* P = 0, creation state for every channel and source; the filter is kept */
long long asdr_tuner_position(const asdr_tuner_t *t);  /* P */
int asdr_tuner_n_channels(const asdr_tuner_t *t);
int asdr_tuner_n_sources(const asdr_tuner_t *t);
int asdr_tuner_decimation(const asdr_tuner_t *t);

/* control plane (all take effect at the current P) */
int asdr_tuner_set_source(asdr_tuner_t *t, int ch, int source);
/* hz in [-Fs_in/2, Fs_in/2], Fs_in = the bank's rate (D * 44100 for a plain bank): fw = (uint32)(int64)llround(hz * 2^32 / Fs_in).  To receive RF f of a capture
 * centred at fc with the chain behind it: hz = f - fc - asdr_getTuningOffset(). */
int asdr_tuner_set_frequency(asdr_tuner_t *t, int ch, double hz);
int asdr_tuner_set_frequency_word(asdr_tuner_t *t, int ch, uint32_t fw);
int asdr_tuner_set_phase(asdr_tuner_t *t, int ch, uint32_t phase);
/* Rejected (old filter kept): L or g out of range, sum |h[k]| > 65535 (32-bit accumulation is then exact). */
int asdr_tuner_set_filter(asdr_tuner_t *t, const int16_t *h, int n_taps, int gain_shift);
/* Copies min(L, cap) taps to h (if not NULL) and g to *gain_shift (if not NULL); returns L. */
int asdr_tuner_get_filter(const asdr_tuner_t *t, int16_t *h, int cap, int *gain_shift);
int asdr_tuner_read_state(const asdr_tuner_t *t, asdr_tuner_state_t *dst /* [n_channels] */);

/* The hot path.  dIQ: n_sources rows of interleaved re, im int16 (CS16), in_stride_samples complex samples apart, each holding
 * n_blocks * 128 * D new samples.  dI, dQ: [n_channels][out_stride_blocks][128] int16 (as asdr_update_device_strided takes them);
 * blocks 0..n_blocks-1 of every row are written.  Device pointers 16-byte aligned; the output spans must not overlap the input span.
 *  _update_device : asynchronous on `stream` (a hipStream_t; NULL = the null stream).  A call on another stream than the
 *                   previous one first waits (event) for that call's work.
 *  _update        : host pointers, contiguous rows (in_stride = n_blocks * 128 * D, out_stride = n_blocks); synchronous. */
int asdr_tuner_update_device(asdr_tuner_t *t, const int16_t *dIQ, long in_stride_samples, int16_t *dI, int16_t *dQ, int n_blocks,
                             long out_stride_blocks, void *stream);
int asdr_tuner_update(asdr_tuner_t *t, const int16_t *IQ, int16_t *I, int16_t *Q, int n_blocks);

/* Rate banks.  NULL (asdr_last_error) for each violated constraint above; ASDR_NO_DEVICE gives a control-plane-only bank. */
asdr_tuner_t *asdr_tuner_create_rate(int n_channels, int n_sources, long long fs_in_hz, int decimation, int device);
long long asdr_tuner_rate(const asdr_tuner_t *t);                /* Fs_in (D * 44100 for a plain bank) */
int asdr_tuner_ratio(const asdr_tuner_t *t, int *up, int *down);  /* U and M (either pointer may be NULL) */
long long asdr_tuner_output_position(const asdr_tuner_t *t);      /* output samples written since creation / reset */
/* Rejected (old resampler kept): n_taps % U != 0, K = n_taps / U or g2 out of range, a phase with sum |h2| > 65535. */
int asdr_tuner_set_resampler(asdr_tuner_t *t, const int16_t *h2, int n_taps, int gain_shift);
/* Copies min(U K, cap) taps to h2 (if not NULL) and g2 to *gain_shift (if not NULL); returns U K. */
int asdr_tuner_get_resampler(const asdr_tuner_t *t, int16_t *h2, int cap, int *gain_shift);
/* Blocks the next call of n_frames frames will write (host arithmetic only; exact for 64-bit positions). */
int asdr_tuner_out_blocks(const asdr_tuner_t *t, int n_frames);
/* The rate hot path: n_frames frames of dIQ (as asdr_tuner_update_device, n_frames * 128 * D samples per source) in, the blocks
 * the call writes out: blocks 0 .. n - 1 of each [n_channels][out_stride_blocks][128] row of dI, dQ; returns n (>= 0) or -1.
 * Fails, with no work done and the state unchanged, when n > out_capacity_blocks or out_stride_blocks < out_capacity_blocks.
 *  _update_rate_device : asynchronous on `stream`, with the stream rule of asdr_tuner_update_device (the wait is on the previous
 *                        call's last kernel).  It also takes plain banks, where it gives asdr_tuner_update_device's output.
 *  _update_rate        : host pointers, contiguous rows (n blocks apart, in_stride = n_frames * 128 * D); synchronous.
 * asdr_tuner_update_device / asdr_tuner_update need a pass-through stage 2 and fail otherwise. */
int asdr_tuner_update_rate_device(asdr_tuner_t *t, const int16_t *dIQ, long in_stride_samples, int n_frames, int16_t *dI,
                                  int16_t *dQ, int out_capacity_blocks, long out_stride_blocks, void *stream);
int asdr_tuner_update_rate(asdr_tuner_t *t, const int16_t *IQ, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks);

/* Fast-convolution banks.  NULL (asdr_last_error) for each violated constraint above; ASDR_NO_DEVICE gives a control-plane-only
 * bank. */
asdr_tuner_t *asdr_tuner_create_fastconv(int n_channels, int n_sources, long long fs_in_hz, int R, int device);
int asdr_tuner_fft_size(const asdr_tuner_t *t);   /* N, or 0 for a direct-form bank */
/* Rejected (old filter kept): Lg outside 1..129, a non-finite tap, a direct-form bank.  Applies from the next call on. */
int asdr_tuner_set_channel_filter(asdr_tuner_t *t, const float *g, int n_taps);
/* Copies min(Lg, cap) taps to g (if not NULL); returns Lg (fails on a direct-form bank). */
int asdr_tuner_get_channel_filter(const asdr_tuner_t *t, float *g, int cap);

/* Input formats (every bank kind, ASDR_NO_DEVICE banks included).  set: 0 / -1; an unknown value is rejected and the old format
 * kept.  It may be called between any two update calls and applies to the rows of the next one. */
int asdr_tuner_set_input_format(asdr_tuner_t *t, int format);
int asdr_tuner_input_format(const asdr_tuner_t *t);   /* ASDR_TUNER_IN_*, -1 for a NULL bank */
/* The hot path in the bank's format: the contract of asdr_tuner_update_rate_device / asdr_tuner_update_rate (all three bank kinds,
 * returns the blocks written, the same stream rule and the same cases that fail with no work done), with rows of n_frames * 128 * D
 * stored samples of the bank's format.  Row starts must be 16-byte aligned: the base pointer, and in_stride_samples times the
 * format's bytes per sample a multiple of 16; otherwise the call fails with no work done.
 * The four int16 update entry points above keep working on CS16 banks and fail, with the state unchanged, on a bank of another
 * format (asdr_last_error names it): an int16 pointer is never read as bytes or floats. */
int asdr_tuner_update_samples_device(asdr_tuner_t *t, const void *dIn, long in_stride_samples, int n_frames, int16_t *dI, int16_t *dQ,
                                     int out_capacity_blocks, long out_stride_blocks, void *stream);
int asdr_tuner_update_samples(asdr_tuner_t *t, const void *In, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks);

/* Monitors (the "Monitors" section above).  All return 0 / -1 unless said otherwise and fail on a bank that is not a
 * fast-convolution bank. */
#define ASDR_TUNER_WIN_RECT 0
#define ASDR_TUNER_WIN_HANN 1
#define ASDR_TUNER_MON_SUM 0
#define ASDR_TUNER_MON_PEAK 1
/* n_bins = B, a power of two in [256, N], or 0 to switch the monitor off (window and mode are then not looked at).  Rejected with
 * the old configuration and accumulators kept: any other B, an unknown window or mode.  Synchronises with the bank's work. */
int asdr_tuner_spectrum_enable(asdr_tuner_t *t, int n_bins, int window, int mode);
int asdr_tuner_spectrum_bins(const asdr_tuner_t *t);      /* B, 0 when off (and for a NULL or direct-form bank) */
int asdr_tuner_spectrum_window(const asdr_tuner_t *t);    /* ASDR_TUNER_WIN_*, -1 when off */
int asdr_tuner_spectrum_mode(const asdr_tuner_t *t);      /* ASDR_TUNER_MON_*, -1 when off */
/* Waits for the bank's work, then copies acc to dst [n_sources][B] (if not NULL) and the frame count to *frames (if not NULL);
 * clear != 0 then clears both.  Fails when the monitor is off. */
int asdr_tuner_spectrum_read(asdr_tuner_t *t, double *dst, long long *frames, int clear);
/* acc [n_sources][B] in device memory, valid in stream order after an update call, until the next enable / destroy; NULL
 * (asdr_last_error) when off or without a device. */
const double *asdr_tuner_spectrum_device(asdr_tuner_t *t);
long long asdr_tuner_spectrum_frames(const asdr_tuner_t *t);   /* frames accumulated by the update calls so far; -1 when off */
int asdr_tuner_spectrum_clear(asdr_tuner_t *t);           /* waits for the bank's work; accumulators and count to 0 */
int asdr_tuner_levels_enable(asdr_tuner_t *t, int on);
int asdr_tuner_levels_enabled(const asdr_tuner_t *t);     /* 1 / 0 (0 for a NULL or direct-form bank) */
/* As asdr_tuner_spectrum_read: dst [n_channels] in channel order (not the kernels' schedule order). */
int asdr_tuner_levels_read(asdr_tuner_t *t, double *dst, long long *frames, int clear);
const double *asdr_tuner_levels_device(asdr_tuner_t *t);
long long asdr_tuner_levels_frames(const asdr_tuner_t *t);
int asdr_tuner_levels_clear(asdr_tuner_t *t);

/* Filter palette and gain (the section above).  All fail on a bank that is not a fast-convolution bank; an ASDR_NO_DEVICE bank
 * takes all of them.  Setters return 0 / -1; a rejected call keeps the old state.
 * palette_set: slot in 1 .. 63 (slot 0 belongs to asdr_tuner_set_channel_filter); n_taps = Lg in 1 .. 129; taps holds Lg floats, or
 * 2 Lg (re, im) when is_complex != 0; every value finite.  Redefining a slot is allowed while channels are on it.
 * palette_get: slot in 0 .. 63; copies min(Lg, cap) taps (cap counts taps: pairs of floats for a complex slot) to taps (if not
 * NULL) and 0 / 1 to *is_complex (if not NULL); returns Lg, 0 for an undefined slot, -1 on error.  Slot 0 reads the channel filter.
 * palette_clear: slot in 1 .. 63 back to undefined; fails while a channel is on it.
 * set_channel_slot: ch or ASDR_ALL; the slot must be 0 or defined.  set_channel_gain: finite, |gain| <= 32768. */
int asdr_tuner_palette_set(asdr_tuner_t *t, int slot, const float *taps, int n_taps, int is_complex);
int asdr_tuner_palette_get(const asdr_tuner_t *t, int slot, float *taps, int cap, int *is_complex);
int asdr_tuner_palette_clear(asdr_tuner_t *t, int slot);
int asdr_tuner_set_channel_slot(asdr_tuner_t *t, int ch, int slot);
int asdr_tuner_read_slots(const asdr_tuner_t *t, int32_t *dst /* [n_channels] */);
int asdr_tuner_set_channel_gain(asdr_tuner_t *t, int ch, float gain);
int asdr_tuner_read_gains(const asdr_tuner_t *t, float *dst /* [n_channels] */);

/* Source conditioning (the section above; every bank kind).  Setters return 0 / -1; a rejected call keeps the old state. */
typedef struct { int32_t dc_re, dc_im, cross_q16, gain_q16; } asdr_tuner_iq_t;
typedef struct { int64_t n, sum_re, sum_im, sum_re2, sum_im2, sum_reim, clipped; } asdr_tuner_iq_stats_t;
/* source: a source index, or ASDR_ALL for set.  Rejected: a word outside its range, a bad source. */
int asdr_tuner_set_iq_correction(asdr_tuner_t *t, int source, const asdr_tuner_iq_t *c);
int asdr_tuner_get_iq_correction(const asdr_tuner_t *t, int source, asdr_tuner_iq_t *c);
/* on != 0: the statistics run from the next update call; either value clears them.  Synchronises with the bank's work. */
int asdr_tuner_iq_stats_enable(asdr_tuner_t *t, int on);
int asdr_tuner_iq_stats_enabled(const asdr_tuner_t *t);   /* 1 / 0 (0 for a NULL bank) */
/* Waits for the bank's work, copies the statistics to dst [n_sources]; clear != 0 then clears them.  Fails when they are off. */
int asdr_tuner_iq_stats_read(asdr_tuner_t *t, asdr_tuner_iq_stats_t *dst /* [n_sources] */, int clear);
int asdr_tuner_iq_stats_clear(asdr_tuner_t *t);
/* The estimator: no bank, no device.  0, or -1 (asdr_last_error) with *c untouched. */
int asdr_tuner_iq_estimate(const asdr_tuner_iq_stats_t *s, asdr_tuner_iq_t *c);
/* Reads the statistics, estimates and sets the correction of `source` (or of every source, ASDR_ALL), clears the statistics.  A
 * source whose estimate fails keeps its correction.  Returns the number of sources it set, -1 when the read fails. */
int asdr_tuner_iq_track(asdr_tuner_t *t, int source);
long long asdr_tuner_condition_launches(const asdr_tuner_t *t);   /* pre-pass launches since creation */

/* State records (the section above).  channels: a host array of n indices in any order, or NULL for channels 0 .. n - 1. */
#define ASDR_TUNER_CHANNEL_RECORD_BYTES 2560
#define ASDR_TUNER_CHANNEL_MAGIC 0x43545341u /* "ASTC" */
#define ASDR_TUNER_BANK_MAGIC 0x42545341u    /* "ASTB" */
#define ASDR_TUNER_STATE_VERSION 1u
#define ASDR_TUNER_CHANNEL_OFF_ORIGIN 16
#define ASDR_TUNER_CHANNEL_OFF_CONTROL 64
#define ASDR_TUNER_CHANNEL_OFF_LEVEL 96
#define ASDR_TUNER_CHANNEL_OFF_CARRY 256
#define ASDR_TUNER_REC_HAS_SIGNAL 1u
#define ASDR_TUNER_REC_HAS_CARRY 2u
#define ASDR_TUNER_REC_HAS_LEVEL 4u
#define ASDR_TUNER_BLOB_HEADER_BYTES 256
#define ASDR_TUNER_BLOB_HAS_SIGNAL 1u
#define ASDR_TUNER_BLOB_CARRY_STALE 2u
size_t asdr_tuner_channel_record_bytes(void);   /* 2560 */
/* Field i of a channel record's head as "name:type" (u32, i32, i64, f32, f64), its byte offset and element count; NULL past the
 * last.  The fields cover bytes 0 .. 255 without gaps or overlaps (pads are fields named pad*). */
const char *asdr_tuner_channel_record_field(int i, int *offset, int *count);
int asdr_tuner_export_channels(asdr_tuner_t *t, const int *channels, int n, void *host_records);
int asdr_tuner_import_channels(asdr_tuner_t *t, const int *channels, int n, const void *host_records);
int asdr_tuner_export_channels_device(asdr_tuner_t *t, const int *channels, int n, void *d_records, void *stream);
int asdr_tuner_import_channels_device(asdr_tuner_t *t, const int *channels, int n, const void *d_records, void *stream);
size_t asdr_tuner_bank_state_bytes(const asdr_tuner_t *t);   /* of the blob an export would write now; 0 for a NULL bank */
/* Synchronises with the bank's work and writes the blob; fails when capacity is short.  Returns 0 / -1. */
int asdr_tuner_export_bank_state(asdr_tuner_t *t, void *host, size_t capacity);
int asdr_tuner_import_bank_state(asdr_tuner_t *t, const void *host, size_t bytes);
/* A new bank of the blob's kind and geometry with n_channels channels on `device` (or ASDR_NO_DEVICE), then the import. */
asdr_tuner_t *asdr_tuner_create_from_bank_state(const void *host, size_t bytes, int n_channels, int device);

int asdr_tuner_synchronize(asdr_tuner_t *t);
float asdr_tuner_last_kernel_ms(asdr_tuner_t *t);  /* device time of the last update (events around its kernels); -1 if none */

#ifdef __cplusplus
}
#endif
#endif /* ASDR_TUNER_H_ */
