/* asdr_tuner_device.h -- launch arguments shared by asdr_tuner.hip (kernels) and asdr_tuner_host.cpp (C ABI) of the digital
 * tuner bank (include/asdr_tuner.h). */
#ifndef ASDR_TUNER_DEVICE_H_
#define ASDR_TUNER_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_tuner.h"

#define ASDR_TUNER_HIST_SLOTS 1024   /* per-source history row: slot j holds sample P - 1024 + j (slot 0 is never read) */

/* Bytes of one stored sample of an input format (include/asdr_tuner.h, "Input formats"). */
#define ASDR_TUNER_FMT_BYTES(f) ((f) == ASDR_TUNER_IN_CS16 ? 4 : (f) == ASDR_TUNER_IN_CF32 ? 8 : 2)

typedef struct {
  const int32_t *in;                /* [n_sources][in_stride] samples of format fmt (CS16: words, re low, im high) */
  const int32_t *hist_rd;           /* [n_sources][1024]: the samples before P (read by the mixer), converted: CS16 words */
  int32_t *hist_wr;                 /* [n_sources][1024]: the samples before P + N (written by the history step) */
  const asdr_tuner_state_t *chan;   /* [n_channels] */
  const int32_t *order;             /* [n_channels]: channels sorted by source (grid x follows it) */
  const int32_t *taps;              /* [A][DP2]: polyphase tap pairs, see asdr_tuner.hip */
  int16_t *out_i, *out_q;           /* [n_channels][out_stride] */
  int64_t pos;                      /* P before this call */
  int64_t in_stride, out_stride;    /* complex samples / output samples */
  int32_t n_channels, n_sources, n_blocks, decimation;
  int32_t n_phase_rows;             /* A = ceil(L / D) */
  int32_t n_phase_pairs;            /* DP2 = ceil(D / 2) */
  int32_t shift, round;             /* s = 15 - g, r = s ? 1 << (s - 1) : 0 */
  int32_t fmt;                      /* ASDR_TUNER_IN_*: picks the kernels' instantiation (the CS16 kernels do not read it) */
} TunerArgs;

/* Stage 2 of a rate bank (asdr_tuner_resample.hip).  Window coordinates: w = 0 is u sample N_u - ASDR_TUNER_CARRY (N_u before the
 * call); w < ASDR_TUNER_CARRY comes from the carry row, the rest from the call's intermediate rows. */
#define ASDR_TUNER_CARRY 576          /* u samples per channel carried across calls: >= K - 1 + ceil(127 M / U) + 1 = 572 */
#define ASDR_TUNER_RS_LANES 256
#define ASDR_TUNER_RS_OUT 512         /* outputs per workgroup (4 blocks); its u window is at most 511 * 4 + 1 + 63 + 1 samples */
#define ASDR_TUNER_RS_WIN 2112

typedef struct {
  const int16_t *mid_i, *mid_q;     /* [n_channels][n_frames * 128]: stage 1's u for this call */
  const int32_t *carry_rd;          /* [n_channels][576]: u (I low, Q high) before N_u */
  int32_t *carry_wr;                /* [n_channels][576]: u before N_u + 128 n_frames */
  const int16_t *taps;              /* [U][KP]: taps[phi][k] = h2[k U + phi], zero past K */
  const int32_t *lane_qr;           /* [512]: (o M / U) << 11 | (o M % U) for o < 512 */
  int16_t *out_i, *out_q;           /* [n_channels][out_stride] */
  int64_t out_stride;               /* output samples */
  int32_t n_channels, n_frames, n_out;   /* n_out = output samples this call (128 x blocks) */
  int32_t up, down, k, kp;          /* U, M, K, KP = K rounded up to 8 */
  int32_t q0, r0;                   /* b_{j0} - (N_u - 576) and j0 M - b_{j0} U for the call's first output j0 */
  int32_t tile_q, tile_r;           /* 512 M / U and 512 M % U */
  int32_t shift, round;             /* s2, r2 */
} ResampleArgs;

/* Stage 1 of a fast-convolution bank (asdr_tuner_fastconv.hip).  Complex values are float pairs (re, im).  X and the four-step
 * scratch are [n_sources][n_frames][N]; frame f of the call is frame b = P / H + f of the bank. */
#define ASDR_TUNER_FC_LANES 256       /* forward kernel: one workgroup per transform (or four-step column / row) */
#define ASDR_TUNER_FC_LDS_MAX 4096    /* largest transform done in one workgroup's LDS (32 KB) */
#define ASDR_TUNER_FC_CH_LANES 64     /* channel kernel: one wave per (channel, frame), 4 of the 256 points per lane */

typedef struct {
  const int32_t *in;                /* [n_sources][in_stride] samples of format fmt (CS16: words, re low, im high) */
  const int32_t *hist_rd;           /* [n_sources][H]: samples P - H .. P - 1, converted: CS16 words */
  int32_t *hist_wr;                 /* [n_sources][H]: samples P + n_frames H - H .. (written by the history step) */
  const float *tw;                  /* [N]: W_N^j = e^{-j 2 pi j / N}; then [256]: W_256^j */
  float *scratch, *x;               /* [n_sources][n_frames][N] each */
  int64_t in_stride;                /* complex samples */
  int32_t n_sources, n_frames, hop; /* H */
  int32_t log2n, log2n1, log2n2;    /* N = N1 N2 for the four-step passes (N > 4096) */
  int32_t pass;                     /* 0: the whole transform; 1: four-step columns (N1 points); 2: four-step rows (N2 points) */
  int32_t fmt;                      /* ASDR_TUNER_IN_*.  RS16: the transform has N / 2 points (log2n1 + log2n2 = log2n - 1) and the
                                       last pass untangles it into the N bins of X */
} FcForwardArgs;

typedef struct {
  const float *x;                   /* [n_sources][n_frames][N] */
  const float *g;                   /* [256]: G[m] at m' = m mod 256 */
  const float *tw256;               /* [256]: W_256^j */
  const asdr_tuner_state_t *chan;   /* [n_channels] */
  const int32_t *order;             /* [n_channels]: channels sorted by (source, k0) (grid x follows it) */
  int16_t *out_i, *out_q;           /* [n_channels][out_stride] */
  int64_t pos;                      /* P before this call (a frame boundary) */
  int64_t out_stride;               /* output samples */
  int32_t n_channels, n_frames, hop, log2n, decimation;   /* H, log2 N, R */
} FcChannelArgs;

/* The monitors of a fast-convolution bank (asdr_tuner_monitor.hip; include/asdr_tuner.h, "Monitors"). */
#define ASDR_TUNER_MON_LANES 256      /* spectrum kernel: four independent waves, each owning max(128, g) consecutive bins of X */

typedef struct {
  const float *x;                   /* [n_sources][n_frames][N]: the call's X */
  double *acc;                      /* [n_sources][B] */
  int32_t n_sources, n_frames, log2n, log2b;   /* log2 N, log2 B */
  int32_t window, mode;             /* ASDR_TUNER_WIN_*, ASDR_TUNER_MON_* */
} FcSpectrumArgs;

typedef struct {
  float *part;                      /* [n_frames][n_channels]: e_b[c] of the call's frames (float; channel order) */
  double *acc;                      /* [n_channels] */
} FcLevelArgs;

/* The palette of a fast-convolution bank (asdr_tuner_palette.hip; include/asdr_tuner.h, "Filter palette and gain"). */
typedef struct {
  const float *tab;                 /* [ASDR_TUNER_FC_MAX_FILTERS][256]: G_s[m] at m' = m mod 256 (rows of undefined slots are never read) */
  const int32_t *slot;              /* [n_channels]: f_c, channel order */
  const float *gain;                /* [n_channels]: a_c */
} FcPaletteArgs;

/* Source conditioning (asdr_tuner_condition.hip; include/asdr_tuner.h, "Source conditioning"): the pre-pass over the call's rows. */
#define ASDR_TUNER_COND_LANES 256     /* a lane takes 16 bytes of output (or of input, whichever is more) per step */
#define ASDR_TUNER_COND_MAX_BLOCKS 2048   /* grid cap (x times y); a workgroup strides over the rest of its row */
#define ASDR_TUNER_IQ_STATS_WORDS 7   /* asdr_tuner_iq_stats_t: n, sum_re, sum_im, sum_re2, sum_im2, sum_reim, clipped */

typedef struct {
  const void *in;                   /* [n_sources][in_stride] samples of format fmt: the caller's rows */
  void *out;                        /* [n_sources][out_stride]: x' as CS16 words (RS16: int16); NULL = the rows are only read */
  const int32_t *corr;              /* [n_sources][4]: d_r, d_i, p, g (read only when out is given) */
  unsigned long long *stats;        /* [n_sources][7]: the int64 sums of asdr_tuner_iq_stats_t, two's complement; NULL = off */
  int64_t in_stride, out_stride;    /* samples */
  int64_t n_samples;                /* per row: a multiple of 128 */
  int32_t n_sources;
  int32_t fmt;                      /* ASDR_TUNER_IN_* of the caller's rows */
  int32_t aligned;                  /* every row of `in` starts 16-byte aligned (always so but for CS16 rows through the int16 entry
                                       points, whose stride is any number of samples) */
} ConditionArgs;

#ifdef __HIP__
/* The formats' loads (include/asdr_tuner.h, "Input formats"): sample m >= 0 of a row as the CS16 word of x (xr low, xi high).
 * Rows start 16-byte aligned, so the 2-byte formats are read as aligned dwords (two samples) and never as bytes or shorts. */
__device__ inline int32_t asdr_cvt_cs8(uint32_t h) { return (int32_t)(((h & 0xffu) << 8) | ((h & 0xff00u) << 16)); }     /* 256 a */
__device__ inline int32_t asdr_cvt_cu8(uint32_t h) { return asdr_cvt_cs8(h ^ 0x8080u) | 0x00800080; }   /* 256 (a - 128) + 128 */
__device__ inline int32_t asdr_cvt_f32(float a) {                       /* sat16(rint(32768 a)), NaN -> 0 */
  const float v = fminf(fmaxf(a * 32768.0f, -32768.0f), 32767.0f);
  return a != a ? 0 : (int32_t)rintf(v);
}
template <int F>
__device__ inline int32_t asdr_half_to_word(uint32_t h) {               /* h: the 16 stored bits of a 2-byte sample */
  return F == ASDR_TUNER_IN_CU8 ? asdr_cvt_cu8(h) : F == ASDR_TUNER_IN_CS8 ? asdr_cvt_cs8(h) : (int32_t)h;   /* RS16: xi = 0 */
}
template <int F>
__device__ inline int32_t asdr_fetch(const void *row, int64_t m) {
  if constexpr (F == ASDR_TUNER_IN_CS16) {
    return ((const int32_t *)row)[m];
  } else if constexpr (F == ASDR_TUNER_IN_CF32) {
    const float2 v = ((const float2 *)row)[m];
    return (asdr_cvt_f32(v.x) & 0xffff) | (int32_t)((uint32_t)asdr_cvt_f32(v.y) << 16);
  } else {
    const uint32_t d = ((const uint32_t *)row)[m >> 1];
    return asdr_half_to_word<F>((m & 1) ? d >> 16 : d & 0xffffu);
  }
}
/* samples m (even) and m + 1 in one load: a dword for the 2-byte formats, 8 bytes for CS16, 16 for CF32 */
template <int F>
__device__ inline void asdr_fetch2(const void *row, int64_t m, int32_t &w0, int32_t &w1) {
  if constexpr (ASDR_TUNER_FMT_BYTES(F) == 2) {
    const uint32_t d = ((const uint32_t *)row)[m >> 1];
    w0 = asdr_half_to_word<F>(d & 0xffffu); w1 = asdr_half_to_word<F>(d >> 16);
  } else if constexpr (F == ASDR_TUNER_IN_CF32) {
    const float4 v = ((const float4 *)row)[m >> 1];
    w0 = (asdr_cvt_f32(v.x) & 0xffff) | (int32_t)((uint32_t)asdr_cvt_f32(v.y) << 16);
    w1 = (asdr_cvt_f32(v.z) & 0xffff) | (int32_t)((uint32_t)asdr_cvt_f32(v.w) << 16);
  } else {
    const int2 v = ((const int2 *)row)[m >> 1];
    w0 = v.x; w1 = v.y;
  }
}
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* a fast-convolution stage 1: the forward step(s), the channel step, then the history step, in order on `stream`.  sp / lv: the
 * monitors' arguments, NULL when off: with lv the channel step is asdr_launch_tuner_channel_levels instead of the plain channel
 * kernel, with sp asdr_launch_tuner_spectrum runs between the channel step and the history step. */
int asdr_launch_tuner_fastconv(const FcForwardArgs *f, const FcChannelArgs *c, const FcSpectrumArgs *sp, const FcLevelArgs *lv,
                               void *stream);
/* the same with asdr_launch_tuner_channel_palette as the channel step (with or without lv): a bank with a channel off slot 0 or
 * gain 1 */
int asdr_launch_tuner_fastconv_palette(const FcForwardArgs *f, const FcChannelArgs *c, const FcSpectrumArgs *sp, const FcLevelArgs *lv,
                                       const FcPaletteArgs *pal, void *stream);
/* asdr_tuner_palette.hip: the channel step with G from row f_c of the table and a_c in the scale; with lv, the level epilogue and
 * asdr_launch_tuner_level_fold */
int asdr_launch_tuner_channel_palette(const FcChannelArgs *c, const FcPaletteArgs *pal, const FcLevelArgs *lv, void *stream);
/* asdr_tuner_monitor.hip: every source x span of bins of X into the spectrum accumulators; the channel step with the level
 * epilogue, then the fold of the call's partials into the level accumulators */
int asdr_launch_tuner_spectrum(const FcSpectrumArgs *sp, void *stream);
int asdr_launch_tuner_channel_levels(const FcChannelArgs *c, const FcLevelArgs *lv, void *stream);
/* the fold alone: the call's partials [n_frames][n_channels] into the level accumulators */
int asdr_launch_tuner_level_fold(const FcLevelArgs *lv, int n_channels, int n_frames, void *stream);
/* asdr_tuner_condition.hip: the pre-pass (out and / or stats given) on `stream` */
int asdr_launch_tuner_condition(const ConditionArgs *a, void *stream);
/* the stage-2 step: every channel x 512-output tile (at least one tile: the carry is written even when no block is) */
int asdr_launch_tuner_resample(const ResampleArgs *a, void *stream);
/* the filter step (every channel x 128-output block) followed by the history step, in order on `stream` */
int asdr_launch_tuner(const TunerArgs *a, void *stream);
#ifdef __cplusplus
}
#endif

#endif /* ASDR_TUNER_DEVICE_H_ */
