/* asdr_tuner_device.h -- launch arguments shared by asdr_tuner.hip (kernels) and asdr_tuner_host.cpp (C ABI) of the digital
 * tuner bank (include/asdr_tuner.h). */
#ifndef ASDR_TUNER_DEVICE_H_
#define ASDR_TUNER_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_tuner.h"

#define ASDR_TUNER_HIST_SLOTS 1024   /* per-source history row: slot j holds sample P - 1024 + j (slot 0 is never read) */

typedef struct {
  const int32_t *in;                /* [n_sources][in_stride] CS16 words (re low, im high) */
  const int32_t *hist_rd;           /* [n_sources][1024]: the samples before P (read by the mixer) */
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
  const int32_t *in;                /* [n_sources][in_stride] CS16 words (re low, im high) */
  const int32_t *hist_rd;           /* [n_sources][H]: samples P - H .. P - 1 */
  int32_t *hist_wr;                 /* [n_sources][H]: samples P + n_frames H - H .. (written by the history step) */
  const float *tw;                  /* [N]: W_N^j = e^{-j 2 pi j / N}; then [256]: W_256^j */
  float *scratch, *x;               /* [n_sources][n_frames][N] each */
  int64_t in_stride;                /* complex samples */
  int32_t n_sources, n_frames, hop; /* H */
  int32_t log2n, log2n1, log2n2;    /* N = N1 N2 for the four-step passes (N > 4096) */
  int32_t pass;                     /* 0: the whole transform; 1: four-step columns (N1 points); 2: four-step rows (N2 points) */
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

#ifdef __cplusplus
extern "C" {
#endif
/* a fast-convolution stage 1: the forward step(s), the channel step, then the history step, in order on `stream` */
int asdr_launch_tuner_fastconv(const FcForwardArgs *f, const FcChannelArgs *c, void *stream);
/* the stage-2 step: every channel x 512-output tile (at least one tile: the carry is written even when no block is) */
int asdr_launch_tuner_resample(const ResampleArgs *a, void *stream);
/* the filter step (every channel x 128-output block) followed by the history step, in order on `stream` */
int asdr_launch_tuner(const TunerArgs *a, void *stream);
#ifdef __cplusplus
}
#endif

#endif /* ASDR_TUNER_DEVICE_H_ */
