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

#ifdef __cplusplus
extern "C" {
#endif
/* the filter step (every channel x 128-output block) followed by the history step, in order on `stream` */
int asdr_launch_tuner(const TunerArgs *a, void *stream);
#ifdef __cplusplus
}
#endif

#endif /* ASDR_TUNER_DEVICE_H_ */
