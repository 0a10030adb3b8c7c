/* asdr_tuner_state.h -- launch arguments shared by asdr_tuner_state.hip (kernels) and asdr_tuner_host.cpp (C ABI) of the tuner
 * bank's channel records (include/asdr_tuner.h, "State records"). */
#ifndef ASDR_TUNER_STATE_H_
#define ASDR_TUNER_STATE_H_

#include "asdr_tuner_device.h"

typedef struct {
  int32_t *carry;   /* [n_channels][576]: the bank's current carry rows (d_carry[ccur]); NULL: no carry moves (see the kernels) */
  double *level;    /* [n_channels]: the level accumulators; NULL when the levels are off */
} TunerStateArgs;

#ifdef __cplusplus
extern "C" {
#endif
/* list: NULL, or [n] (channel, record index) pairs in device memory; NULL: entry e is channel ch0 + e, record rec0 + e.
 * head (gather): [n][256] bytes in device memory, the head of entry e as the host filled it. */
int asdr_launch_tuner_state_gather(const TunerStateArgs *a, const int *list, int n, int ch0, int rec0, void *records, const void *head,
                                   void *stream);
int asdr_launch_tuner_state_scatter(const TunerStateArgs *a, const int *list, int n, int ch0, int rec0, const void *records, void *stream);
#ifdef __cplusplus
}
#endif

#endif /* ASDR_TUNER_STATE_H_ */
