// asdr_spectrogram_device.h -- what asdr_spectrogram_host.cpp and asdr_spectrogram.hip share: the kernels' argument block and
// launch entries.
#ifndef ASDR_SPECTROGRAM_DEVICE_H_
#define ASDR_SPECTROGRAM_DEVICE_H_

#include <stdint.h>

#include "../../include/asdr_spectrogram.h"

#define ASDR_SPECTROGRAM_THREADS 256        // lanes per workgroup of all kernels
#define ASDR_SPECTROGRAM_SMALL_MAX_N 1024   // up to here a wave owns a transform (<= 512 complex points), four to a workgroup
#define ASDR_SPECTROGRAM_SMALL_POINTS 512   // complex points of a small transform's LDS buffer
#define ASDR_SPECTROGRAM_LARGE_POINTS 4096  // complex points of a large transform's LDS buffer: 32 KiB

struct SpectrogramArgs {
  const int16_t *audio;        // [n_channels][stride]
  int64_t stride;              // samples
  const int16_t *carry;        // [n_channels][N]: the last N samples before this call
  int16_t *carry_next;         // the other half of the double buffer
  float *out;                  // [rows][out_stride][B] (x 2 for complex)
  int64_t out_stride;          // frames
  const int32_t *index;        // NULL: row c is channel c
  const int32_t *count;
  const float *window;         // [N]
  const float *tw;             // float2 [N]: W_N^k = e^{-j 2 pi k / N}, built in float64
  int32_t n_channels, n_samples, grid_rows, capacity_rows;
  int32_t log2n, hop, k0, n_bins, complex_out;
  int32_t n_frames;            // frames of this call per row
  int32_t first;               // the call's first frame begins at sample `first` of the call: -N < first <= 0
  float scale;                 // 1 / N
};

// the transform pass over grid_rows rows x n_frames frames
extern "C" int asdr_launch_spectrogram(const SpectrogramArgs *a, void *stream);
// every channel's new carry into carry_next
extern "C" int asdr_launch_spectrogram_carry(const SpectrogramArgs *a, void *stream);

#endif
