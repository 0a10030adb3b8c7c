// asdr_tuner_resample.hip -- stage 2 of a rate bank (include/asdr_tuner.h): the polyphase rational resampler U / M that takes each
// channel's stage-1 sequence u at Fs_mid to 44.1 kHz.  Kept apart from asdr_tuner.hip, whose stage-1 kernels it leaves untouched.
//
// Form: one workgroup of 256 lanes = one channel x one tile of up to 512 outputs.  The tile's u window (carried
// history + this call's intermediate row), I and Q packed in one dword, is staged in LDS; lane o finds b_j and phi_j from the
// tile's (b, r) and a host table of (o M / U, o M % U) -- one compare, no division per lane -- reads its phase's K taps from the
// [U][KP] table with 16-byte loads (the table, at most 256 KB, stays in L2) and accumulates both components in int32.  Tile 0 of
// each channel also writes the channel's new carry into the other carry buffer, so no launch reads what it overwrites.
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"

namespace {

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// u at window index w (I low, Q high)
__device__ inline int32_t window_word(const ResampleArgs &a, int c, int w) {
  if (w < ASDR_TUNER_CARRY) return a.carry_rd[(size_t)c * ASDR_TUNER_CARRY + w];
  const size_t m = (size_t)c * a.n_frames * 128 + (w - ASDR_TUNER_CARRY);
  return (int32_t)(uint16_t)a.mid_i[m] | ((int32_t)a.mid_q[m] << 16);
}

}  // namespace

__global__ __launch_bounds__(ASDR_TUNER_RS_LANES) void asdr_tuner_resample_kernel(ResampleArgs a) {
  __shared__ int32_t win[ASDR_TUNER_RS_WIN];
  const int t = threadIdx.x, c = blockIdx.x, tile = blockIdx.y;
  const int U = a.up, K = a.k;

  if (tile == 0)   // new carry: slot i = u sample N_u + 128 n_frames - 576 + i = window index 128 n_frames + i
    for (int i = t; i < ASDR_TUNER_CARRY; i += ASDR_TUNER_RS_LANES)
      a.carry_wr[(size_t)c * ASDR_TUNER_CARRY + i] = window_word(a, c, a.n_frames * 128 + i);

  const int o0 = tile * ASDR_TUNER_RS_OUT;
  const int n = min(ASDR_TUNER_RS_OUT, a.n_out - o0);
  if (n <= 0) return;
  // the tile's first output: b (window index) and remainder, from the call's (q0, r0) and the per-tile step (wave-uniform)
  const int rt0 = a.r0 + tile * a.tile_r;
  const int bt = a.q0 + tile * a.tile_q + rt0 / U, rt = rt0 % U;
  const int last_qr = a.lane_qr[n - 1];
  const int b_last = bt + (last_qr >> 11) + ((rt + (last_qr & 2047)) >= U ? 1 : 0);
  const int lo = bt - (K - 1);            // >= 4: the carry reaches 572 samples back (asdr_tuner_device.h)
  const int span = b_last - lo + 1;       // <= 2109
  for (int i = t; i < span; i += ASDR_TUNER_RS_LANES) win[i] = window_word(a, c, lo + i);
  __syncthreads();

  for (int o = t; o < n; o += ASDR_TUNER_RS_LANES) {
    const int qr = a.lane_qr[o];
    int r = rt + (qr & 2047), b = bt + (qr >> 11);
    if (r >= U) { r -= U; b++; }
    const uint4 *hp = (const uint4 *)(a.taps + (size_t)r * a.kp);
    const int32_t *u = win + (b - lo);    // u[-k] = window index b - k
    int acc_i = 0, acc_q = 0;
    for (int k8 = 0; k8 < K; k8 += 8) {
      const uint4 h4 = hp[k8 >> 3];
      const uint32_t hw[4] = {h4.x, h4.y, h4.z, h4.w};
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const int k = k8 + e;
        if (k < K) {                        // taps past K are zero, but u[-k] may lie before the window
          const int h = (int16_t)(hw[e >> 1] >> (16 * (e & 1)));
          const int32_t z = u[-k];
          acc_i += h * (int)(int16_t)(z & 0xffff);   // |sum| <= 65535 * 32768 < 2^31: exact in int32
          acc_q += h * (z >> 16);
        }
      }
    }
    const int64_t d = (int64_t)c * a.out_stride + o0 + o;
    a.out_i[d] = (int16_t)sat16((acc_i + a.round) >> a.shift);
    a.out_q[d] = (int16_t)sat16((acc_q + a.round) >> a.shift);
  }
}

extern "C" int asdr_launch_tuner_resample(const ResampleArgs *a, void *stream) {
  const int tiles = a->n_out > 0 ? (a->n_out + ASDR_TUNER_RS_OUT - 1) / ASDR_TUNER_RS_OUT : 1;
  hipLaunchKernelGGL(asdr_tuner_resample_kernel, dim3(a->n_channels, tiles), dim3(ASDR_TUNER_RS_LANES), 0, (hipStream_t)stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
