// asdr_spectrogram.hip -- the audio spectrogram's kernels (include/asdr_spectrogram.h): the windowed real transforms of every
// written row's new frames, band bins only, and the new carry of every channel.  A deployment that creates no spectrogram launches
// nothing from this file.
//
// Form:
//  * One transform per (row, frame).  The call's frames are numbered row-major, item = row * n_frames + frame, so that a call of
//    two frames per row (a C2 step's audio at H = N / 2) fills its workgroups as well as a call of hundreds.
//  * Half-size real transform: z[m] = w[2m] x[2m] + j w[2m + 1] x[2m + 1], an N / 2-point complex Stockham FFT in LDS (radix-4 passes
//    in registers between the exchanges, radix 2 last for an odd log2; twiddles from the host's float64-built W_N table, no FMA
//    contraction: the house style of asdr_tuner_fastconv.hip), then the split
//        X[k] = (Z[k] + conj Z[N/2 - k]) / 2 - (j / 2) W_N^k (Z[k] - conj Z[N/2 - k])
//    for the B bins of the band only (bin N / 2 is Re Z[0] - Im Z[0]); nothing is computed or stored for the other bins after the
//    last pass.  1 / N is a power of two: it scales the split's result exactly.
//  * Mapping by size: N <= 1024 (<= 512 complex points, <= 8 per lane) is one wave per transform and four transforms per workgroup,
//    16 KiB of LDS; N >= 2048 (up to 4096 points, 16 per lane) is one 256-lane workgroup per transform, 32 KiB.  The four waves of a
//    small workgroup run the same pass sequence (one N per launch), so they share the workgroup's barriers; a wave whose item lies
//    past the call's last one runs on zeros and stores nothing.
//  * Samples: a frame's samples are loaded straight into the transform's buffer (converted, times the window), as aligned dwords
//    where the row's address allows it and as two shorts otherwise (rows are 2-byte aligned, strides may be odd).  A sample at
//    s >= 0 comes from the call's rows, a sample at s < 0 from the record; the values are the same wherever the call boundaries
//    fall, and everything after the load is one instruction sequence per N: splitting a sequence into calls leaves every bit.
//    Overlapping frames of a row are neighbouring items, so their common samples come from L2; the span is not staged a second
//    time in LDS (DESIGN.md 3.13 says why).
//  * Stores: the band row of a frame is B (or 2 B) contiguous floats, written by consecutive lanes.
//  * carry: a lane moves two samples of a channel's new record, read from the old record or from the call's rows, written as one
//    dword to the other half of the double buffer; nothing reads what the same call overwrites.
#include <hip/hip_runtime.h>

#include "asdr_spectrogram_device.h"

namespace {

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// forward 4-point DFT: y_q = sum_r u_r e^{-j 2 pi q r / 4}
__device__ inline void dft4(float2 u0, float2 u1, float2 u2, float2 u3, float2 &y0, float2 &y1, float2 &y2, float2 &y3) {
  const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
  const float2 v3 = make_float2(d.y, -d.x);   // -j d
  y0 = cadd(v0, v2); y1 = cadd(v1, v3); y2 = csub(v0, v2); y3 = csub(v1, v3);
}

// Forward FFT of n = 2^log2n points in buf (LDS), in place, by the LANES lanes t = 0 .. LANES - 1 of one transform; n <= 16 LANES.
// Stockham: the pass with sub-transform length p and radix r maps item i < n / r, k = i mod p, to inputs i + q n / r times
// e^{-j 2 pi q k / (r p)} and outputs (i - k) r + k + q p.  tw = W_M with M = 2^log2m >= 2 n.  The barriers are the workgroup's:
// every wave of the workgroup calls this with the same log2n.  Enters and leaves synchronised.
template <int LANES>
__device__ inline void lds_fft(float2 *buf, int log2n, const float2 *tw, int log2m, int t) {
  constexpr int ITEMS = LANES == 64 ? 2 : 4;   // radix-4 items per lane at the largest n of this mapping
  const int n = 1 << log2n;
  int lp = 0;
  for (; lp + 2 <= log2n; lp += 2) {
    const int p = 1 << lp, nq = n >> 2, sh = log2m - lp - 2;
    float2 v[ITEMS][4];
#pragma unroll
    for (int s = 0; s < ITEMS; s++) {
      const int i = t + s * LANES;
      if (i < nq)
#pragma unroll
        for (int q = 0; q < 4; q++) v[s][q] = buf[i + q * nq];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < ITEMS; s++) {
      const int i = t + s * LANES;
      if (i < nq) {
        const int k = i & (p - 1), j = ((i - k) << 2) + k;
        float2 y0, y1, y2, y3;
        dft4(v[s][0], cmul(v[s][1], tw[k << sh]), cmul(v[s][2], tw[(2 * k) << sh]), cmul(v[s][3], tw[(3 * k) << sh]), y0, y1, y2, y3);
        buf[j] = y0; buf[j + p] = y1; buf[j + 2 * p] = y2; buf[j + 3 * p] = y3;
      }
    }
    __syncthreads();
  }
  if (lp < log2n) {   // radix 2 with p = n / 2: item i reads and writes i and i + n / 2 only
    const int h = n >> 1, sh = log2m - log2n;
    for (int i = t; i < h; i += LANES) {
      const float2 u0 = buf[i], u1 = cmul(buf[i + h], tw[i << sh]);
      buf[i] = cadd(u0, u1); buf[i + h] = csub(u0, u1);
    }
    __syncthreads();
  }
}

// X[k] from Z[k], Z[N/2 - k] and W_N^k
__device__ inline float2 untangle(float2 zk, float2 zm, float2 w) {
  const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));   // (Z[k] + conj Z[M - k]) / 2
  const float2 o = make_float2(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));   // (Z[k] - conj Z[M - k]) / 2
  const float2 p = cmul(w, o);
  return make_float2(e.x + p.y, e.y - p.x);                                   // e - j p
}

// two neighbouring samples from a 2-byte aligned address: one dword where it is 4-byte aligned
__device__ inline void load2(const int16_t *p, int &x0, int &x1) {
  if (((uintptr_t)p & 2u) == 0) {
    const int32_t w = *(const int32_t *)p;
    x0 = (int16_t)(w & 0xffff); x1 = w >> 16;
  } else {
    x0 = p[0]; x1 = p[1];
  }
}

// samples s and s + 1 of the call: row = the channel's new samples, rec = the end of its record (sample -1 is rec[-1])
__device__ inline void fetch2(const int16_t *row, const int16_t *rec, int s, int &x0, int &x1) {
  if (s >= 0) load2(row + s, x0, x1);
  else if (s < -1) load2(rec + s, x0, x1);
  else { x0 = rec[-1]; x1 = row[0]; }
}

}  // namespace

// grid ceil(grid_rows * n_frames / (256 / LANES)).  LANES lanes per transform: 64 (N <= 1024) or 256 (N >= 2048)
template <int LANES>
__global__ __launch_bounds__(ASDR_SPECTROGRAM_THREADS) void asdr_spectrogram_kernel(SpectrogramArgs a) {
  constexpr int PER = ASDR_SPECTROGRAM_THREADS / LANES;
  constexpr int POINTS = LANES == 64 ? ASDR_SPECTROGRAM_SMALL_POINTS : ASDR_SPECTROGRAM_LARGE_POINTS;
  __shared__ float2 lds[PER * POINTS];
  const int t = threadIdx.x & (LANES - 1), slot = threadIdx.x / LANES;
  const int N = 1 << a.log2n, M = N >> 1;
  int rows = a.grid_rows;
  if (a.index) rows = min(rows, min(*a.count, a.capacity_rows));
  const uint32_t item0 = blockIdx.x * (uint32_t)PER, nf = (uint32_t)a.n_frames;
  if ((int)(item0 / nf) >= rows) return;                      // the whole workgroup
  const uint32_t item = item0 + slot;
  const int row = (int)(item / nf), frame = (int)(item - (uint32_t)row * nf);
  const bool active = row < rows;
  const int c = active ? (a.index ? a.index[row] : row) : -1;
  const bool valid = (uint32_t)c < (uint32_t)a.n_channels;    // a row whose index names no channel reads zeros
  float2 *buf = lds + slot * POINTS;
  const float2 *tw = (const float2 *)a.tw, *win = (const float2 *)a.window;

  if (valid) {
    const int16_t *src = a.audio + (int64_t)c * a.stride;
    const int16_t *rec = a.carry + ((int64_t)c + 1) * N;
    const int s0 = a.first + frame * a.hop;                   // > -N; s0 + N <= n_samples
    for (int m = t; m < M; m += LANES) {
      int x0, x1;
      fetch2(src, rec, s0 + 2 * m, x0, x1);
      const float2 w = win[m];
      buf[m] = make_float2(w.x * (float)x0, w.y * (float)x1);
    }
  } else {
    for (int m = t; m < M; m += LANES) buf[m] = make_float2(0.0f, 0.0f);
  }
  __syncthreads();
  lds_fft<LANES>(buf, a.log2n - 1, tw, a.log2n, t);
  if (!active) return;

  const int64_t at = ((int64_t)row * a.out_stride + frame) * a.n_bins;
  if (a.complex_out) {
    float *o = a.out + 2 * at;
    const bool wide = ((uintptr_t)o & 4u) == 0;               // the same for every row and frame: 2 B floats per frame
    for (int j = t; j < a.n_bins; j += LANES) {
      const int k = a.k0 + j;
      float2 v = k == M ? make_float2(buf[0].x - buf[0].y, 0.0f) : untangle(buf[k], buf[(M - k) & (M - 1)], tw[k]);
      v.x *= a.scale; v.y *= a.scale;
      if (wide) ((float2 *)o)[j] = v;
      else { o[2 * j] = v.x; o[2 * j + 1] = v.y; }
    }
  } else {
    float *o = a.out + at;
    for (int j = t; j < a.n_bins; j += LANES) {
      const int k = a.k0 + j;
      float2 v = k == M ? make_float2(buf[0].x - buf[0].y, 0.0f) : untangle(buf[k], buf[(M - k) & (M - 1)], tw[k]);
      v.x *= a.scale; v.y *= a.scale;
      o[j] = v.x * v.x + v.y * v.y;
    }
  }
}

// grid ceil(n_channels * (N / 2) / 256): lane = samples 2p, 2p + 1 of a channel's new record
__global__ __launch_bounds__(ASDR_SPECTROGRAM_THREADS) void asdr_spectrogram_carry_kernel(SpectrogramArgs a) {
  const int64_t w = (int64_t)blockIdx.x * ASDR_SPECTROGRAM_THREADS + threadIdx.x;
  const int N = 1 << a.log2n;
  const int64_t c = w >> (a.log2n - 1);
  const int p = (int)(w & ((N >> 1) - 1));
  if (c >= a.n_channels) return;
  int x0, x1;
  fetch2(a.audio + c * a.stride, a.carry + (c + 1) * N, a.n_samples - N + 2 * p, x0, x1);   // >= 1 - N; the pair ends before n_samples
  ((uint32_t *)a.carry_next)[w] = ((uint32_t)x0 & 0xffffu) | ((uint32_t)x1 << 16);
}

extern "C" int asdr_launch_spectrogram(const SpectrogramArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (a->grid_rows <= 0 || a->n_frames <= 0) return 0;
  const int64_t items = (int64_t)a->grid_rows * a->n_frames;
  if ((1 << a->log2n) <= ASDR_SPECTROGRAM_SMALL_MAX_N) {
    const int per = ASDR_SPECTROGRAM_THREADS / 64;
    hipLaunchKernelGGL(asdr_spectrogram_kernel<64>, dim3((uint32_t)((items + per - 1) / per)), dim3(ASDR_SPECTROGRAM_THREADS), 0, stream, *a);
  } else {
    hipLaunchKernelGGL(asdr_spectrogram_kernel<256>, dim3((uint32_t)items), dim3(ASDR_SPECTROGRAM_THREADS), 0, stream, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_spectrogram_carry(const SpectrogramArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t pairs = (int64_t)a->n_channels << (a->log2n - 1);
  const uint32_t grid = (uint32_t)((pairs + ASDR_SPECTROGRAM_THREADS - 1) / ASDR_SPECTROGRAM_THREADS);
  hipLaunchKernelGGL(asdr_spectrogram_carry_kernel, dim3(grid), dim3(ASDR_SPECTROGRAM_THREADS), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
