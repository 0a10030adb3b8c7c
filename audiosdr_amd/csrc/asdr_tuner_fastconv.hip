// asdr_tuner_fastconv.hip -- stage 1 of a fast-convolution bank (include/asdr_tuner.h, "Fast-convolution banks"): one forward
// FFT per source and frame, shared by all of its channels, then per channel 256 bins weighted by G, a 256-point inverse FFT, the
// coarse sign and the fine NCO.  Kept apart from asdr_tuner.hip and asdr_tuner_resample.hip, whose kernels it leaves untouched;
// stage 2 is asdr_tuner_resample_kernel, unchanged.
//
// Form:
//  * forward: Stockham radix-4 passes (radix 2 last for odd log2 n) in one workgroup's LDS, twiddles from the host's float64-built
//    W_N table.  N <= 4096 is one transform per workgroup; above, four-step N = N1 N2: column FFTs of N1 points read straight from
//    the int16 window, times W_N^{n2 k1}, into the scratch; then row FFTs of N2 points into X in natural bin order.  All sources x
//    frames of a call go in one launch per pass.
//  * channel (the hot path): one wave per (channel, frame).  The first radix-4 pass takes its 4 points per lane straight from the
//    gather (X[(k0 + m) mod N] G[m], 64 consecutive bins per load); the last pass leaves y[t + 64 q] in lane t's registers, so only
//    q = 2, 3 (n = 128 .. 255, the samples overlap-save keeps) are formed.  Coarse sign, fine NCO (sincospif of (int32) theta
//    / 2^31), round-half-even and sat16 follow, and the int16 samples go to the caller's rows or the stage-2 intermediate.
//  * history: the call's last H samples per source into the other history buffer.
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"

namespace {

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// 4-point DFT with sign -1 (forward) or +1 (inverse): y_q = sum_r u_r e^{sign j 2 pi q r / 4}
template <int SIGN>
__device__ inline void dft4(float2 u0, float2 u1, float2 u2, float2 u3, float2 &y0, float2 &y1, float2 &y2, float2 &y3) {
  const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
  const float2 v3 = SIGN < 0 ? make_float2(d.y, -d.x) : make_float2(-d.y, d.x);   // d * (SIGN j)
  y0 = cadd(v0, v2); y1 = cadd(v1, v3); y2 = csub(v0, v2); y3 = csub(v1, v3);
}

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// Forward FFT of n = 2^log2n <= 4096 points in buf (LDS), in place, by ASDR_TUNER_FC_LANES lanes.  Stockham: the pass with
// sub-transform length p and radix r maps lane item i < n / r, k = i mod p, to inputs i + q n / r times e^{-j 2 pi q k / (r p)}
// and outputs (i - k) r + k + q p.  tw = W_M with M = 2^log2m >= n.  Enters and leaves with the workgroup synchronised.
__device__ void lds_fft(float2 *buf, int log2n, const float2 *tw, int log2m) {
  const int n = 1 << log2n, t = threadIdx.x;
  int lp = 0;
  for (; lp + 2 <= log2n; lp += 2) {
    const int p = 1 << lp, nq = n >> 2, sh = log2m - lp - 2;
    float2 v[4][4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int i = t + s * ASDR_TUNER_FC_LANES;
      if (i < nq)
#pragma unroll
        for (int q = 0; q < 4; q++) v[s][q] = buf[i + q * nq];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const int i = t + s * ASDR_TUNER_FC_LANES;
      if (i < nq) {
        const int k = i & (p - 1), j = ((i - k) << 2) + k;
        float2 y0, y1, y2, y3;
        dft4<-1>(v[s][0], cmul(v[s][1], tw[k << sh]), cmul(v[s][2], tw[(2 * k) << sh]), cmul(v[s][3], tw[(3 * k) << sh]), y0, y1, y2, y3);
        buf[j] = y0; buf[j + p] = y1; buf[j + 2 * p] = y2; buf[j + 3 * p] = y3;
      }
    }
    __syncthreads();
  }
  if (lp < log2n) {   // radix 2 with p = n / 2: item i reads and writes i and i + n / 2 only
    const int h = n >> 1, sh = log2m - log2n;
    for (int i = t; i < h; i += ASDR_TUNER_FC_LANES) {
      const float2 u0 = buf[i], u1 = cmul(buf[i + h], tw[i << sh]);
      buf[i] = cadd(u0, u1); buf[i + h] = csub(u0, u1);
    }
    __syncthreads();
  }
}

}  // namespace

__global__ __launch_bounds__(ASDR_TUNER_FC_LANES) void asdr_tuner_fc_forward_kernel(FcForwardArgs a) {
  __shared__ float2 buf[ASDR_TUNER_FC_LDS_MAX];
  const int t = threadIdx.x, unit = blockIdx.x, f = blockIdx.y, s = blockIdx.z;
  const int H = a.hop, n1 = 1 << a.log2n1;
  const float2 *tw = (const float2 *)a.tw;
  const size_t xoff = ((size_t)s * a.n_frames + f) << a.log2n;
  const int log2m = a.pass == 0 ? a.log2n : (a.pass == 1 ? a.log2n1 : a.log2n2);
  const int m = 1 << log2m;
  if (a.pass != 2) {   // window sample w = e (whole) or e N2 + n2 (column n2 = unit): input (f - 1) H + w of the call
    const int stride = a.pass == 0 ? 1 : 1 << a.log2n2, off = a.pass == 0 ? 0 : unit;
    const int32_t *row = a.in + (size_t)s * a.in_stride;
    const int32_t *hrow = a.hist_rd + (size_t)s * H;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) {
      const int64_t mm = (int64_t)(f - 1) * H + (int64_t)e * stride + off;
      const int32_t word = mm >= 0 ? row[mm] : hrow[H + mm];
      buf[e] = make_float2((float)(int16_t)(word & 0xffff), (float)(word >> 16));
    }
  } else {             // row k1 = unit: T[n2 N1 + k1]
    const float2 *src = (const float2 *)a.scratch + xoff;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) buf[e] = src[((size_t)e << a.log2n1) + unit];
  }
  __syncthreads();
  lds_fft(buf, log2m, tw, a.log2n);
  float2 *x = (float2 *)a.x + xoff;
  if (a.pass == 0) {
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) x[e] = buf[e];
  } else if (a.pass == 1) {   // T[n2 N1 + k1] = W_N^{n2 k1} (column FFT)[k1]; n2 k1 < N
    float2 *dst = (float2 *)a.scratch + xoff + (size_t)unit * n1;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) dst[e] = cmul(buf[e], tw[unit * e]);
  } else {                    // X[k1 + N1 k2]
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) x[unit + ((size_t)e << a.log2n1)] = buf[e];
  }
}

__global__ __launch_bounds__(ASDR_TUNER_FC_CH_LANES) void asdr_tuner_fc_channel_kernel(FcChannelArgs a) {
  __shared__ float2 buf[256];
  const int t = threadIdx.x;
  const int c = a.order[blockIdx.x], f = blockIdx.y;
  const asdr_tuner_state_t st = a.chan[c];
  const int lq = 32 - a.log2n, N = 1 << a.log2n;
  const int k0 = (int)(((int64_t)(int32_t)st.fw + (1LL << (lq - 1))) >> lq);   // floor(((int32) fw + q / 2) / q)
  const uint32_t rw = st.fw - ((uint32_t)k0 << lq);
  const float2 *X = (const float2 *)a.x + (((size_t)st.src * a.n_frames + f) << a.log2n);
  const float2 *G = (const float2 *)a.g, *tw = (const float2 *)a.tw256;

  // pass p = 1: lane t takes m' = t + 64 q (m = m' or m' - 256), no twiddle
  float2 u[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int mp = t + 64 * q, mm = mp < 128 ? mp : mp - 256;
    u[q] = cmul(X[(k0 + mm) & (N - 1)], G[mp]);
  }
  float2 y0, y1, y2, y3;
  dft4<1>(u[0], u[1], u[2], u[3], y0, y1, y2, y3);
  buf[4 * t] = y0; buf[4 * t + 1] = y1; buf[4 * t + 2] = y2; buf[4 * t + 3] = y3;
  __syncthreads();
  // passes p = 4, 16: inputs t + 64 q times e^{+j 2 pi q k / (4 p)} = conj(W_256^{q k 64 / p})
#pragma unroll
  for (int lp = 2; lp <= 4; lp += 2) {
    const int p = 1 << lp, k = t & (p - 1), j = ((t - k) << 2) + k, sh = 6 - lp;
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = buf[t + 64 * q];
    __syncthreads();
    dft4<1>(u[0], cmulc(u[1], tw[k << sh]), cmulc(u[2], tw[(2 * k) << sh]), cmulc(u[3], tw[(3 * k) << sh]), y0, y1, y2, y3);
    buf[j] = y0; buf[j + p] = y1; buf[j + 2 * p] = y2; buf[j + 3 * p] = y3;
    __syncthreads();
  }
  // pass p = 64: k = t, outputs y[t + 64 q]; keep q = 2, 3 (n = 128 + t, 192 + t)
#pragma unroll
  for (int q = 0; q < 4; q++) u[q] = buf[t + 64 * q];
  {
    const float2 u1 = cmulc(u[1], tw[t]), u2 = cmulc(u[2], tw[2 * t]), u3 = cmulc(u[3], tw[3 * t]);
    const float2 v0 = cadd(u[0], u2), v1 = csub(u[0], u2), v2 = cadd(u1, u3), d = csub(u1, u3);
    const float2 v3 = make_float2(-d.y, d.x);
    y2 = csub(v0, v2); y3 = csub(v1, v3);
  }

  const int64_t b = a.pos / a.hop + f;                       // the bank's frame index
  const float scale = ldexpf((((int)k0 & 1) && ((b - 1) & 1)) ? -1.0f : 1.0f, -a.log2n);   // 1 / N and (-1)^{k0 (b - 1)}
  const uint32_t th0 = st.ph_a + rw * (uint32_t)(b * a.hop - st.pos_a);
  int16_t *oi = a.out_i + (int64_t)c * a.out_stride + (int64_t)f * 128;
  int16_t *oq = a.out_q + (int64_t)c * a.out_stride + (int64_t)f * 128;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int n = t + 64 * h;                                // i = 128 b + n
    const float2 y = h ? y3 : y2;
    const uint32_t th = th0 + rw * (uint32_t)(n * a.decimation);
    float sn, cs;
    sincospif((float)(int32_t)th * 4.656612873077393e-10f, &sn, &cs);   // (int32) theta / 2^31 half turns
    const float re = (y.x * cs + y.y * sn) * scale, im = (y.y * cs - y.x * sn) * scale;
    oi[n] = (int16_t)sat16(__float2int_rn(fminf(fmaxf(re, -40000.0f), 40000.0f)));
    oq[n] = (int16_t)sat16(__float2int_rn(fminf(fmaxf(im, -40000.0f), 40000.0f)));
  }
}

// history: slot j of source s after the call = the call's sample (n_frames - 1) H + j
__global__ __launch_bounds__(256) void asdr_tuner_fc_history_kernel(FcForwardArgs a) {
  const int s = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.hop) return;
  a.hist_wr[(size_t)s * a.hop + j] = a.in[(size_t)s * a.in_stride + (int64_t)(a.n_frames - 1) * a.hop + j];
}

extern "C" int asdr_launch_tuner_fastconv(const FcForwardArgs *f, const FcChannelArgs *c, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (f->pass == 0) {
    hipLaunchKernelGGL(asdr_tuner_fc_forward_kernel, dim3(1, f->n_frames, f->n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, *f);
  } else {
    FcForwardArgs p = *f;
    p.pass = 1;
    hipLaunchKernelGGL(asdr_tuner_fc_forward_kernel, dim3(1 << p.log2n2, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return -1;
    p.pass = 2;
    hipLaunchKernelGGL(asdr_tuner_fc_forward_kernel, dim3(1 << p.log2n1, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
  }
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(asdr_tuner_fc_channel_kernel, dim3(c->n_channels, c->n_frames), dim3(ASDR_TUNER_FC_CH_LANES), 0, stream, *c);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(asdr_tuner_fc_history_kernel, dim3((f->hop + 255) / 256, f->n_sources), dim3(256), 0, stream, *f);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
