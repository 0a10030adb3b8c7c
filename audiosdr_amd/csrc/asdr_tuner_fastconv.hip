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
//  * monitors (asdr_tuner_monitor.hip): when a bank has them on, the launch function below puts that file's
//    level sibling in the channel kernel's place and its spectrum kernel between the channel step and the history step.
//  * palette (asdr_tuner_palette.hip): when a bank has a channel off slot 0 or gain 1, the launch function puts
//    that file's channel step in the place of the channel kernel and of its level sibling.
//  * input formats (include/asdr_tuner.h): asdr_tuner_fc_forward_kernel / _history_kernel are the CS16 bank's, as
//    they were.  asdr_tuner_fc_fmt_forward_kernel<F> / asdr_tuner_fc_fmt_history_kernel<F> convert in the window load (asdr_fetch);
//    a converted value is an integer of at most 16 bits, exact as a float, and everything after the load is the same code.
//    RS16: asdr_tuner_fc_real_forward_kernel transforms z[n] = w[2n] + j w[2n + 1] (N / 2 points; a dword of the row IS z[n]) and
//    untangles, X[k] = (Z[k] + conj Z[N/2 - k]) / 2 - (j / 2) W_N^k (Z[k] - conj Z[N/2 - k]), X[N - k] = conj X[k], into all N
//    bins in natural order: in LDS before the store for N / 2 <= 2048; above, fused into the four-step row pass, whose workgroup
//    takes the rows k1 and M1 - k1 (Z[k] and Z[N/2 - k] lie in them) and stores the four mirror images of each pair.
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

// asdr_tuner_fc_forward_kernel for a complex format F != CS16, passes 0 and 1 (pass 2 reads no input: the CS16 kernel runs it)
template <int F>
__global__ __launch_bounds__(ASDR_TUNER_FC_LANES) void asdr_tuner_fc_fmt_forward_kernel(FcForwardArgs a) {
  __shared__ float2 buf[ASDR_TUNER_FC_LDS_MAX];
  const int t = threadIdx.x, unit = blockIdx.x, f = blockIdx.y, s = blockIdx.z;
  const int H = a.hop, n1 = 1 << a.log2n1;
  const float2 *tw = (const float2 *)a.tw;
  const size_t xoff = ((size_t)s * a.n_frames + f) << a.log2n;
  const int log2m = a.pass == 0 ? a.log2n : a.log2n1;
  const int m = 1 << log2m;
  const char *row = (const char *)a.in + (size_t)s * a.in_stride * ASDR_TUNER_FMT_BYTES(F);
  const int32_t *hrow = a.hist_rd + (size_t)s * H;
  if (a.pass == 0) {   // window samples 2e, 2e + 1 (input (f - 1) H + 2e of the call: even, so both lie on one side of 0)
    for (int e = t; e < m / 2; e += ASDR_TUNER_FC_LANES) {
      const int64_t mm = (int64_t)(f - 1) * H + 2 * e;
      int2 w;
      if (mm >= 0) asdr_fetch2<F>(row, mm, w.x, w.y);
      else w = *(const int2 *)(hrow + H + mm);
      buf[2 * e] = make_float2((float)(int16_t)(w.x & 0xffff), (float)(w.x >> 16));
      buf[2 * e + 1] = make_float2((float)(int16_t)(w.y & 0xffff), (float)(w.y >> 16));
    }
  } else {             // column n2 = unit: window sample e N2 + n2, one per lane and load (an aligned dword for the 2-byte formats)
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) {
      const int64_t mm = (int64_t)(f - 1) * H + ((int64_t)e << a.log2n2) + unit;
      const int32_t word = mm >= 0 ? asdr_fetch<F>(row, mm) : hrow[H + mm];
      buf[e] = make_float2((float)(int16_t)(word & 0xffff), (float)(word >> 16));
    }
  }
  __syncthreads();
  lds_fft(buf, log2m, tw, a.log2n);
  if (a.pass == 0) {
    float2 *x = (float2 *)a.x + xoff;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) x[e] = buf[e];
  } else {
    float2 *dst = (float2 *)a.scratch + xoff + (size_t)unit * n1;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) dst[e] = cmul(buf[e], tw[unit * e]);
  }
}

namespace {
// X[k] from Z[k], Z[N/2 - k] and W_N^k
__device__ inline float2 untangle(float2 zk, float2 zm, float2 w) {
  const float2 e = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));   // (Z[k] + conj Z[M - k]) / 2
  const float2 o = make_float2(0.5f * (zk.x - zm.x), 0.5f * (zk.y + zm.y));   // (Z[k] - conj Z[M - k]) / 2
  const float2 p = cmul(w, o);
  return make_float2(e.x + p.y, e.y - p.x);                                   // e - j p
}
// X[k] and its mirror image X[N - k] (k = 0: X[N/2] = Re Z[0] - Im Z[0] instead, the one bin no k < N/2 mirrors to)
__device__ inline void store_bins(float2 *x, int k, int n, float2 zk, float2 zm, float2 w) {
  const float2 v = untangle(zk, zm, w);
  x[k] = v;
  if (k) x[n - k] = make_float2(v.x, -v.y);
  else x[n >> 1] = make_float2(zk.x - zk.y, 0.0f);
}
}  // namespace

// The forward step of an RS16 bank: M = N / 2 = 2^(log2n - 1) complex points z[n] = w[2n] + j w[2n + 1], M = M1 M2 (log2n1, log2n2)
// for the four-step passes.  pass 0: the whole transform and the untangle in LDS (M <= 2048).  pass 1: column n2 = unit (M1 points),
// times W_M^{n2 k1} = W_N^{2 n2 k1}, into the scratch.  pass 2: rows k1 = unit and M1 - unit (unit = 0 .. M1 / 2) and the untangle.
__global__ __launch_bounds__(ASDR_TUNER_FC_LANES) void asdr_tuner_fc_real_forward_kernel(FcForwardArgs a) {
  __shared__ float2 buf[ASDR_TUNER_FC_LDS_MAX];
  const int t = threadIdx.x, unit = blockIdx.x, f = blockIdx.y, s = blockIdx.z;
  const int H = a.hop, N = 1 << a.log2n, m1 = 1 << a.log2n1, m2 = 1 << a.log2n2;
  const float2 *tw = (const float2 *)a.tw;
  const size_t xoff = ((size_t)s * a.n_frames + f) << a.log2n;
  float2 *x = (float2 *)a.x + xoff;
  if (a.pass != 2) {   // z[n], n = e (whole) or e M2 + n2: real samples (f - 1) H + 2n, + 1 of the call -- one dword of the row
    const int m = a.pass == 0 ? N >> 1 : m1;
    const int stride = a.pass == 0 ? 1 : m2, off = a.pass == 0 ? 0 : unit;
    const int32_t *row = (const int32_t *)((const char *)a.in + (size_t)s * a.in_stride * 2);
    const int32_t *hrow = a.hist_rd + (size_t)s * H;
    for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) {
      const int64_t mm = (int64_t)(f - 1) * H + 2 * ((int64_t)e * stride + off);
      if (mm >= 0) {
        const int32_t word = row[mm >> 1];
        buf[e] = make_float2((float)(int16_t)(word & 0xffff), (float)(word >> 16));
      } else {         // converted words (xr, 0)
        const int2 w = *(const int2 *)(hrow + H + mm);
        buf[e] = make_float2((float)(int16_t)(w.x & 0xffff), (float)(int16_t)(w.y & 0xffff));
      }
    }
    __syncthreads();
    lds_fft(buf, a.pass == 0 ? a.log2n - 1 : a.log2n1, tw, a.log2n);
    if (a.pass == 0) {
      for (int k = t; k < m; k += ASDR_TUNER_FC_LANES) store_bins(x, k, N, buf[k], buf[(m - k) & (m - 1)], tw[k]);
    } else {
      float2 *dst = (float2 *)a.scratch + xoff + (size_t)unit * m1;
      for (int e = t; e < m; e += ASDR_TUNER_FC_LANES) dst[e] = cmul(buf[e], tw[2 * unit * e]);
    }
    return;
  }
  // pass 2: A = row k1 = unit (Z[k1 + M1 k2] at buf[k2]), B = row M1 - k1 (at buf[M2 + k2]); rows 0 and M1 / 2 pair with themselves
  const float2 *src = (const float2 *)a.scratch + xoff;
  const int kb = (m1 - unit) & (m1 - 1);
  const bool self = kb == unit;
  for (int e = t; e < m2; e += ASDR_TUNER_FC_LANES) {
    buf[e] = src[((size_t)e << a.log2n1) + unit];
    if (!self) buf[m2 + e] = src[((size_t)e << a.log2n1) + kb];
  }
  __syncthreads();
  lds_fft(buf, a.log2n2, tw, a.log2n);
  if (!self) lds_fft(buf + m2, a.log2n2, tw, a.log2n);
  // partner of k = k1 + M1 k2 is M - k = (M1 - k1) + M1 (M2 - 1 - k2) for k1 >= 1, and M1 ((M2 - k2) mod M2) for k1 = 0
  const float2 *zb = self ? buf : buf + m2;
  for (int e = t; e < m2; e += ASDR_TUNER_FC_LANES) {
    const int pe = unit == 0 ? (m2 - e) & (m2 - 1) : m2 - 1 - e;
    const int k = unit + (e << a.log2n1);
    store_bins(x, k, N, buf[e], zb[pe], tw[k]);
    if (!self) {
      const int k2 = kb + (e << a.log2n1);
      store_bins(x, k2, N, zb[e], buf[pe], tw[k2]);
    }
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

// history for a bank of format F != CS16: lane = slots 2j, 2j + 1, converted and written as one 8-byte store
template <int F>
__global__ __launch_bounds__(256) void asdr_tuner_fc_fmt_history_kernel(FcForwardArgs a) {
  const int s = blockIdx.y, j = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (j >= a.hop) return;
  const char *row = (const char *)a.in + (size_t)s * a.in_stride * ASDR_TUNER_FMT_BYTES(F);
  int2 w;
  asdr_fetch2<F>(row, (int64_t)(a.n_frames - 1) * a.hop + j, w.x, w.y);
  *(int2 *)(a.hist_wr + (size_t)s * a.hop + j) = w;
}

namespace {
// the forward and history steps of a complex format F != CS16 (the channel step between them is the caller's)
template <int F>
int launch_fmt_forward(const FcForwardArgs *f, hipStream_t stream) {
  if (f->pass == 0) {
    hipLaunchKernelGGL(asdr_tuner_fc_fmt_forward_kernel<F>, dim3(1, f->n_frames, f->n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, *f);
  } else {
    FcForwardArgs p = *f;
    p.pass = 1;
    hipLaunchKernelGGL(asdr_tuner_fc_fmt_forward_kernel<F>, dim3(1 << p.log2n2, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return -1;
    p.pass = 2;
    hipLaunchKernelGGL(asdr_tuner_fc_forward_kernel, dim3(1 << p.log2n1, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
template <int F>
int launch_fmt_history(const FcForwardArgs *f, hipStream_t stream) {
  hipLaunchKernelGGL(asdr_tuner_fc_fmt_history_kernel<F>, dim3((f->hop / 2 + 255) / 256, f->n_sources), dim3(256), 0, stream, *f);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int launch_real_forward(const FcForwardArgs *f, hipStream_t stream) {
  if (f->pass == 0) {
    hipLaunchKernelGGL(asdr_tuner_fc_real_forward_kernel, dim3(1, f->n_frames, f->n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, *f);
  } else {
    FcForwardArgs p = *f;
    p.pass = 1;
    hipLaunchKernelGGL(asdr_tuner_fc_real_forward_kernel, dim3(1 << p.log2n2, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
    if (hipGetLastError() != hipSuccess) return -1;
    p.pass = 2;
    hipLaunchKernelGGL(asdr_tuner_fc_real_forward_kernel, dim3((1 << p.log2n1) / 2 + 1, p.n_frames, p.n_sources), dim3(ASDR_TUNER_FC_LANES), 0, stream, p);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the channel step (with the level epilogue when lv is given), then the spectrum monitor when sp is given: X is read once more
// before the history step, while the channel step's reads still have it in L2 / MALL.  pal: the bank has a palette in use
// (asdr_tuner_palette.hip's channel step, with or without lv)
int launch_channel(const FcChannelArgs *c, const FcSpectrumArgs *sp, const FcLevelArgs *lv, const FcPaletteArgs *pal, hipStream_t stream) {
  if (pal) {
    if (asdr_launch_tuner_channel_palette(c, pal, lv, stream) != 0) return -1;
  } else if (lv) {
    if (asdr_launch_tuner_channel_levels(c, lv, stream) != 0) return -1;
  } else {
    hipLaunchKernelGGL(asdr_tuner_fc_channel_kernel, dim3(c->n_channels, c->n_frames), dim3(ASDR_TUNER_FC_CH_LANES), 0, stream, *c);
    if (hipGetLastError() != hipSuccess) return -1;
  }
  return sp ? asdr_launch_tuner_spectrum(sp, stream) : 0;
}
}  // namespace

extern "C" int asdr_launch_tuner_fastconv(const FcForwardArgs *f, const FcChannelArgs *c, const FcSpectrumArgs *sp,
                                          const FcLevelArgs *lv, void *stream_) {
  return asdr_launch_tuner_fastconv_palette(f, c, sp, lv, nullptr, stream_);
}

extern "C" int asdr_launch_tuner_fastconv_palette(const FcForwardArgs *f, const FcChannelArgs *c, const FcSpectrumArgs *sp,
                                                  const FcLevelArgs *lv, const FcPaletteArgs *pal, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (f->fmt != ASDR_TUNER_IN_CS16) {
    int rc;
    switch (f->fmt) {
      case ASDR_TUNER_IN_CU8: rc = launch_fmt_forward<ASDR_TUNER_IN_CU8>(f, stream); break;
      case ASDR_TUNER_IN_CS8: rc = launch_fmt_forward<ASDR_TUNER_IN_CS8>(f, stream); break;
      case ASDR_TUNER_IN_CF32: rc = launch_fmt_forward<ASDR_TUNER_IN_CF32>(f, stream); break;
      case ASDR_TUNER_IN_RS16: rc = launch_real_forward(f, stream); break;
      default: rc = -1;
    }
    if (rc != 0) return -1;
    if (launch_channel(c, sp, lv, pal, stream) != 0) return -1;
    switch (f->fmt) {
      case ASDR_TUNER_IN_CU8: return launch_fmt_history<ASDR_TUNER_IN_CU8>(f, stream);
      case ASDR_TUNER_IN_CS8: return launch_fmt_history<ASDR_TUNER_IN_CS8>(f, stream);
      case ASDR_TUNER_IN_CF32: return launch_fmt_history<ASDR_TUNER_IN_CF32>(f, stream);
      default: return launch_fmt_history<ASDR_TUNER_IN_RS16>(f, stream);
    }
  }
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
  if (launch_channel(c, sp, lv, pal, stream) != 0) return -1;
  hipLaunchKernelGGL(asdr_tuner_fc_history_kernel, dim3((f->hop + 255) / 256, f->n_sources), dim3(256), 0, stream, *f);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
