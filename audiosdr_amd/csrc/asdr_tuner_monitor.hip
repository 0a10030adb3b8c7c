// asdr_tuner_monitor.hip -- the monitors of a fast-convolution bank (include/asdr_tuner.h, "Monitors"): the wideband power
// spectrum of every source, taken from the X that stage 1 has already computed, and the level of every channel, taken from the
// channel step's unrounded samples.  Both are off by default; a bank that enables neither launches nothing from this file.
//
// Form:
//  * spectrum: a streaming reduction over X [source][frame][N].  A wave owns span = max(128, g) consecutive bins of one source
//    (g = N / B bins per output bin) and walks them in chunks of 128: lane l loads bins 2l, 2l + 1 of the chunk as one 16-byte
//    load, so a wave's load is 1 KB contiguous whatever g is.  The Hann combine W[k] = X[k] / 2 - (X[k-1] + X[k+1]) / 4 takes its
//    neighbours from the adjacent lanes (ds_bpermute); only lanes 0 and 63 load one more bin (mod N: the bin 0 / bin N - 1 seam).
//    |W|^2 / N^2 and the sum over a group are float32 (quad and row DPP steps, then ds_bpermute across rows); the call's frames
//    are then added (or maximised) in a float64 register and the owner lane does the one float64 read-modify-write per output
//    bin.  Every (source, output bin) has exactly one owner: no atomics.
//  * level: asdr_tuner_fc_channel_level_kernel is asdr_tuner_fc_channel_kernel (asdr_tuner_fastconv.hip) with one more epilogue:
//    the same statements in the same order up to the int16 stores (the build has no FMA contraction, so the outputs are bit
//    for bit the plain kernel's), then |y2|^2 + |y3|^2 per lane, a 64-lane reduction (DPP in the rows, v_readlane across them)
//    and one float per (frame, channel) to a scratch row.  asdr_tuner_fc_level_fold_kernel adds a call's partials to the float64
//    accumulators in frame order.
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"

namespace {

// the complex helpers of asdr_tuner_fastconv.hip, which keeps them file-local
__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)
__device__ inline float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int SIGN>
__device__ inline void dft4(float2 u0, float2 u1, float2 u2, float2 u3, float2 &y0, float2 &y1, float2 &y2, float2 &y3) {
  const float2 v0 = cadd(u0, u2), v1 = csub(u0, u2), v2 = cadd(u1, u3), d = csub(u1, u3);
  const float2 v3 = SIGN < 0 ? make_float2(d.y, -d.x) : make_float2(-d.y, d.x);   // d * (SIGN j)
  y0 = cadd(v0, v2); y1 = cadd(v1, v3); y2 = csub(v0, v2); y3 = csub(v1, v3);
}

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// v of another lane of the same row of 16 by a DPP control: quad_perm [1,0,3,2] (lane ^ 1), quad_perm [2,3,0,1] (lane ^ 2),
// row_half_mirror (7 - lane within 8), row_mirror (15 - lane within 16)
template <int CTRL>
__device__ inline float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
constexpr int kQuadXor1 = 0xb1, kQuadXor2 = 0x4e, kHalfMirror = 0x141, kRowMirror = 0x140;

// Sum of v over aligned groups of 2^steps lanes (steps in 0 .. 6), left in every lane of the group.  After the two quad steps a
// quad's lanes agree, so the mirrors pair each lane with one of the other half: the sum of 8, then of 16.
__device__ inline float group_sum(float v, int steps) {
  if (steps > 0) v += dpp<kQuadXor1>(v);
  if (steps > 1) v += dpp<kQuadXor2>(v);
  if (steps > 2) v += dpp<kHalfMirror>(v);
  if (steps > 3) v += dpp<kRowMirror>(v);
  if (steps > 4) v += __shfl_xor(v, 16);
  if (steps > 5) v += __shfl_xor(v, 32);
  return v;
}

__device__ inline float power(float2 w) { return w.x * w.x + w.y * w.y; }

}  // namespace

// grid (N / span / 4, n_sources), span = max(128, g): wave w of a source owns bins [w span, (w + 1) span).
template <int HANN, int PEAK>
__global__ __launch_bounds__(ASDR_TUNER_MON_LANES) void asdr_tuner_fc_spectrum_kernel(FcSpectrumArgs a) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * (ASDR_TUNER_MON_LANES / 64) + (threadIdx.x >> 6), s = blockIdx.y;
  const int N = 1 << a.log2n, lg = a.log2n - a.log2b;        // g = 2^lg
  const int lspan = lg > 7 ? lg : 7, chunks = 1 << (lspan - 7);
  const int k0 = (wave << lspan) + 2 * lane;                  // this lane's first bin of chunk 0
  const int steps = lg > 7 ? 6 : lg - 1;                      // lanes per group = g / 2 (lg >= 1), at most the wave
  const float inv = ldexpf(1.0f, -2 * a.log2n);               // 1 / N^2
  double acc0 = 0.0, acc1 = 0.0;                              // powers are >= 0, so 0 also starts a maximum
  for (int f = 0; f < a.n_frames; f++) {
    const float2 *X = (const float2 *)a.x + (((size_t)s * a.n_frames + f) << a.log2n);
    float p0 = 0.0f, p1 = 0.0f;
    for (int c = 0; c < chunks; c++) {
      const int k = k0 + (c << 7);
      const float4 v = *(const float4 *)(X + k);
      float2 w0 = make_float2(v.x, v.y), w1 = make_float2(v.z, v.w);
      if (HANN) {
        float2 prev = make_float2(__shfl_up(v.z, 1), __shfl_up(v.w, 1)), next = make_float2(__shfl_down(v.x, 1), __shfl_down(v.y, 1));
        if (lane == 0) prev = X[(k - 1) & (N - 1)];
        if (lane == 63) next = X[(k + 2) & (N - 1)];
        const float2 x0 = w0, x1 = w1;
        w0 = make_float2(0.5f * x0.x - 0.25f * (prev.x + x1.x), 0.5f * x0.y - 0.25f * (prev.y + x1.y));
        w1 = make_float2(0.5f * x1.x - 0.25f * (x0.x + next.x), 0.5f * x1.y - 0.25f * (x0.y + next.y));
      }
      p0 += power(w0) * inv; p1 += power(w1) * inv;
    }
    if (lg == 0) {                                            // B = N: both bins are output bins
      acc0 = PEAK ? fmax(acc0, (double)p0) : acc0 + (double)p0;
      acc1 = PEAK ? fmax(acc1, (double)p1) : acc1 + (double)p1;
    } else {
      const float P = group_sum(p0 + p1, steps);
      acc0 = PEAK ? fmax(acc0, (double)P) : acc0 + (double)P;
    }
  }
  double *row = a.acc + ((size_t)s << a.log2b);
  if (lg == 0) {
    double2 *o = (double2 *)(row + k0);
    const double2 old = *o;
    *o = PEAK ? make_double2(fmax(old.x, acc0), fmax(old.y, acc1)) : make_double2(old.x + acc0, old.y + acc1);
  } else if ((lane & ((1 << steps) - 1)) == 0) {              // the group's first lane owns output bin j
    double *o = row + (k0 >> lg);
    *o = PEAK ? fmax(*o, acc0) : *o + acc0;
  }
}

// asdr_tuner_fc_channel_kernel with the level epilogue: everything up to the int16 stores is that kernel's text.
__global__ __launch_bounds__(ASDR_TUNER_FC_CH_LANES) void asdr_tuner_fc_channel_level_kernel(FcChannelArgs a, FcLevelArgs lv) {
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

  // level: e_b[c] = sum_n |y[n] / N|^2 over the 128 kept samples, before the NCO (unit modulus), the rounding and the clamp
  const float y2s = power(make_float2(y2.x * scale, y2.y * scale)), y3s = power(make_float2(y3.x * scale, y3.y * scale));
  const float r = group_sum(y2s + y3s, 4);                   // each row of 16 lanes holds its sum
  const float e0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 0));
  const float e1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 16));
  const float e2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 32));
  const float e3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 48));
  if (t == 0) lv.part[(size_t)f * a.n_channels + c] = (e0 + e1) + (e2 + e3);
}

// level[c] += the call's e_b[c], frames in order
__global__ __launch_bounds__(256) void asdr_tuner_fc_level_fold_kernel(FcLevelArgs lv, int n_channels, int n_frames) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n_channels) return;
  double s = lv.acc[c];
  for (int f = 0; f < n_frames; f++) s += (double)lv.part[(size_t)f * n_channels + c];
  lv.acc[c] = s;
}

extern "C" int asdr_launch_tuner_spectrum(const FcSpectrumArgs *sp, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int lg = sp->log2n - sp->log2b, lspan = lg > 7 ? lg : 7;
  const dim3 grid((1u << (sp->log2n - lspan)) / (ASDR_TUNER_MON_LANES / 64), sp->n_sources), block(ASDR_TUNER_MON_LANES);
  const bool hann = sp->window == ASDR_TUNER_WIN_HANN, peak = sp->mode == ASDR_TUNER_MON_PEAK;
  if (hann && peak) hipLaunchKernelGGL((asdr_tuner_fc_spectrum_kernel<1, 1>), grid, block, 0, stream, *sp);
  else if (hann) hipLaunchKernelGGL((asdr_tuner_fc_spectrum_kernel<1, 0>), grid, block, 0, stream, *sp);
  else if (peak) hipLaunchKernelGGL((asdr_tuner_fc_spectrum_kernel<0, 1>), grid, block, 0, stream, *sp);
  else hipLaunchKernelGGL((asdr_tuner_fc_spectrum_kernel<0, 0>), grid, block, 0, stream, *sp);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_tuner_channel_levels(const FcChannelArgs *c, const FcLevelArgs *lv, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(asdr_tuner_fc_channel_level_kernel, dim3(c->n_channels, c->n_frames), dim3(ASDR_TUNER_FC_CH_LANES), 0, stream, *c, *lv);
  if (hipGetLastError() != hipSuccess) return -1;
  return asdr_launch_tuner_level_fold(lv, c->n_channels, c->n_frames, stream_);
}

extern "C" int asdr_launch_tuner_level_fold(const FcLevelArgs *lv, int n_channels, int n_frames, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(asdr_tuner_fc_level_fold_kernel, dim3((n_channels + 255) / 256), dim3(256), 0, stream, *lv, n_channels, n_frames);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
