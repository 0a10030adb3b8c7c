// asdr_tuner_palette.hip -- the channel step of a fast-convolution bank whose channels choose their filter from a palette and carry
// a gain (include/asdr_tuner.h, "Filter palette and gain").  A bank with every channel on slot 0 at gain 1 launches nothing from
// this file: asdr_tuner_fastconv.hip and asdr_tuner_monitor.hip keep their kernels, untouched.
//
// Form: asdr_tuner_fc_channel_palette_kernel<LEVELS> is asdr_tuner_fc_channel_kernel (asdr_tuner_fastconv.hip;
// LEVELS: asdr_tuner_fc_channel_level_kernel, asdr_tuner_monitor.hip) with two changes.  G is row f_c of the palette's table
// [64][256]: the channel, hence the slot and the row's address, are the same for the whole wave, so the row base lives in SGPRs and
// the gather's four 512-byte row loads stay what they were.  a_c is multiplied into the 1 / N scale (+-2^-log2 N: the product is
// exact).  Every other statement is that kernel's, in its order (the build has no FMA contraction), so a channel on slot 0 at
// gain 1 comes out bit for bit as the plain kernel writes it.  The level epilogue uses the scale without a_c: a level is the
// signal's.  One wave per (channel, frame), the (source, k0) schedule order, 2 KB of LDS.
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"

namespace {

// the helpers of asdr_tuner_fastconv.hip and asdr_tuner_monitor.hip, which keep them file-local
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

template <int CTRL>
__device__ inline float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
constexpr int kQuadXor1 = 0xb1, kQuadXor2 = 0x4e, kHalfMirror = 0x141, kRowMirror = 0x140;

// sum of v over each row of 16 lanes, left in every lane of the row (asdr_tuner_monitor.hip's group_sum with steps = 4)
__device__ inline float row_sum(float v) {
  v += dpp<kQuadXor1>(v);
  v += dpp<kQuadXor2>(v);
  v += dpp<kHalfMirror>(v);
  v += dpp<kRowMirror>(v);
  return v;
}

__device__ inline float power(float2 w) { return w.x * w.x + w.y * w.y; }

}  // namespace

template <int LEVELS>
__global__ __launch_bounds__(ASDR_TUNER_FC_CH_LANES) void asdr_tuner_fc_channel_palette_kernel(FcChannelArgs a, FcPaletteArgs pal,
                                                                                                FcLevelArgs lv) {
  __shared__ float2 buf[256];
  const int t = threadIdx.x;
  const int c = a.order[blockIdx.x], f = blockIdx.y;
  const asdr_tuner_state_t st = a.chan[c];
  const int lq = 32 - a.log2n, N = 1 << a.log2n;
  const int k0 = (int)(((int64_t)(int32_t)st.fw + (1LL << (lq - 1))) >> lq);   // floor(((int32) fw + q / 2) / q)
  const uint32_t rw = st.fw - ((uint32_t)k0 << lq);
  const float2 *X = (const float2 *)a.x + (((size_t)st.src * a.n_frames + f) << a.log2n);
  // row f_c of the table: c comes from blockIdx, so the slot, the gain and this address are the wave's (scalar loads, SGPRs)
  const float2 *G = (const float2 *)pal.tab + ((size_t)(pal.slot[c] & (ASDR_TUNER_FC_MAX_FILTERS - 1)) << 8);
  const float gain = pal.gain[c];
  const float2 *tw = (const float2 *)a.tw256;

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
  const float unit = ldexpf((((int)k0 & 1) && ((b - 1) & 1)) ? -1.0f : 1.0f, -a.log2n);   // 1 / N and (-1)^{k0 (b - 1)}
  const float scale = unit * gain;                           // times a_c: exact, unit is a power of two
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

  if (LEVELS) {
    // level: e_b[c] = sum_n |y[n] / N|^2 over the 128 kept samples, before the gain, the NCO, the rounding and the clamp
    const float y2s = power(make_float2(y2.x * unit, y2.y * unit)), y3s = power(make_float2(y3.x * unit, y3.y * unit));
    const float r = row_sum(y2s + y3s);                      // each row of 16 lanes holds its sum
    const float e0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 0));
    const float e1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 16));
    const float e2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 32));
    const float e3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(r), 48));
    if (t == 0) lv.part[(size_t)f * a.n_channels + c] = (e0 + e1) + (e2 + e3);
  }
}

// the channel step of a bank with a palette in use; with lv, the level epilogue and then the fold of the call's partials
extern "C" int asdr_launch_tuner_channel_palette(const FcChannelArgs *c, const FcPaletteArgs *pal, const FcLevelArgs *lv,
                                                 void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const dim3 grid(c->n_channels, c->n_frames), block(ASDR_TUNER_FC_CH_LANES);
  if (lv) {
    hipLaunchKernelGGL(asdr_tuner_fc_channel_palette_kernel<1>, grid, block, 0, stream, *c, *pal, *lv);
    if (hipGetLastError() != hipSuccess) return -1;
    return asdr_launch_tuner_level_fold(lv, c->n_channels, c->n_frames, stream);
  }
  FcLevelArgs none;
  none.part = nullptr; none.acc = nullptr;
  hipLaunchKernelGGL(asdr_tuner_fc_channel_palette_kernel<0>, grid, block, 0, stream, *c, *pal, none);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
