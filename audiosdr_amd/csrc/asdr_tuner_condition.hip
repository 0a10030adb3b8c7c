// asdr_tuner_condition.hip -- source conditioning of the tuner banks (include/asdr_tuner.h, "Source conditioning"): one pass over
// the caller's wideband rows, before any bank kernel, that (i) writes the DC- and I/Q-imbalance-corrected samples x' as CS16
// (RS16 for a real bank) into a bank-owned scratch the bank's unchanged kernels then read, and / or (ii) accumulates the exact
// integer moments and the clip count of the uncorrected x per source.  A bank with every correction at the identity and the
// statistics off launches nothing from this file.
//
// Form:
//  * grid (x, n_sources); a workgroup of 256 lanes strides over its row in steps of 256 items.  An item is 16 bytes of output
//    or of input, whichever is more: 4 CS16 samples (one 16-byte load, one 16-byte store), 8 CU8 / CS8 samples (one load, two
//    stores), 4 CF32 samples (two loads, one store), 8 RS16 samples (one load, one store).  A wave's loads and stores are
//    contiguous kilobytes.  Row and item offsets are 64-bit: in_stride_samples goes up to 2^40.
//  * the formats' conversions are restated here on unpacked parts (the bank kernels' loads in asdr_tuner_device.h produce packed
//    words); p a + g b is formed in 64 bits, |g b| reaches 2^33.
//  * statistics: six int64 partial sums per lane (a product of two int16 fits 32 bits), a wave reduction by shuffles, the four
//    waves through 192 bytes of LDS, then one 64-bit integer atomic add per workgroup and value; n is added once per row.  Integer
//    sums are exact in any order, so the result does not depend on the arrival order.  No float atomics.
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"

namespace {

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
__device__ inline int sat16_64(long long v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : (int)v); }

// Input formats, restated: a stored part to the int16 value of x
__device__ inline int part_cu8(uint32_t b) { return 256 * (int)b - 32640; }
__device__ inline int part_cs8(uint32_t b) { return 256 * (int)(int8_t)b; }
__device__ inline int part_f32(float a) {                   // sat16(rint(32768 a)), round half to even, NaN -> 0, +-inf saturate
  const float v = fminf(fmaxf(a * 32768.0f, -32768.0f), 32767.0f);
  return a != a ? 0 : (int)rintf(v);
}
// a part at the format's rail
__device__ inline bool rail_u8(uint32_t b) { return b == 0u || b == 255u; }
__device__ inline bool rail_s8(uint32_t b) { return b == 0x80u || b == 0x7fu; }
__device__ inline bool rail_16(int v) { return v == -32768 || v == 32767; }
__device__ inline bool rail_f32(float a) { return !(fabsf(a) < 1.0f); }   // |a| >= 1, +-inf, NaN

struct Sums { long long sr, si, srr, sii, sri, clip; };

template <bool STATS>
__device__ inline void take(Sums &s, int xr, int xi, bool clipped) {
  if (STATS) {
    s.sr += xr; s.si += xi;
    s.srr += xr * xr; s.sii += xi * xi; s.sri += xr * xi;   // |products| <= 2^30
    s.clip += clipped ? 1 : 0;
  }
}

// x' of a complex sample as a CS16 word (xr' low, xi' high); c = (d_r, d_i, p, g)
__device__ inline int32_t corrected(int xr, int xi, int4 c) {
  const int a = xr - c.x, b = xi - c.y;
  const long long q = (long long)c.z * a + (long long)c.w * b + 32768;
  return (sat16(a) & 0xffff) | (int32_t)((uint32_t)sat16_64(q >> 16) << 16);
}

// two stored 2-byte-format samples of one dword; F is CU8 or CS8
template <int F, bool WRITE, bool STATS>
__device__ inline void pair8(uint32_t d, int4 c, Sums &s, int32_t &w0, int32_t &w1) {
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t br = (d >> (16 * k)) & 0xffu, bi = (d >> (16 * k + 8)) & 0xffu;
    const int xr = F == ASDR_TUNER_IN_CU8 ? part_cu8(br) : part_cs8(br), xi = F == ASDR_TUNER_IN_CU8 ? part_cu8(bi) : part_cs8(bi);
    take<STATS>(s, xr, xi, F == ASDR_TUNER_IN_CU8 ? (rail_u8(br) || rail_u8(bi)) : (rail_s8(br) || rail_s8(bi)));
    if (WRITE) (k ? w1 : w0) = corrected(xr, xi, c);
  }
}

template <bool WRITE, bool STATS>
__device__ inline int32_t word16(int32_t w, int4 c, Sums &s) {
  const int xr = (int)(int16_t)(w & 0xffff), xi = w >> 16;
  take<STATS>(s, xr, xi, rail_16(xr) || rail_16(xi));
  return WRITE ? corrected(xr, xi, c) : 0;
}

template <bool WRITE, bool STATS>
__device__ inline int32_t pair_f32(float re, float im, int4 c, Sums &s) {
  const int xr = part_f32(re), xi = part_f32(im);
  take<STATS>(s, xr, xi, rail_f32(re) || rail_f32(im));
  return WRITE ? corrected(xr, xi, c) : 0;
}

// two real samples of one dword to two corrected int16 in one dword
template <bool WRITE, bool STATS>
__device__ inline int32_t pair_real(int32_t d, int4 c, Sums &s) {
  const int x0 = (int)(int16_t)(d & 0xffff), x1 = d >> 16;
  take<STATS>(s, x0, 0, rail_16(x0));
  take<STATS>(s, x1, 0, rail_16(x1));
  return WRITE ? ((sat16(x0 - c.x) & 0xffff) | (int32_t)((uint32_t)sat16(x1 - c.x) << 16)) : 0;
}

}  // namespace

// grid (x, n_sources).  ALIGNED = 0 (CS16 only): the rows start on a sample, not on 16 bytes, and are read by dwords.
template <int F, bool WRITE, bool STATS, bool ALIGNED>
__global__ __launch_bounds__(ASDR_TUNER_COND_LANES) void asdr_tuner_condition_kernel(ConditionArgs a) {
  constexpr int kPerItem = (F == ASDR_TUNER_IN_CS16 || F == ASDR_TUNER_IN_CF32) ? 4 : 8;   // samples
  constexpr int kInBytes = kPerItem * ASDR_TUNER_FMT_BYTES(F);                              // 16, or 32 for CF32
  constexpr int kOutBytes = kPerItem * (F == ASDR_TUNER_IN_RS16 ? 2 : 4);                   // 16, or 32 for CU8 / CS8
  const int s = blockIdx.y;
  const char *in = (const char *)a.in + (int64_t)s * a.in_stride * ASDR_TUNER_FMT_BYTES(F);
  char *out = WRITE ? (char *)a.out + (int64_t)s * a.out_stride * (F == ASDR_TUNER_IN_RS16 ? 2 : 4) : nullptr;
  const int4 c = WRITE ? ((const int4 *)a.corr)[s] : make_int4(0, 0, 0, 65536);
  const int64_t items = a.n_samples / kPerItem, step = (int64_t)gridDim.x * ASDR_TUNER_COND_LANES;
  Sums sum = {0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * ASDR_TUNER_COND_LANES + threadIdx.x; i < items; i += step) {
    const char *src = in + i * kInBytes;
    char *dst = out + i * kOutBytes;
    if constexpr (F == ASDR_TUNER_IN_CS16) {
      int4 v;
      if (ALIGNED) {
        v = *(const int4 *)src;
      } else {
        const int32_t *w = (const int32_t *)src;
        v = make_int4(w[0], w[1], w[2], w[3]);
      }
      const int4 o = make_int4(word16<WRITE, STATS>(v.x, c, sum), word16<WRITE, STATS>(v.y, c, sum),
                               word16<WRITE, STATS>(v.z, c, sum), word16<WRITE, STATS>(v.w, c, sum));
      if (WRITE) *(int4 *)dst = o;
    } else if constexpr (F == ASDR_TUNER_IN_CF32) {
      const float4 v0 = *(const float4 *)src, v1 = *(const float4 *)(src + 16);
      const int4 o = make_int4(pair_f32<WRITE, STATS>(v0.x, v0.y, c, sum), pair_f32<WRITE, STATS>(v0.z, v0.w, c, sum),
                               pair_f32<WRITE, STATS>(v1.x, v1.y, c, sum), pair_f32<WRITE, STATS>(v1.z, v1.w, c, sum));
      if (WRITE) *(int4 *)dst = o;
    } else if constexpr (F == ASDR_TUNER_IN_RS16) {
      const int4 v = *(const int4 *)src;
      const int4 o = make_int4(pair_real<WRITE, STATS>(v.x, c, sum), pair_real<WRITE, STATS>(v.y, c, sum),
                               pair_real<WRITE, STATS>(v.z, c, sum), pair_real<WRITE, STATS>(v.w, c, sum));
      if (WRITE) *(int4 *)dst = o;
    } else {
      const int4 v = *(const int4 *)src;
      int4 o0 = make_int4(0, 0, 0, 0), o1 = o0;
      pair8<F, WRITE, STATS>((uint32_t)v.x, c, sum, o0.x, o0.y);
      pair8<F, WRITE, STATS>((uint32_t)v.y, c, sum, o0.z, o0.w);
      pair8<F, WRITE, STATS>((uint32_t)v.z, c, sum, o1.x, o1.y);
      pair8<F, WRITE, STATS>((uint32_t)v.w, c, sum, o1.z, o1.w);
      if (WRITE) { *(int4 *)dst = o0; *(int4 *)(dst + 16) = o1; }
    }
  }
  if constexpr (STATS) {
    __shared__ long long red[ASDR_TUNER_COND_LANES / 64][6];
    long long v[6] = {sum.sr, sum.si, sum.srr, sum.sii, sum.sri, sum.clip};
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
      for (int k = 0; k < 6; k++) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    unsigned long long *row = a.stats + (size_t)s * ASDR_TUNER_IQ_STATS_WORDS;
    if (threadIdx.x < 6) {
      long long tot = 0;
#pragma unroll
      for (int w = 0; w < ASDR_TUNER_COND_LANES / 64; w++) tot += red[w][threadIdx.x];
      if (tot != 0) atomicAdd(row + 1 + threadIdx.x, (unsigned long long)tot);
    } else if (threadIdx.x == 6 && blockIdx.x == 0) {
      atomicAdd(row, (unsigned long long)a.n_samples);
    }
  }
}

namespace {
template <int F, bool ALIGNED>
int launch(const ConditionArgs *a, const dim3 &grid, hipStream_t stream) {
  const dim3 block(ASDR_TUNER_COND_LANES);
  if (a->out && a->stats) hipLaunchKernelGGL((asdr_tuner_condition_kernel<F, true, true, ALIGNED>), grid, block, 0, stream, *a);
  else if (a->out) hipLaunchKernelGGL((asdr_tuner_condition_kernel<F, true, false, ALIGNED>), grid, block, 0, stream, *a);
  else hipLaunchKernelGGL((asdr_tuner_condition_kernel<F, false, true, ALIGNED>), grid, block, 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
}  // namespace

extern "C" int asdr_launch_tuner_condition(const ConditionArgs *a, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if ((!a->out && !a->stats) || (a->out && !a->corr) || a->n_sources <= 0 || a->n_sources > 65535 || a->n_samples <= 0 ||
      a->n_samples % 128 != 0)
    return -1;
  const int per_item = (a->fmt == ASDR_TUNER_IN_CS16 || a->fmt == ASDR_TUNER_IN_CF32) ? 4 : 8;
  const int64_t want = (a->n_samples / per_item + ASDR_TUNER_COND_LANES - 1) / ASDR_TUNER_COND_LANES;
  const int64_t cap = ASDR_TUNER_COND_MAX_BLOCKS / a->n_sources > 0 ? ASDR_TUNER_COND_MAX_BLOCKS / a->n_sources : 1;
  const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)a->n_sources);
  switch (a->fmt) {
    case ASDR_TUNER_IN_CS16: return a->aligned ? launch<ASDR_TUNER_IN_CS16, true>(a, grid, stream) : launch<ASDR_TUNER_IN_CS16, false>(a, grid, stream);
    case ASDR_TUNER_IN_CU8: return a->aligned ? launch<ASDR_TUNER_IN_CU8, true>(a, grid, stream) : -1;
    case ASDR_TUNER_IN_CS8: return a->aligned ? launch<ASDR_TUNER_IN_CS8, true>(a, grid, stream) : -1;
    case ASDR_TUNER_IN_CF32: return a->aligned ? launch<ASDR_TUNER_IN_CF32, true>(a, grid, stream) : -1;
    case ASDR_TUNER_IN_RS16: return a->aligned ? launch<ASDR_TUNER_IN_RS16, true>(a, grid, stream) : -1;
  }
  return -1;
}
