// asdr_tuner.hip -- kernels of the digital tuner bank (include/asdr_tuner.h): NCO mixer + decimating FIR per channel, then the
// per-source history step.  Kept out of asdr_kernels.hip, whose kernels are the chain's launch census.
//
// Form: one workgroup of 128 lanes = one channel x one 128-sample output block; lane t computes output
// n = 128 * block + t, I and Q.  The channel's mixed input z is staged in LDS in POLYPHASE order: with tap k = a D + b the filter is
//   I[n] = sum_a sum_b h[aD + b] zr[(n - a) D + (D - 1 - b)],
// so z is stored as rows of phase p = D - 1 - b over q = n - a.  Two adjacent phases share one 32-bit word (zr2[pp][q] =
// zr[qD + 2pp] | zr[qD + 2pp + 1] << 16), and the matching tap pair (h[aD + D - 1 - 2pp], h[aD + D - 2 - 2pp]) is the same for every
// lane: one v_dot2_i32_i16 per word, the word address moving by one dword from lane to lane (no bank conflicts for any D), the tap
// pair a wave-uniform scalar load.  Taps past L and the pad phase of an odd D are zero.
//
// Input formats (include/asdr_tuner.h): asdr_tuner_kernel / asdr_tuner_history_kernel are the CS16 bank's, as
// they were; asdr_tuner_fmt_kernel<F> / asdr_tuner_fmt_history_kernel<F> are the same steps with the conversion in the load
// (asdr_fetch, asdr_tuner_device.h).  A 2-byte format's word (two adjacent samples) comes from one aligned dword when its first
// sample is even; the history row always holds converted CS16 words.  RS16 drops the two xi products of the mixer (xi = 0).
#include <hip/hip_runtime.h>

#include "asdr_tuner_device.h"
#include "asdr_tuner_tables.h"

__constant__ int32_t asdr_tuner_nco[ASDR_TUNER_NCO_SIZE] = {ASDR_TUNER_NCO_TABLE_INIT};

typedef short short2_t __attribute__((ext_vector_type(2)));

namespace {

constexpr int kOut = 128;   // outputs per workgroup = lanes

__device__ inline int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// z of one input word (re low, im high) at NCO phase theta
__device__ inline void mix(int32_t word, uint32_t theta, int &zr, int &zi) {
  const int32_t cs = asdr_tuner_nco[theta >> 20];
  const int c = (int16_t)(cs & 0xffff), s = cs >> 16;
  const int xr = (int16_t)(word & 0xffff), xi = word >> 16;
  zr = sat16((xr * c + xi * s + 16384) >> 15);   // |xr c| + |xi s| <= 2 * 32768 * 32767 < 2^31: exact in int32
  zi = sat16((xi * c - xr * s + 16384) >> 15);
}

// z of a real sample (xi = 0): the same statement without its two zero products
__device__ inline void mix_real(int32_t word, uint32_t theta, int &zr, int &zi) {
  const int32_t cs = asdr_tuner_nco[theta >> 20];
  const int c = (int16_t)(cs & 0xffff), s = cs >> 16;
  const int xr = (int16_t)(word & 0xffff);
  zr = sat16((xr * c + 16384) >> 15);
  zi = sat16((16384 - xr * s) >> 15);
}

template <int F>
__device__ inline void mix_fmt(int32_t word, uint32_t theta, int &zr, int &zi) {
  if constexpr (F == ASDR_TUNER_IN_RS16) mix_real(word, theta, zr, zi); else mix(word, theta, zr, zi);
}

__device__ inline int dot2(int32_t z, int32_t h, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2_t, z), __builtin_bit_cast(short2_t, h), acc, false);
}

}  // namespace

__global__ __launch_bounds__(kOut) void asdr_tuner_kernel(TunerArgs a) {
  extern __shared__ int32_t lds[];
  const int t = threadIdx.x;
  const int c = a.order[blockIdx.x];
  const int blk = blockIdx.y;
  const int D = a.decimation, A = a.n_phase_rows, DP2 = a.n_phase_pairs;
  const int QL = kOut + A - 1;              // q = n - a over the block: q0 .. q0 + QL - 1
  const int QS = QL | 1;
  const int q0 = blk * kOut - (A - 1);
  int32_t *zr2 = lds, *zi2 = lds + DP2 * QS;

  const asdr_tuner_state_t st = a.chan[c];
  const int64_t rel = a.pos - st.pos_a;     // >= 0: anchors are set at positions already reached
  const uint32_t theta0 = st.ph_a + (uint32_t)rel * st.fw;   // theta(P + m) = theta0 + m * fw mod 2^32, exactly
  const int first = rel >= (1 << 30) ? -(1 << 30) : -(int)rel;   // z = 0 for m < first (before the anchor)
  const int32_t *row = a.in + st.src * a.in_stride;
  const int32_t *hrow = a.hist_rd + (size_t)st.src * ASDR_TUNER_HIST_SLOTS;

  // mixer: word (pp, ql) = phases 2pp, 2pp + 1 at q = q0 + ql, i.e. input samples m = q D + 2pp (+1), m >= -(A - 1) D >= -1023
  {
    int pp = t % DP2, ql = t / DP2;
    const int dp = kOut % DP2, dq = kOut / DP2;
    for (; ql < QL; ) {
      const int m = (q0 + ql) * D + 2 * pp;
      int r0 = 0, i0 = 0, r1 = 0, i1 = 0;
      if (m >= first) mix(m >= 0 ? row[m] : hrow[ASDR_TUNER_HIST_SLOTS + m], theta0 + (uint32_t)m * st.fw, r0, i0);
      if (2 * pp + 1 < D && m + 1 >= first)
        mix(m + 1 >= 0 ? row[m + 1] : hrow[ASDR_TUNER_HIST_SLOTS + m + 1], theta0 + (uint32_t)(m + 1) * st.fw, r1, i1);
      zr2[pp * QS + ql] = (r0 & 0xffff) | (r1 << 16);
      zi2[pp * QS + ql] = (i0 & 0xffff) | (i1 << 16);
      pp += dp; ql += dq;
      if (pp >= DP2) { pp -= DP2; ql++; }
    }
  }
  __syncthreads();

  // filter: lane t = output n; row a of the polyphase taps meets z at q = n - a, i.e. ql = t + A - 1 - a
  int acc_i = 0, acc_q = 0;
  const int32_t *taps = a.taps;
  for (int ar = 0; ar < A; ar++) {
    const int ql = t + A - 1 - ar;
    const int32_t *hr = taps + ar * DP2;
    for (int pp = 0; pp < DP2; pp++) {
      const int32_t h = hr[pp];
      acc_i = dot2(zr2[pp * QS + ql], h, acc_i);
      acc_q = dot2(zi2[pp * QS + ql], h, acc_q);
    }
  }
  const int64_t o = (int64_t)c * a.out_stride + (int64_t)blk * kOut + t;
  a.out_i[o] = (int16_t)sat16((acc_i + a.round) >> a.shift);
  a.out_q[o] = (int16_t)sat16((acc_q + a.round) >> a.shift);
}

// history: slot j of source s after the call = sample P + N - 1024 + j (from this call's input, or the old row)
__global__ __launch_bounds__(256) void asdr_tuner_history_kernel(TunerArgs a) {
  const int s = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
  const int n_in = a.n_blocks * kOut * a.decimation;
  const int m = n_in - ASDR_TUNER_HIST_SLOTS + j;
  const int32_t *row = a.in + s * a.in_stride;
  const int32_t *hrow = a.hist_rd + (size_t)s * ASDR_TUNER_HIST_SLOTS;
  a.hist_wr[(size_t)s * ASDR_TUNER_HIST_SLOTS + j] = m >= 0 ? row[m] : hrow[ASDR_TUNER_HIST_SLOTS + m];
}

// asdr_tuner_kernel for a bank of format F != CS16: the mixer's loads convert, everything after the mixer is the same code.
template <int F>
__global__ __launch_bounds__(kOut) void asdr_tuner_fmt_kernel(TunerArgs a) {
  extern __shared__ int32_t lds[];
  const int t = threadIdx.x;
  const int c = a.order[blockIdx.x];
  const int blk = blockIdx.y;
  const int D = a.decimation, A = a.n_phase_rows, DP2 = a.n_phase_pairs;
  const int QL = kOut + A - 1;
  const int QS = QL | 1;
  const int q0 = blk * kOut - (A - 1);
  int32_t *zr2 = lds, *zi2 = lds + DP2 * QS;

  const asdr_tuner_state_t st = a.chan[c];
  const int64_t rel = a.pos - st.pos_a;
  const uint32_t theta0 = st.ph_a + (uint32_t)rel * st.fw;
  const int first = rel >= (1 << 30) ? -(1 << 30) : -(int)rel;
  const char *row = (const char *)a.in + st.src * a.in_stride * ASDR_TUNER_FMT_BYTES(F);
  const int32_t *hrow = a.hist_rd + (size_t)st.src * ASDR_TUNER_HIST_SLOTS;

  {
    int pp = t % DP2, ql = t / DP2;
    const int dp = kOut % DP2, dq = kOut / DP2;
    for (; ql < QL; ) {
      const int m = (q0 + ql) * D + 2 * pp;
      const bool two = 2 * pp + 1 < D;
      int32_t w0, w1 = 0;
      // The loads are not guarded by m >= first as the CS16 kernel's are: a sample before the anchor is loaded and dropped (its z
      // stays 0 below).  Every such address exists: m >= -1023, so the history slot is there, and the rows hold m < n_in.
      // m even and in the call's rows: m + 1 is in them too (a row holds an even number of samples), one load gives both
      if (ASDR_TUNER_FMT_BYTES(F) == 2 && m >= 0 && (m & 1) == 0) {
        asdr_fetch2<F>(row, m, w0, w1);
      } else {
        w0 = m >= 0 ? asdr_fetch<F>(row, m) : hrow[ASDR_TUNER_HIST_SLOTS + m];
        if (two) w1 = m + 1 >= 0 ? asdr_fetch<F>(row, m + 1) : hrow[ASDR_TUNER_HIST_SLOTS + m + 1];
      }
      int r0 = 0, i0 = 0, r1 = 0, i1 = 0;
      if (m >= first) mix_fmt<F>(w0, theta0 + (uint32_t)m * st.fw, r0, i0);
      if (two && m + 1 >= first) mix_fmt<F>(w1, theta0 + (uint32_t)(m + 1) * st.fw, r1, i1);
      zr2[pp * QS + ql] = (r0 & 0xffff) | (r1 << 16);
      zi2[pp * QS + ql] = (i0 & 0xffff) | (i1 << 16);
      pp += dp; ql += dq;
      if (pp >= DP2) { pp -= DP2; ql++; }
    }
  }
  __syncthreads();

  int acc_i = 0, acc_q = 0;
  const int32_t *taps = a.taps;
  for (int ar = 0; ar < A; ar++) {
    const int ql = t + A - 1 - ar;
    const int32_t *hr = taps + ar * DP2;
    for (int pp = 0; pp < DP2; pp++) {
      const int32_t h = hr[pp];
      acc_i = dot2(zr2[pp * QS + ql], h, acc_i);
      acc_q = dot2(zi2[pp * QS + ql], h, acc_q);
    }
  }
  const int64_t o = (int64_t)c * a.out_stride + (int64_t)blk * kOut + t;
  a.out_i[o] = (int16_t)sat16((acc_i + a.round) >> a.shift);
  a.out_q[o] = (int16_t)sat16((acc_q + a.round) >> a.shift);
}

// history for a bank of format F != CS16: lane = slots 2j, 2j + 1 (samples m even, m + 1: both from the call or both from the old
// row, since the call's sample count is even), converted and written as one 8-byte store
template <int F>
__global__ __launch_bounds__(256) void asdr_tuner_fmt_history_kernel(TunerArgs a) {
  const int s = blockIdx.x, j = 2 * (blockIdx.y * 256 + threadIdx.x);
  const int n_in = a.n_blocks * kOut * a.decimation;
  const int m = n_in - ASDR_TUNER_HIST_SLOTS + j;
  const char *row = (const char *)a.in + s * a.in_stride * ASDR_TUNER_FMT_BYTES(F);
  const int32_t *hrow = a.hist_rd + (size_t)s * ASDR_TUNER_HIST_SLOTS;
  int2 w;
  if (m >= 0) asdr_fetch2<F>(row, m, w.x, w.y);
  else w = *(const int2 *)(hrow + ASDR_TUNER_HIST_SLOTS + m);
  *(int2 *)(a.hist_wr + (size_t)s * ASDR_TUNER_HIST_SLOTS + j) = w;
}

template <int F>
static int launch_fmt(const TunerArgs *a, size_t lds, hipStream_t stream) {
  hipLaunchKernelGGL(asdr_tuner_fmt_kernel<F>, dim3(a->n_channels, a->n_blocks), dim3(kOut), lds, stream, *a);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(asdr_tuner_fmt_history_kernel<F>, dim3(a->n_sources, ASDR_TUNER_HIST_SLOTS / 512), dim3(256), 0, stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int asdr_launch_tuner(const TunerArgs *a, void *stream) {
  const int QS = (kOut + a->n_phase_rows - 1) | 1;
  const size_t lds = 2 * (size_t)a->n_phase_pairs * QS * sizeof(int32_t);   // <= 2 * 32 * 145 * 4 = 37,120 B (D = 63, L = 1024)
  switch (a->fmt) {
    case ASDR_TUNER_IN_CS16: break;
    case ASDR_TUNER_IN_CU8: return launch_fmt<ASDR_TUNER_IN_CU8>(a, lds, (hipStream_t)stream);
    case ASDR_TUNER_IN_CS8: return launch_fmt<ASDR_TUNER_IN_CS8>(a, lds, (hipStream_t)stream);
    case ASDR_TUNER_IN_CF32: return launch_fmt<ASDR_TUNER_IN_CF32>(a, lds, (hipStream_t)stream);
    case ASDR_TUNER_IN_RS16: return launch_fmt<ASDR_TUNER_IN_RS16>(a, lds, (hipStream_t)stream);
    default: return -1;
  }
  hipLaunchKernelGGL(asdr_tuner_kernel, dim3(a->n_channels, a->n_blocks), dim3(kOut), lds, (hipStream_t)stream, *a);
  if (hipGetLastError() != hipSuccess) return -1;
  hipLaunchKernelGGL(asdr_tuner_history_kernel, dim3(a->n_sources, ASDR_TUNER_HIST_SLOTS / 256), dim3(256), 0, (hipStream_t)stream, *a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
