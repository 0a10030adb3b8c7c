// asdr_fir.h -- the folded 257-tap Hilbert FIR shared by the update kernels (AudioSDR.cpp:99-110) and the IQ generator
// (AudioIQgenerator.cpp:60-76): same structure, different taps.  Device code only.
#ifndef ASDR_FIR_H
#define ASDR_FIR_H
#include <hip/hip_runtime.h>

typedef float v2f __attribute__((ext_vector_type(2)));   // one aligned VGPR pair: operand of v_pk_mul_f32 / v_pk_add_f32
#ifndef SCHED_FENCE
#define SCHED_FENCE() do { } while (0)
#endif

// Output pairs E0 .. E0 + NE - 1 of this lane's eight (outputs i = 16 s8 + 2e, + 1):
//   Q[i] = sum_k h[k] * (x[255 + i - 2k] - x[i + 2k + 1]),  k = 0..63 ascending, accumulate from 0.0, every operation separately rounded
// `hist` holds three blocks of history in natural order shifted by one float -- x[m] at hist[m - 1], m = 1..383 (x[0] is never
// used) -- so that every operand pair PX[p] = (x[2p+1], x[2p+2]) is an 8-byte-aligned LDS pair.  The operands of the output pair e
// are PX[127 + p0 + e - k] and PX[p0 + e + k] (p0 = 8 s8): per chunk of 8 taps two contiguous (NE + 7)-pair register windows
// (ds_read_b128).  v_pk_mul_f32 / v_pk_add_f32 round each half exactly like the scalar ops, so the result is bit-identical to
// the scalar loop.  `taps`: 64 floats in constant memory (uniform address: scalar loads).
template <int E0, int NE>
__device__ __forceinline__ void hilbert_fir_rows(const float *hist, int p0, v2f *acc2, const float *taps) {
  constexpr int NW = NE + 7;
  const v2f *PX = reinterpret_cast<const v2f *>(hist) + E0;
#pragma unroll 1
  for (int kc = 0; kc < 8; ++kc) {
    v2f dw[NW], uw[NW];   // dw[t] = PX[120 + p0 - 8kc + t], uw[t] = PX[p0 + 8kc + t]  (t = 0..NW-1, pairs counted from E0)
    const float4 *dp = reinterpret_cast<const float4 *>(PX + 120 + p0 - 8 * kc);
    const float4 *up = reinterpret_cast<const float4 *>(PX + p0 + 8 * kc);
#pragma unroll
    for (int q = 0; q < NW / 2; ++q) {
      const float4 d4 = dp[q], u4 = up[q];
      dw[2 * q] = (v2f){d4.x, d4.y}; dw[2 * q + 1] = (v2f){d4.z, d4.w};
      uw[2 * q] = (v2f){u4.x, u4.y}; uw[2 * q + 1] = (v2f){u4.z, u4.w};
    }
    if (NW & 1) { dw[NW - 1] = PX[120 + p0 - 8 * kc + NW - 1]; uw[NW - 1] = PX[p0 + 8 * kc + NW - 1]; }
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const float hk = taps[8 * kc + kk];
      const v2f hk2 = (v2f){hk, hk};
      v2f d[NE];   // the pair-chains of a tap are independent: issue them interleaved (no dependent back-to-back pk ops)
#pragma unroll
      for (int e = 0; e < NE; ++e) d[e] = dw[7 + e - kk] - uw[e + kk];
#pragma unroll
      for (int e = 0; e < NE; ++e) d[e] = hk2 * d[e];
#pragma unroll
      for (int e = 0; e < NE; ++e) acc2[e] += d[e];
      SCHED_FENCE();
    }
  }
}

// The same sums with SLIDING windows in a closed register ring, for the four-wave update kernels (all eight output pairs of a lane).  Tap T of the
// output pair e reads D[63 - T + e] and U[T + e], D[t] = PX[64 + p0 + t], U[t] = PX[p0 + t]: from tap to tap the down window moves one pair down, the up
// window one pair up.  Pair t of a window lives in register pair t mod 16 -- the eight live ones plus the pieces requested ahead -- and every second tap
// requests one 16-byte piece per window, the pairs that taps T + 4 .. T + 6 bring in: no tap waits on a read issued less than four taps before it, and the
// FIR issues 2 x (6 + 32) = 76 LDS reads where the chunked form issues 8 x 16 and drains them eight times.  Sixteen taps move a window by exactly 16 pairs, so a trip of 16
// taps closes the register naming: 4 trips, one load of 16 taps each (a scalar load shares its counter with the LDS reads: inside a trip it would drain them).
// The last trip's last two requests bring in pairs no tap uses (D[-4 .. -1], U[72 .. 75]: words 2 p0 + 120 .. 127 and 2 p0 + 144 .. 151 <= 263 of the row).
// D[71], requested with D[70] in front of the loop, ends at word 383 for the last lane of a channel: inside the row, the value unused.
// Per accumulator the same sub, mul, add on the same operands in the same order as above: bit-identical.
__device__ __forceinline__ void hilbert_fir_rows_ring(const float *hist, int p0, v2f *acc2, const float *taps) {
  constexpr int NE = 8;
  const v2f *PD = reinterpret_cast<const v2f *>(hist) + 64 + p0;   // D[0]
  const v2f *PU = reinterpret_cast<const v2f *>(hist) + p0;        // U[0]
  v2f D[16], U[16];   // D[t] at D[t & 15], U[t] at U[t & 15]
  auto ld2 = [](const v2f *p, v2f &a, v2f &b) { const float4 q = *reinterpret_cast<const float4 *>(p); a = (v2f){q.x, q.y}; b = (v2f){q.z, q.w}; };
  // taps 0..3: D[60..70] and U[0..10], whole 16-byte pieces
#pragma unroll
  for (int t = 60; t < 72; t += 2) ld2(PD + t, D[t & 15], D[(t + 1) & 15]);
#pragma unroll
  for (int t = 0; t < 12; t += 2) ld2(PU + t, U[t], U[t + 1]);
#pragma unroll 1
  for (int tc = 0; tc < 4; ++tc) {
    float h[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) h[i] = taps[16 * tc + i];
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) {   // tap T = 16 tc + tt
      if ((tt & 1) == 0) {   // D[58 - T], D[59 - T] and U[12 + T], U[13 + T]
        ld2(PD + 58 - tt, D[(58 - tt) & 15], D[(59 - tt) & 15]);
        ld2(PU + 12 + tt, U[(12 + tt) & 15], U[(13 + tt) & 15]);
      }
      const v2f hk2 = (v2f){h[tt], h[tt]};
      v2f d[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e) d[e] = D[(63 - tt + e) & 15] - U[(tt + e) & 15];
#pragma unroll
      for (int e = 0; e < NE; ++e) d[e] = hk2 * d[e];
#pragma unroll
      for (int e = 0; e < NE; ++e) acc2[e] += d[e];
      if ((tt & 1) == 1) __builtin_amdgcn_sched_barrier(0);   // (the requests stay where they are written: nothing is asked for more than two taps early)
    }
    PD -= 16; PU += 16;
  }
}
#endif
