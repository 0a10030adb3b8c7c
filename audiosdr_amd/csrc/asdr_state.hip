// asdr_state.hip -- receiver state records (include/asdr.h "receiver state records"): the two copy kernels between a
// batch's state rows (asdr_device.h) and the canonical per-channel records.
//
//   asdr_state_gather_kernel    state rows -> records   (asdr_export_state*)
//   asdr_state_scatter_kernel   records -> state rows   (asdr_import_state*)
//
// ONE WAVE PER LIST ENTRY, four entries per workgroup.  A record's signal part is 390 16-byte pieces; a wave moves it with seven
// 16-byte loads and seven 16-byte stores per lane, ALL loads issued before the first store (28 VGPRs of payload in flight per lane,
// as a copy kernel wants).  Each half-wave (32 lanes x 16 B) covers one whole 512-byte row segment -- one ring slot of nb_hist / hil_q /
// hil_i / als_x, or als_w, or audio_prev -- so the canonical order is address arithmetic only: the slot of the two batch-wide rings
// (UpdateArgs.nb_phase, als_phase) is a launch constant, the Hilbert parity one word per channel (ChanSmall.hil_slot, read by the
// gather; the scatter stores rows in canonical order with hil_slot = 0, which IS a valid ring position).  No lane exchanges data with
// another, no LDS, no scratch.  The seven instructions per lane ("items"):
//   A  lanes 0..27: ChanSmall (28 record pieces)     lanes 32..41: nb_mask (10 pieces)
//   B  lanes 0..31: nb_hist oldest                   lanes 32..63: nb_hist middle
//   C  lanes 0..31: nb_hist newest                   lanes 32..63: als_w
//   D  hil_q older | newer       E  hil_i older | newer       F  als_x previous | current
//   G  lanes 0..31: audio_prev                       lanes 32..41: the record's header + control part (gather only: written by the host)
// A record holds ChanSmall as 112 words in the ORIGINAL member order; the row in HBM is 512 bytes with the plain kind's fields in front
// (asdr_device.h).  Whole 16-byte pieces correspond (row_piece / rec_piece below), except that the record's piece 21 ends with a PLL word
// that the row keeps behind its other PLL words: the lanes of that piece and of the row's last PLL piece load two pieces and merge.
// The record's last five pieces are not a plain copy either: words 94 (unused) and 103.. (padding) are zero in a record, hil_slot is 0, and the
// six blanker gains rotate with the blanker ring -- the two lanes that hold them (record pieces 24, 25) load both pieces and select by the
// wave-uniform phase.  The scatter's lanes 0..31 write all 32 pieces of the row (padding zero).
// The record side is read / written once per call: non-temporal.  The state side is what the next update reads: plain.
#include <hip/hip_runtime.h>

#include "../../include/asdr.h"
#include "asdr_device.h"

namespace {

static_assert(sizeof(ChanSmall) == 512, "row layout");
static_assert(ASDR_STATE_OFF_NB_HIST - ASDR_STATE_OFF_SMALL == 448 && ASDR_STATE_OFF_NB_MASK - ASDR_STATE_OFF_NB_HIST == 1536 &&
              ASDR_STATE_OFF_HIL_Q - ASDR_STATE_OFF_NB_MASK == ASDR_NB_MASK_ROW && ASDR_STATE_OFF_HIL_I - ASDR_STATE_OFF_HIL_Q == 1024 &&
              ASDR_STATE_OFF_ALS_X - ASDR_STATE_OFF_HIL_I == 1024 && ASDR_STATE_OFF_ALS_W - ASDR_STATE_OFF_ALS_X == 1024 &&
              ASDR_STATE_OFF_AUDIO_PREV - ASDR_STATE_OFF_ALS_W == 512 && ASDR_STATE_RECORD_BYTES - ASDR_STATE_OFF_AUDIO_PREV == 512 &&
              ASDR_STATE_RECORD_BYTES % 256 == 0, "record layout");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 ld(const u32x4 *p) { return *p; }
__device__ __forceinline__ u32x4 ld_nt(const u32x4 *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st(u32x4 *p, u32x4 v) { *p = v; }
__device__ __forceinline__ void st_nt(u32x4 *p, u32x4 v) { __builtin_nontemporal_store(v, p); }

// The entry this wave works on: channel (local to the batch) and record index.  list == nullptr: entry e is channel ch0 + e, record rec0 + e.
struct Entry { int e, ch, rec; };
__device__ __forceinline__ bool wave_entry(const int2 *list, int n, int ch0, int rec0, Entry &en) {
  const int e = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (e >= n) return false;
  en.e = e;
  if (list) { const int2 v = list[e]; en.ch = __builtin_amdgcn_readfirstlane(v.x); en.rec = __builtin_amdgcn_readfirstlane(v.y); }
  else { en.ch = ch0 + e; en.rec = rec0 + e; }
  return true;
}

// blanker gains {g[slot][I, Q]} of pieces 24 | 25 = words (status, g0, g1, g2 | g3, g4, g5, pad): rotated LEFT by `rot` slots
// (out slot j = in slot (j + rot) % 3); rot is wave-uniform
__device__ __forceinline__ void rotate_gains(u32x4 &p24, u32x4 &p25, uint32_t rot) {
  const uint32_t g0 = p24.y, g1 = p24.z, g2 = p24.w, g3 = p25.x, g4 = p25.y, g5 = p25.z;
  if (rot == 1u) { p24.y = g2; p24.z = g3; p24.w = g4; p25.x = g5; p25.y = g0; p25.z = g1; }
  else if (rot == 2u) { p24.y = g4; p24.z = g5; p24.w = g0; p25.x = g1; p25.y = g2; p25.z = g3; }
  p25.w = 0u;
}

// A record keeps ChanSmall in its ORIGINAL field order (112 words: if_state, img_state, af_state, the scalars); the row in HBM has the plain kind's
// fields in its first 256 bytes (asdr_device.h).  Whole 16-byte pieces correspond, except where a PLL word sat between the scalars:
//   record piece   0..7    8..15    16..19   20   21             22   23                24   25
//   row piece      0..7    16..23   8..11    12   13.xyz | 25.z  24   25.xy (0, 0)      14   15 (.w = 0)
__device__ __forceinline__ int row_piece(int r) { return r < 8 ? r : r < 16 ? r + 8 : r < 20 ? r - 8 : r == 20 ? 12 : r == 21 ? 13 : r == 22 ? 24 : r == 23 ? 25 : r == 24 ? 14 : 15; }
__device__ __forceinline__ int row_piece2(int r) { return r == 21 ? 25 : r == 24 ? 15 : r == 25 ? 14 : -1; }
// ... and the other way: the record piece(s) row piece n (< 26) is made of
__device__ __forceinline__ int rec_piece(int n) { return n < 8 ? n : n < 12 ? n + 8 : n == 12 ? 20 : n == 13 ? 21 : n == 14 ? 24 : n == 15 ? 25 : n < 24 ? n - 8 : n == 24 ? 22 : 23; }
__device__ __forceinline__ int rec_piece2(int n) { return n == 14 ? 25 : n == 15 ? 24 : n == 25 ? 21 : -1; }
static_assert(offsetof(ChanSmall, af_state) == 16 * 8 && offsetof(ChanSmall, phase_ssb) == 16 * 12 && offsetof(ChanSmall, agc_gain) == 16 * 13 &&
              offsetof(ChanSmall, nb_slot_unused) == 16 * 13 + 12 && offsetof(ChanSmall, status) == 16 * 14 && offsetof(ChanSmall, nb_gain) == 16 * 14 + 4 &&
              offsetof(ChanSmall, hil_slot) == 16 * 15 + 12 && offsetof(ChanSmall, img_state) == 16 * 16 && offsetof(ChanSmall, pll_y_im) == 16 * 24 &&
              offsetof(ChanSmall, pll_phase_est) == 16 * 25 && offsetof(ChanSmall, pll_y_re) == 16 * 25 + 8, "piece map");

}  // namespace

// `records`: the caller's array; `ctl`: nullptr, or [n][10] pieces = header + control part of entry e (filled by the host)
extern "C" __global__ __launch_bounds__(256) void asdr_state_gather_kernel(UpdateArgs a, const int2 *list, int n, int ch0, int rec0,
                                                                           u32x4 *records, const u32x4 *ctl) {
  Entry en;
  if (!wave_entry(list, n, ch0, rec0, en)) return;
  const int lane = (int)(threadIdx.x & 63u), h = lane >> 5, l = lane & 31;
  const size_t ch = (size_t)en.ch;
  u32x4 *rec = records + (size_t)en.rec * (ASDR_STATE_RECORD_BYTES / 16);
  const u32x4 *small = reinterpret_cast<const u32x4 *>(a.small + ch);
  const u32x4 *nbh = reinterpret_cast<const u32x4 *>(a.nb_hist + ch * 768);
  const uint32_t p3 = a.nb_phase % 3u, p2 = a.als_phase & 1u;
  const uint32_t hs = a.small[ch].hil_slot & 1u;   // (one word per channel; the Hilbert loads below wait for it)
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 vA = zero, vA2 = zero, vB, vC, vD, vE, vF, vG = zero;
  const bool a_small = (h == 0 && l < 28), a_mask = (h == 1 && l < ASDR_NB_MASK_ROW / 16);
  // ---- loads
  if (a_small && l < 26) vA = ld(small + row_piece(l));
  if (a_small && row_piece2(l) >= 0) vA2 = ld(small + row_piece2(l));   // the other piece of the gains / the row piece that holds pll_y_re
  if (a_mask) vA = ld(reinterpret_cast<const u32x4 *>(a.nb_mask + ch * ASDR_NB_MASK_ROW) + l);
  vB = ld(nbh + ((p3 + (uint32_t)h) % 3u) * 32u + l);
  vC = h == 0 ? ld(nbh + ((p3 + 2u) % 3u) * 32u + l) : ld(reinterpret_cast<const u32x4 *>(a.als_w + ch * 128) + l);
  vD = ld(reinterpret_cast<const u32x4 *>(a.hil_q + ch * 256) + (((uint32_t)h ^ hs) * 32u + l));
  vE = ld(reinterpret_cast<const u32x4 *>(a.hil_i + ch * 256) + (((uint32_t)h ^ hs) * 32u + l));
  vF = ld(reinterpret_cast<const u32x4 *>(a.als_x + ch * 256) + (((uint32_t)h ^ p2 ^ 1u) * 32u + l));
  if (h == 0) { if (a.audio_prev) vG = ld(reinterpret_cast<const u32x4 *>(a.audio_prev + ch * 128) + l); }
  else if (ctl && l < ASDR_STATE_OFF_SMALL / 16) vG = ld_nt(ctl + (size_t)en.e * (ASDR_STATE_OFF_SMALL / 16) + l);
  // ---- the canonical form of ChanSmall's tail
  if (a_small) {
    if (l == 21) vA.w = vA2.z;                          // (agc_gain, agc_old_abs, agc_hang_counter | pll_y_re)
    else if (l == 23) { vA.z = 0u; vA.w = 0u; }         // (pll_phase_est, pll_freq | nb_slot_unused, hil_slot: zero in a record)
    else if (l == 24) { u32x4 o = vA2; rotate_gains(vA, o, p3); }
    else if (l == 25) { u32x4 o = vA2; rotate_gains(o, vA, p3); }
    else if (l >= 26) vA = zero;                        // padding
  }
  // ---- stores
  if (a_small) st_nt(rec + ASDR_STATE_OFF_SMALL / 16 + l, vA);
  if (a_mask) st_nt(rec + ASDR_STATE_OFF_NB_MASK / 16 + l, vA);
  st_nt(rec + ASDR_STATE_OFF_NB_HIST / 16 + lane, vB);
  st_nt(rec + (h == 0 ? ASDR_STATE_OFF_NB_HIST / 16 + 64 : ASDR_STATE_OFF_ALS_W / 16) + l, vC);
  st_nt(rec + ASDR_STATE_OFF_HIL_Q / 16 + lane, vD);
  st_nt(rec + ASDR_STATE_OFF_HIL_I / 16 + lane, vE);
  st_nt(rec + ASDR_STATE_OFF_ALS_X / 16 + lane, vF);
  if (h == 0) st_nt(rec + ASDR_STATE_OFF_AUDIO_PREV / 16 + l, vG);
  else if (ctl && l < ASDR_STATE_OFF_SMALL / 16) st_nt(rec + l, vG);
}

// A record without ASDR_STATE_HAS_SIGNAL is skipped (the host has set the channel's reset bits instead).
extern "C" __global__ __launch_bounds__(256) void asdr_state_scatter_kernel(UpdateArgs a, const int2 *list, int n, int ch0, int rec0,
                                                                            const u32x4 *records) {
  Entry en;
  if (!wave_entry(list, n, ch0, rec0, en)) return;
  const int lane = (int)(threadIdx.x & 63u), h = lane >> 5, l = lane & 31;
  const size_t ch = (size_t)en.ch;
  const u32x4 *rec = records + (size_t)en.rec * (ASDR_STATE_RECORD_BYTES / 16);
  const uint32_t content = reinterpret_cast<const uint32_t *>(rec)[3];   // (one word per record)
  if (!(content & ASDR_STATE_HAS_SIGNAL)) return;
  u32x4 *small = reinterpret_cast<u32x4 *>(a.small + ch);
  u32x4 *nbh = reinterpret_cast<u32x4 *>(a.nb_hist + ch * 768);
  const uint32_t p3 = a.nb_phase % 3u, p2 = a.als_phase & 1u;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  u32x4 vA = zero, vA2 = zero, vB, vC, vD, vE, vF, vG = zero;
  const bool a_row = (h == 0), a_mask = (h == 1 && l < ASDR_NB_MASK_ROW / 16);   // a_row: lane l makes piece l of the 32-piece row
  const bool keep_prev = (content & ASDR_STATE_HAS_AUDIO_PREV) != 0u;
  // ---- loads
  if (a_row && l < 26) vA = ld_nt(rec + ASDR_STATE_OFF_SMALL / 16 + rec_piece(l));
  if (a_row && rec_piece2(l) >= 0) vA2 = ld_nt(rec + ASDR_STATE_OFF_SMALL / 16 + rec_piece2(l));
  if (a_mask) vA = ld_nt(rec + ASDR_STATE_OFF_NB_MASK / 16 + l);
  vB = ld_nt(rec + ASDR_STATE_OFF_NB_HIST / 16 + lane);
  vC = ld_nt(rec + (h == 0 ? ASDR_STATE_OFF_NB_HIST / 16 + 64 : ASDR_STATE_OFF_ALS_W / 16) + l);
  vD = ld_nt(rec + ASDR_STATE_OFF_HIL_Q / 16 + lane);
  vE = ld_nt(rec + ASDR_STATE_OFF_HIL_I / 16 + lane);
  vF = ld_nt(rec + ASDR_STATE_OFF_ALS_X / 16 + lane);
  if (h == 0 && keep_prev) vG = ld_nt(rec + ASDR_STATE_OFF_AUDIO_PREV / 16 + l);
  // ---- ChanSmall's tail for THIS batch's ring position: the gains rotate back, the Hilbert parity is 0 (rows stored in canonical order)
  if (a_row) {
    if (l == 13) vA.w = 0u;                             // (agc_gain, agc_old_abs, agc_hang_counter | nb_slot_unused; the record has pll_y_re there)
    else if (l == 14) { u32x4 o = vA2; rotate_gains(vA, o, (3u - p3) % 3u); }
    else if (l == 15) { u32x4 o = vA2; rotate_gains(o, vA, (3u - p3) % 3u); }   // (.w = hil_slot = 0)
    else if (l == 25) { vA.z = vA2.w; vA.w = 0u; }      // (pll_phase_est, pll_freq | pll_y_re, padding)
    else if (l >= 26) vA = zero;
  }
  // ---- stores
  if (a_row) st(small + l, vA);
  if (a_mask) st(reinterpret_cast<u32x4 *>(a.nb_mask + ch * ASDR_NB_MASK_ROW) + l, vA);
  st(nbh + ((p3 + (uint32_t)h) % 3u) * 32u + l, vB);
  if (h == 0) st(nbh + ((p3 + 2u) % 3u) * 32u + l, vC); else st(reinterpret_cast<u32x4 *>(a.als_w + ch * 128) + l, vC);
  st(reinterpret_cast<u32x4 *>(a.hil_q + ch * 256) + lane, vD);
  st(reinterpret_cast<u32x4 *>(a.hil_i + ch * 256) + lane, vE);
  st(reinterpret_cast<u32x4 *>(a.als_x + ch * 256) + (((uint32_t)h ^ p2 ^ 1u) * 32u + l), vF);
  if (h == 0 && a.audio_prev) st(reinterpret_cast<u32x4 *>(a.audio_prev + ch * 128) + l, vG);
}

// One launch serves a list of any length (1 .. 1,048,576 entries: at most 262,144 workgroups).  The host has checked every index.
extern "C" int asdr_launch_state_gather(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, void *records, const void *ctl, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(asdr_state_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, *a, reinterpret_cast<const int2 *>(list), n, ch0, rec0,
                     reinterpret_cast<u32x4 *>(records), reinterpret_cast<const u32x4 *>(ctl));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asdr_launch_state_scatter(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, const void *records, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(asdr_state_scatter_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, *a, reinterpret_cast<const int2 *>(list), n, ch0, rec0,
                     reinterpret_cast<const u32x4 *>(records));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
