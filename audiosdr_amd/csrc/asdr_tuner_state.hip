// asdr_tuner_state.hip -- tuner channel records (include/asdr_tuner.h "State records"): the two copy kernels between a
// bank's per-channel device state (the stage-2 carry row and the level accumulator) and the canonical 2,560-byte channel records.
//
//   asdr_tuner_state_gather_kernel    carry rows, levels -> records   (asdr_tuner_export_channels*)
//   asdr_tuner_state_scatter_kernel   records -> carry rows, levels   (asdr_tuner_import_channels*)
//
// The design asdr_state.hip proved: ONE WAVE PER LIST ENTRY, four entries per workgroup, one launch for a list of any length.  A record's
// device part is 16 + 144 16-byte pieces: the 256-byte head and the 2,304-byte carry row.  A lane moves at most three pieces, ALL loads
// issued before the first store:
//   A  lanes 0..63: carry pieces 0..63      B  lanes 0..63: carry pieces 64..127
//   C  lanes 0..15: carry pieces 128..143   lanes 16..31: the head's pieces 0..15 (gather only: the host has filled them in a staging
//      area; the lane of piece 6 puts the channel's level accumulator into bytes 96..103)
// The carry row is linear in the bank (slot i = u sample N_u - 576 + i), so the canonical order is the bank's own and the double-buffer
// parity is the host's choice of pointer.  No lane exchanges data with another, no LDS, no scratch.  The one access that is not a 16-byte
// piece is the level: one aligned double per channel.
// The record side is read / written once per call: non-temporal.  The bank side is what the next update reads: plain.
#include <hip/hip_runtime.h>

#include "asdr_tuner_state.h"

namespace {

static_assert(ASDR_TUNER_CHANNEL_RECORD_BYTES == ASDR_TUNER_CHANNEL_OFF_CARRY + ASDR_TUNER_CARRY * 4 && ASDR_TUNER_CHANNEL_OFF_CARRY == 256 &&
              ASDR_TUNER_CHANNEL_OFF_LEVEL == 96 && ASDR_TUNER_CHANNEL_RECORD_BYTES % 256 == 0, "record layout");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kRecPieces = ASDR_TUNER_CHANNEL_RECORD_BYTES / 16;   // 160
constexpr int kHeadPieces = ASDR_TUNER_CHANNEL_OFF_CARRY / 16;     // 16
constexpr int kCarryPieces = ASDR_TUNER_CARRY * 4 / 16;            // 144
constexpr int kLevelPiece = ASDR_TUNER_CHANNEL_OFF_LEVEL / 16;     // 6: bytes 96..111, the level in its first two words

__device__ __forceinline__ u32x4 ld(const u32x4 *p) { return *p; }
__device__ __forceinline__ u32x4 ld_nt(const u32x4 *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ void st(u32x4 *p, u32x4 v) { *p = v; }
__device__ __forceinline__ void st_nt(u32x4 *p, u32x4 v) { __builtin_nontemporal_store(v, p); }

// The entry this wave works on.  list == nullptr: entry e is channel ch0 + e, record rec0 + e.
__device__ __forceinline__ bool wave_entry(const int2 *list, int n, int ch0, int rec0, int &e, int &ch, int &rec) {
  e = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
  if (e >= n) return false;
  if (list) { const int2 v = list[e]; ch = __builtin_amdgcn_readfirstlane(v.x); rec = __builtin_amdgcn_readfirstlane(v.y); }
  else { ch = ch0 + e; rec = rec0 + e; }
  return true;
}

}  // namespace

// `head`: [n][16] pieces, the head of entry e as the host wrote it (level 0).  a.carry == nullptr: the carry section is zeros (a
// pass-through stage 2, or a carry that is logically zero); a.level == nullptr: the level stays 0.
extern "C" __global__ __launch_bounds__(256) void asdr_tuner_state_gather_kernel(TunerStateArgs a, const int2 *list, int n, int ch0, int rec0,
                                                                                 u32x4 *records, const u32x4 *head) {
  int e, ch, r;
  if (!wave_entry(list, n, ch0, rec0, e, ch, r)) return;
  const int lane = (int)(threadIdx.x & 63u);
  u32x4 *rec = records + (size_t)r * kRecPieces;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const bool c_carry = lane < kCarryPieces - 128, c_head = lane >= 16 && lane < 16 + kHeadPieces;
  u32x4 vA = zero, vB = zero, vC = zero;
  u32x2 lev = {0u, 0u};
  // ---- loads
  if (a.carry) {
    const u32x4 *row = reinterpret_cast<const u32x4 *>(a.carry) + (size_t)ch * kCarryPieces;
    vA = ld(row + lane);
    vB = ld(row + 64 + lane);
    if (c_carry) vC = ld(row + 128 + lane);
  }
  if (c_head && head) vC = ld_nt(head + (size_t)e * kHeadPieces + (lane - 16));
  if (lane == 16 + kLevelPiece && a.level) lev = *reinterpret_cast<const u32x2 *>(a.level + ch);
  if (lane == 16 + kLevelPiece) { vC.x = lev.x; vC.y = lev.y; }
  // ---- stores
  st_nt(rec + kHeadPieces + lane, vA);
  st_nt(rec + kHeadPieces + 64 + lane, vB);
  if (c_carry) st_nt(rec + kHeadPieces + 128 + lane, vC);
  if (c_head) st_nt(rec + (lane - 16), vC);
}

// The host has checked every record's head.  A record without ASDR_TUNER_REC_HAS_CARRY gives the channel a zero carry, one without
// ASDR_TUNER_REC_HAS_LEVEL a zero level.  a.carry == nullptr (a pass-through destination): the carry section is ignored; a.level ==
// nullptr (levels off): the level is.
extern "C" __global__ __launch_bounds__(256) void asdr_tuner_state_scatter_kernel(TunerStateArgs a, const int2 *list, int n, int ch0, int rec0,
                                                                                  const u32x4 *records) {
  int e, ch, r;
  if (!wave_entry(list, n, ch0, rec0, e, ch, r)) return;
  const int lane = (int)(threadIdx.x & 63u);
  const u32x4 *rec = records + (size_t)r * kRecPieces;
  const uint32_t content = reinterpret_cast<const uint32_t *>(rec)[3];   // (one word per record)
  const bool has_carry = (content & ASDR_TUNER_REC_HAS_CARRY) != 0u, has_level = (content & ASDR_TUNER_REC_HAS_LEVEL) != 0u;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const bool c_carry = lane < kCarryPieces - 128, c_level = lane == 16 + kLevelPiece && a.level != nullptr;
  u32x4 vA = zero, vB = zero, vC = zero;
  // ---- loads
  if (a.carry && has_carry) {
    vA = ld_nt(rec + kHeadPieces + lane);
    vB = ld_nt(rec + kHeadPieces + 64 + lane);
    if (c_carry) vC = ld_nt(rec + kHeadPieces + 128 + lane);
  }
  if (c_level && has_level) vC = ld_nt(rec + kLevelPiece);
  // ---- stores
  if (a.carry) {
    u32x4 *row = reinterpret_cast<u32x4 *>(a.carry) + (size_t)ch * kCarryPieces;
    st(row + lane, vA);
    st(row + 64 + lane, vB);
    if (c_carry) st(row + 128 + lane, vC);
  }
  if (c_level) { const u32x2 lev = {vC.x, vC.y}; *reinterpret_cast<u32x2 *>(a.level + ch) = lev; }
}

// One launch serves a list of any length (1 .. 1,048,576 entries: at most 262,144 workgroups).  The host has checked every index.
extern "C" int asdr_launch_tuner_state_gather(const TunerStateArgs *a, const int *list, int n, int ch0, int rec0, void *records, const void *head,
                                              void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(asdr_tuner_state_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *a,
                     reinterpret_cast<const int2 *>(list), n, ch0, rec0, reinterpret_cast<u32x4 *>(records), reinterpret_cast<const u32x4 *>(head));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int asdr_launch_tuner_state_scatter(const TunerStateArgs *a, const int *list, int n, int ch0, int rec0, const void *records, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(asdr_tuner_state_scatter_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, *a,
                     reinterpret_cast<const int2 *>(list), n, ch0, rec0, reinterpret_cast<const u32x4 *>(records));
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
