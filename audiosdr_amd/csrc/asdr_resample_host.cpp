// asdr_resample_host.cpp -- host side + C ABI (include/asdr_resample.h) of the audio resampler.  The filter lives in a host copy
// (what the getters return) and, as the kernel's two pair tables, on the device; the state records live on the device only, in a
// double buffer whose halves a call reads and writes (an ASDR_NO_DEVICE resampler keeps them on the host instead).  The position
// N and everything a call derives from it (first output, first b, first phase, the tile's steps) is 64-bit host arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "asdr_resample_device.h"
#include "asdr_stage_host.h"

struct asdr_resampler : StageDev {
  int up = 1, down = 1, K = 1, shift = 15;
  std::vector<int16_t> taps;                   // h[k * up + phi]
  long long pos = 0;                           // N
  CarryPair carry;                             // the state records
  uint32_t *d_taps = nullptr;
};

namespace {
const char *kNoDevice = "control-plane-only resampler (ASDR_NO_DEVICE): the signal path needs a HIP device";
constexpr int kRecord = ASDR_RESAMPLE_STATE_SAMPLES;
constexpr long long kMaxN = 1LL << 53;   // N U stays below 2^63

// words per phase of a pair table: K / 2 + 1 pairs, zero filled to whole scalar loads
int pairs_of(int K) { return (K / 2 + 1 + ASDR_RESAMPLE_PAIR_BATCH - 1) / ASDR_RESAMPLE_PAIR_BATCH * ASDR_RESAMPLE_PAIR_BATCH; }
size_t tap_words(int up, int K) { return (size_t)2 * pairs_of(K) * up; }

long long gcd_ll(long long a, long long b) { while (b) { const long long t = a % b; a = b; b = t; } return a; }
long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
uint32_t magic(int d) { return (uint32_t)(((1ULL << 32) + (uint32_t)d - 1) / (uint32_t)d); }   // d >= 2

double bessel_i0(double x) {
  double s = 1.0, term = 1.0;
  for (int k = 1; k < 500; k++) {
    const double f = x / (2.0 * k);
    term *= f * f;
    s += term;
    if (term < 1e-17 * s) break;
  }
  return s;
}

int check_rate(int up, int down) {
  if (up < 1 || up > ASDR_RESAMPLE_MAX_UP) return fail("resampler: U must be in 1..512");
  if (down < up) return fail("resampler: interpolation (U > M) is not supported");
  if (down > ASDR_RESAMPLE_MAX_RATIO * up) return fail("resampler: M must not exceed 16 U");
  return 0;
}

int check_filter(int up, int K, const int16_t *taps, int shift) {
  if (K < 1 || K > ASDR_RESAMPLE_MAX_TAPS) return fail("resampler: taps per phase must be in 1..256");
  if (!taps) return fail("null taps");
  if (shift < 0 || shift > 15) return fail("resampler: shift must be in 0..15");
  for (int ph = 0; ph < up; ph++) {
    long sum = 0;
    for (int k = 0; k < K; k++) sum += std::abs((int)taps[(size_t)k * up + ph]);
    if (sum > ASDR_RESAMPLE_MAX_ABS_SUM)
      return fail("resampler: phase " + std::to_string(ph) + " has sum |h| = " + std::to_string(sum) + " > 65535");
  }
  return 0;
}

// the default filter of include/asdr_resample.h
void design(int up, int fs_out, std::vector<int16_t> &h, int &K) {
  const double pi = 3.14159265358979323846;
  const double fs_hi = (double)up * ASDR_RESAMPLE_FS_IN;
  const double dw = 2.0 * pi * 0.16 * fs_out / fs_hi;
  K = 2 * (int)std::ceil((80.0 - 7.95) / (2.285 * dw) / (2.0 * up));
  const int L = up * K;
  const double fc = 0.5 * fs_out / fs_hi, beta = 0.1102 * (80.0 - 8.7), i0b = bessel_i0(beta);
  std::vector<double> w(L);
  for (int i = 0; i < L; i++) {
    const double x = 2.0 * fc * (i - 0.5 * (L - 1)), u = 2.0 * i / (L - 1) - 1.0;
    const double sinc = x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x);
    w[i] = 2.0 * fc * sinc * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
  }
  h.assign(L, 0);
  for (int ph = 0; ph < up; ph++) {
    double sum = 0.0;
    for (int k = 0; k < K; k++) sum += w[(size_t)k * up + ph];
    long tot = 0;
    int big = 0;
    std::vector<long> q(K);
    for (int k = 0; k < K; k++) {
      q[k] = std::lround(32768.0 * w[(size_t)k * up + ph] / sum);
      tot += q[k];
      if (std::labs(q[k]) > std::labs(q[big])) big = k;
    }
    q[big] += 32768 - tot;                                      // the phase sums to 32768 exactly
    for (int k = 0; k < K; k++) h[(size_t)k * up + ph] = (int16_t)q[k];
  }
}

// the kernel's pair tables (asdr_resample.hip): [table][phase][k], low half = the tap of the word's first (even) sample
void pair_tables(const asdr_resampler_t *r, std::vector<uint32_t> &t) {
  const int P = pairs_of(r->K), U = r->up;
  auto h = [&](int k, int ph) -> uint32_t { return (k < 0 || k >= r->K) ? 0u : (uint32_t)(uint16_t)r->taps[(size_t)k * U + ph]; };
  t.assign(tap_words(U, r->K), 0u);
  for (int k = 0; k < P; k++)
    for (int ph = 0; ph < U; ph++) {
      t[((size_t)0 * U + ph) * P + k] = h(2 * k + 1, ph) | (h(2 * k, ph) << 16);       // odd b:  x[b - 2k - 1], x[b - 2k]
      t[((size_t)1 * U + ph) * P + k] = h(2 * k, ph) | (h(2 * k - 1, ph) << 16);       // even b: x[b - 2k], x[b - 2k + 1]
    }
}

int push_filter(asdr_resampler_t *r) {
  std::vector<uint32_t> t;
  pair_tables(r, t);
  HIPCHK(hipMemcpy(r->d_taps, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  return 0;
}

asdr_resampler_t *make(int n_channels, int up, int down, int K, const int16_t *taps, int shift, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  if (check_rate(up, down) != 0 || check_filter(up, K, taps, shift) != 0) return nullptr;
  asdr_resampler *r = new asdr_resampler;
  r->n = n_channels; r->up = up; r->down = down; r->K = K; r->shift = shift;
  r->taps.assign(taps, taps + (size_t)up * K);
  r->carry.samples = kRecord;
  if (device == ASDR_NO_DEVICE) {
    r->carry.reset(*r);
    return r;
  }
  const size_t rec = (size_t)n_channels * kRecord * sizeof(int16_t);
  if (stage_open(*r, device, "resampler") != 0) { asdr_resampler_destroy(r); return nullptr; }
  if (hipMalloc(&r->carry.d[0], rec) != hipSuccess || hipMalloc(&r->carry.d[1], rec) != hipSuccess ||
      hipMalloc(&r->d_taps, tap_words(up, ASDR_RESAMPLE_MAX_TAPS) * sizeof(uint32_t)) != hipSuccess ||
      hipMemset(r->carry.d[0], 0, rec) != hipSuccess || hipMemset(r->carry.d[1], 0, rec) != hipSuccess ||
      push_filter(r) != 0 || hipDeviceSynchronize() != hipSuccess) {
    fail("resampler: device allocation failed");
    asdr_resampler_destroy(r);
    return nullptr;
  }
  return r;
}
}  // namespace

extern "C" {

asdr_resampler_t *asdr_resampler_create(int n_channels, int fs_out, int device) {
  if (fs_out <= 0 || fs_out > ASDR_RESAMPLE_FS_IN) {
    fail(fs_out <= 0 ? "resampler: Fs_out must be positive" : "resampler: interpolation (U > M) is not supported");
    return nullptr;
  }
  const long long g = gcd_ll(fs_out, ASDR_RESAMPLE_FS_IN);
  const long long up = fs_out / g, down = ASDR_RESAMPLE_FS_IN / g;
  if (up > ASDR_RESAMPLE_MAX_UP) { fail("resampler: U must be in 1..512"); return nullptr; }
  if (check_rate((int)up, (int)down) != 0) return nullptr;
  if (up == 1 && down == 1) {                                   // the identity: (16384 x + 8192) >> 14 = x
    const int16_t one = 16384;
    return make(n_channels, 1, 1, 1, &one, 14, device);
  }
  std::vector<int16_t> h;
  int K = 1;
  design((int)up, fs_out, h, K);
  if (K >ASDR_RESAMPLE_MAX_TAPS) { fail("resampler: the default filter of this rate needs more than 256 taps per phase"); return nullptr; }
  return make(n_channels, (int)up, (int)down, K, h.data(), 15, device);
}

asdr_resampler_t *asdr_resampler_create_custom(int n_channels, int up, int down, int taps_per_phase, const int16_t *taps, int shift, int device) {
  return make(n_channels, up, down, taps_per_phase, taps, shift, device);
}

void asdr_resampler_destroy(asdr_resampler_t *r) {
  if (!r) return;
  stage_close(*r, {r->carry.d[0], r->carry.d[1], r->d_taps});
  delete r;
}

int asdr_resampler_n_channels(const asdr_resampler_t *r) { return r ? r->n : fail("null resampler"); }
int asdr_resampler_up(const asdr_resampler_t *r) { return r ? r->up : fail("null resampler"); }
int asdr_resampler_down(const asdr_resampler_t *r) { return r ? r->down : fail("null resampler"); }
int asdr_resampler_taps_per_phase(const asdr_resampler_t *r) { return r ? r->K : fail("null resampler"); }

int asdr_resampler_get_taps(const asdr_resampler_t *r, int16_t *taps, int *shift) {
  if (!r) return fail("null resampler");
  if (taps) std::memcpy(taps, r->taps.data(), r->taps.size() * sizeof(int16_t));
  if (shift) *shift = r->shift;
  return 0;
}

double asdr_resampler_delay(const asdr_resampler_t *r) {
  if (!r) { fail("null resampler"); return std::numeric_limits<double>::quiet_NaN(); }
  return ((double)r->up * r->K - 1.0) / (2.0 * r->up);
}

int asdr_resampler_set_filter(asdr_resampler_t *r, int taps_per_phase, const int16_t *taps, int shift) {
  if (!r) return fail("null resampler");
  if (check_filter(r->up, taps_per_phase, taps, shift) != 0) return -1;
  if (stage_quiesce(*r) != 0) return -1;
  r->K = taps_per_phase; r->shift = shift;
  r->taps.assign(taps, taps + (size_t)r->up * taps_per_phase);
  return r->device == ASDR_NO_DEVICE ? 0 : push_filter(r);
}

long long asdr_resampler_position(const asdr_resampler_t *r) { return r ? r->pos : (long long)fail("null resampler"); }

long long asdr_resampler_output_position(const asdr_resampler_t *r) {
  return r ? ceil_div(r->pos * r->up, r->down) : (long long)fail("null resampler");
}

long asdr_resampler_out_samples(const asdr_resampler_t *r, int n_blocks) {
  if (!r) return fail("null resampler");
  if (n_blocks < 0 || n_blocks > 65535) return fail("n_blocks must be in 0..65535");
  const long long n1 = r->pos + 128LL * n_blocks;
  if (n1 > kMaxN) return fail("resampler: position past 2^53");
  return (long)(ceil_div(n1 * r->up, r->down) - ceil_div(r->pos * r->up, r->down));
}

int asdr_resampler_set_position(asdr_resampler_t *r, long long n) {
  if (!r) return fail("null resampler");
  if (n < 0 || n > ASDR_RESAMPLE_MAX_POSITION) return fail("resampler: position must be in 0..2^50");
  if (stage_quiesce(*r) != 0) return -1;
  r->pos = n;
  return 0;
}

long asdr_resampler_update_device(asdr_resampler_t *r, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dOut,
                                  long out_stride_samples, const int32_t *dIndex, const int32_t *dCount, int capacity_rows, void *stream_) {
  if (!r) return fail("null resampler");
  if (r->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!dAudio || !dOut) return fail("null device pointer");
  if (n_blocks < 0 || n_blocks > 65535) return fail("n_blocks must be in 0..65535");
  if (stride_blocks < n_blocks) return fail("row stride shorter than n_blocks");
  if (stride_blocks > (1L << 30)) return fail("row stride too large");
  if (((uintptr_t)dAudio & 15u) != 0) return fail("the audio rows must be 16-byte aligned");
  if (((uintptr_t)dOut & 1u) != 0) return fail("the output rows must be 2-byte aligned");
  if (dIndex && !dCount) return fail("an index needs a count");
  if (dIndex && capacity_rows < 0) return fail("capacity_rows is negative");
  if (n_blocks == 0) return 0;
  const long long n0 = r->pos, n1 = n0 + 128LL * n_blocks;
  if (n1 > kMaxN) return fail("resampler: position past 2^53");
  const long long U = r->up, M = r->down;
  const long long j0 = ceil_div(n0 * U, M), j1 = ceil_div(n1 * U, M);
  const long long n_out = j1 - j0;                              // >= 8 n_blocks: M <= 16 U
  if (out_stride_samples < n_out) return fail("output row stride shorter than the call's output count");
  if (out_stride_samples > (1L << 40)) return fail("output row stride too large");
  const int grid_rows = dIndex ? std::min(capacity_rows, r->n) : r->n;
  if (grid_rows > 0) {
    const size_t audio_bytes = ((size_t)(r->n - 1) * stride_blocks + n_blocks) * 256;
    const size_t out_bytes = ((size_t)(grid_rows - 1) * out_stride_samples + n_out) * 2;
    if (overlap((uintptr_t)dAudio, audio_bytes, (uintptr_t)dOut, out_bytes)) return fail("output span overlaps the audio span");
  }

  ResampleArgs a;
  a.audio = dAudio; a.stride_blocks = stride_blocks;
  a.carry = r->carry.current(); a.carry_next = r->carry.next();
  a.out = dOut; a.out_stride = out_stride_samples;
  a.index = dIndex; a.count = dCount;
  a.taps = r->d_taps;
  a.n_channels = r->n; a.n_blocks = n_blocks; a.grid_rows = grid_rows; a.capacity_rows = dIndex ? capacity_rows : r->n;
  a.up = r->up; a.pairs = pairs_of(r->K); a.shift = r->shift; a.round = r->shift ? 1 << (r->shift - 1) : 0;
  a.n_out = (int32_t)n_out;
  a.phi0 = (int32_t)(j0 * M % U); a.lb0 = (int32_t)(j0 * M / U - n0);
  a.reach = 2 * a.pairs + 1;
  // The tile: as many outputs as keep 64 windows within the LDS budget.  A tile of w outputs starting in phase phi runs over
  // span = (phi + (w - 1) M) / U + 1 input samples (phi = U - 1 at worst), staged from up to 7 samples early and one sample past.
  const int max_pieces = (ASDR_RESAMPLE_MAX_LDS / (4 * ASDR_RESAMPLE_ROWS) - 1) / 4;
  const long long max_span = 8LL * max_pieces - a.reach - 15;
  const long long fit = 1 + ((max_span - 1) * U - (U - 1)) / M;
  if (max_span < 2 || fit < 1) return fail("internal: resampler window does not fit");
  a.tile_out = (int32_t)std::min<long long>(fit, n_out);
  const long long span = ((U - 1) + (long long)(a.tile_out - 1) * M) / U + 1;
  a.pieces = (int32_t)((a.reach + 8 + span + 7) / 8);
  a.pieces_magic = magic(a.pieces);
  a.row_words = 4 * a.pieces + 1;
  a.tile_q = (int32_t)((long long)a.tile_out * M / U); a.tile_r = (int32_t)((long long)a.tile_out * M % U);
  a.q1 = (int32_t)(M / U); a.r1 = (int32_t)(M % U); a.q4 = (int32_t)(4 * M / U); a.r4 = (int32_t)(4 * M % U);
  const long long tiles = ceil_div(n_out, a.tile_out), groups = ceil_div(std::max(grid_rows, 1), ASDR_RESAMPLE_ROWS);
  if (a.lb0 < 0 || a.lb0 > ASDR_RESAMPLE_MAX_RATIO || a.pieces < 2 || a.pieces > max_pieces ||
      (size_t)ASDR_RESAMPLE_ROWS * a.row_words * 4 > ASDR_RESAMPLE_MAX_LDS)
    return fail("internal: resampler launch geometry out of range");
  if (tiles >= (1LL << 22) || tiles * groups * ASDR_RESAMPLE_THREADS >= (1LL << 32))
    return fail("resampler: the call is too large for one launch; split it");

  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*r, stream) != 0) return -1;
  if (asdr_launch_resample(&a, stream) != 0) return fail("resampler kernel launch failed");
  if (asdr_launch_resample_carry(&a, stream) != 0) return fail("resampler carry kernel launch failed");
  if (stage_after_launch(*r, stream) != 0) return -1;
  r->carry.flip();
  r->pos = n1;
  return (long)n_out;
}

int asdr_resampler_read_state(asdr_resampler_t *r, int16_t *dst) {
  if (!r) return fail("null resampler");
  return r->carry.read(*r, dst);
}

int asdr_resampler_write_state(asdr_resampler_t *r, const int *channels, int n, const int16_t *src) {
  if (!r) return fail("null resampler");
  return r->carry.write(*r, channels, n, src);
}

int asdr_resampler_reset(asdr_resampler_t *r) {
  if (!r) return fail("null resampler");
  if (r->carry.reset(*r) != 0) return -1;
  r->pos = 0;
  return 0;
}

int asdr_resampler_synchronize(asdr_resampler_t *r) {
  if (!r) return fail("null resampler");
  return stage_quiesce(*r);
}

}  // extern "C"
