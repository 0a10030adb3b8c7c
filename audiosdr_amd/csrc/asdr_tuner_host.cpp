// asdr_tuner_host.cpp -- host side + C ABI (include/asdr_tuner.h) of the digital tuner bank.  The control plane lives in a host
// mirror (channel anchors, the source-sorted schedule, the polyphase taps) that is pushed before a launch when a setter touched it;
// the per-source history rows live on the device only, double-buffered so that the launch that reads one writes the other.
// Fast-convolution banks share all of it; their stage 1 (asdr_tuner_fastconv.hip) adds the channel filter's response G and the
// twiddle tables, pushed the same way, and keeps H samples per source in the history rows.  A bank with a channel off slot 0 or
// gain 1 also pushes the palette's table and the channels' slots and gains, and runs asdr_tuner_palette.hip's channel step.
// Source conditioning (asdr_tuner_condition.hip) is a pre-pass of run_stage1: a bank with a correction off the identity reads its
// stage-1 input from a scratch of corrected CS16 / RS16 rows instead of the caller's; one with the statistics on also sums there.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "asdr_stage_host.h"
#include "asdr_tuner_device.h"
#include "asdr_tuner_state.h"

namespace {
const char *kFormatNames[] = {"CS16", "CU8", "CS8", "CF32", "RS16"};
const char *kNoDevice = "control-plane-only tuner bank (ASDR_NO_DEVICE): the signal path needs a HIP device";
constexpr int kTapWords = 1088;   // >= ceil(L / D) * ceil(D / 2) for every D <= 64, L <= 1024 (the largest is 1024, D = 1)

double bessel_i0(double x) {
  double s = 1.0, term = 1.0;
  for (int k = 1; k < 200; k++) {
    const double f = x / (2.0 * k);
    term *= f * f;
    s += term;
    if (term < 1e-17 * s) break;
  }
  return s;
}

// Kaiser-windowed (beta 9 unless given) sinc of L taps with cut-off fc (cycles per sample); returns the sum of the taps.
double kaiser_sinc(int L, double fc, std::vector<double> &w, double beta = 9.0) {
  const int M = L - 1;
  const double pi = 3.14159265358979323846;
  w.assign(L, 0.0);
  double sum = 0.0;
  for (int n = 0; n < L; n++) {
    const double x = n - 0.5 * M, u = 2.0 * n / M - 1.0;
    const double s = (x == 0.0) ? 2.0 * fc : std::sin(2.0 * pi * fc * x) / (pi * x);
    w[n] = s * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / bessel_i0(beta);
    sum += w[n];
  }
  return sum;
}

// The default filter (asdr_tuner.h): D = 1 -> {16384}, g = 1; D >= 2 -> a Kaiser-windowed sinc of 12 D + 1 taps (beta 9, cut-off
// midway between 11.2 kHz and 32.1 kHz), normalised to unit DC gain and rounded to Q15, g = 0.  Its measured response: DESIGN.md 3.8.
void default_filter(int D, std::vector<int16_t> &h, int &g) {
  if (D == 1) { h.assign(1, 16384); g = 1; return; }
  const int L = 12 * D + 1;
  std::vector<double> w;
  const double sum = kaiser_sinc(L, 0.5 * (11200.0 + 32100.0) / (44100.0 * D), w);
  h.resize(L);
  for (int n = 0; n < L; n++) h[n] = (int16_t)std::llround(32768.0 * w[n] / sum);
  g = 0;
}

// A rate bank's stage-1 default (asdr_tuner.h): the plain default at Fs_mid = 44100, else stop band from Fs_mid - 12 kHz, cut-off
// midway between 11.2 kHz and that edge, L1 = 2 ceil(6 D Fs_mid 20900 / (44100 (Fs_mid - 23200))) + 1 taps.
void default_rate_filter(int D, long long fs_mid, std::vector<int16_t> &h, int &g) {
  if (fs_mid == 44100 || D == 1) { default_filter(D, h, g); return; }
  const long long num = 6LL * D * fs_mid * 20900, den = 44100LL * (fs_mid - 23200);
  const int L = (int)(2 * ((num + den - 1) / den) + 1);
  std::vector<double> w;
  const double sum = kaiser_sinc(L, 0.5 * (11200.0 + (double)(fs_mid - 12000)) / (double)(fs_mid * D), w);
  h.resize(L);
  for (int n = 0; n < L; n++) h[n] = (int16_t)std::llround(32768.0 * w[n] / sum);
  g = 0;
}

// Stage-2 default: U = M = 1 -> {16384}, g2 = 1; otherwise a prototype of U K taps at U Fs_mid, cut-off 21.65 kHz,
// K = 2 ceil(6 Fs_mid / 44100); each phase rounded to Q15 on its own, the residual to 32768 put on its largest tap; g2 = 0.
// (K and the cut-off in cycles per sample at U Fs_mid are given: resampler_taps.)
void resampler_taps(int U, int K, double fc, std::vector<int16_t> &h2, int &g2);
void default_resampler(int U, int M, long long fs_mid, std::vector<int16_t> &h2, int &g2) {
  if (U == 1 && M == 1) { h2.assign(1, 16384); g2 = 1; return; }
  resampler_taps(U, (int)(2 * ((6 * fs_mid + 44099) / 44100)), 21650.0 / ((double)U * (double)fs_mid), h2, g2);
}

// The same rule at a fast-convolution bank's Fs_mid = Fs_in / R, which may be fractional: K = 2 ceil(6 Fs_in / (44100 R)),
// cut-off 21650 R / (U Fs_in).
void default_fastconv_resampler(int U, int M, long long fs_in, int R, std::vector<int16_t> &h2, int &g2) {
  if (U == 1 && M == 1) { h2.assign(1, 16384); g2 = 1; return; }
  const long long d = 44100LL * R;
  resampler_taps(U, (int)(2 * ((6 * fs_in + d - 1) / d)), 21650.0 * R / ((double)U * (double)fs_in), h2, g2);
}

void resampler_taps(int U, int K, double fc, std::vector<int16_t> &h2, int &g2) {
  const int L = U * K;
  std::vector<double> w;
  const double sum = kaiser_sinc(L, fc, w);
  h2.assign(L, 0);
  for (int ph = 0; ph < U; ph++) {
    long long tot = 0;
    int big = ph;
    for (int k = 0; k < K; k++) {
      const int i = k * U + ph;
      h2[i] = (int16_t)std::llround(32768.0 * U * w[i] / sum);
      tot += h2[i];
      if (h2[i] > h2[big]) big = i;
    }
    h2[big] = (int16_t)(h2[big] + (32768 - tot));
  }
  g2 = 0;
}

long long gcd_ll(long long a, long long b) { while (b) { const long long r = a % b; a = b; b = r; } return a; }

// The fast-convolution default channel filter (asdr_tuner.h): Kaiser (beta 7.857) windowed sinc of 129 taps at Fs_mid, cut-off
// 11.5 kHz + delta / 2 with delta = 0.0392 Fs_mid, normalised to sum 1, rounded to float.
void default_channel_filter(double fs_mid, std::vector<float> &g) {
  std::vector<double> w;
  const double sum = kaiser_sinc(ASDR_TUNER_FC_MAX_TAPS, (11500.0 + 0.5 * 0.0392 * fs_mid) / fs_mid, w, 7.857);
  g.resize(ASDR_TUNER_FC_MAX_TAPS);
  for (int n = 0; n < ASDR_TUNER_FC_MAX_TAPS; n++) g[n] = (float)(w[n] / sum);
}

// U K taps and g2 passing the set_resampler rules for a bank with up-factor U
std::string resampler_error(int U, const int16_t *h2, int n_taps, int g2) {
  if (!h2) return "null taps";
  if (n_taps < U || n_taps % U != 0) return "resampler length must be a multiple of U";
  if (n_taps / U > ASDR_TUNER_MAX_RESAMPLER_TAPS) return "resampler taps per phase (K) must be in 1..64";
  if (g2 < 0 || g2 > ASDR_TUNER_MAX_GAIN_SHIFT) return "gain shift must be in 0..15";
  for (int ph = 0; ph < U; ph++) {
    long sum = 0;
    for (int i = ph; i < n_taps; i += U) sum += std::labs((long)h2[i]);
    if (sum > 65535) return "a resampler phase has sum of |h2| over 65535";
  }
  return "";
}
}  // namespace

struct asdr_tuner_bank : StageDev {
  int n_src = 0, D = 1;
  int fmt = ASDR_TUNER_IN_CS16;       // input format of the next call's rows
  long long pos = 0;
  // rate bank (stage 2): Fs_in, U / M, the prototype [U K] and g2, output samples written
  long long fs_in = 44100;
  int up = 1, down = 1, k2 = 1, g2 = 1;
  std::vector<int16_t> h2;
  long long out_pos = 0;
  bool rs_dirty = true, carry_stale = false;
  std::vector<asdr_tuner_state_t> chan;
  std::vector<int32_t> order;
  std::vector<int16_t> h;
  int g = 0;
  bool chan_dirty = true, order_dirty = true, taps_dirty = true;
  // fast-convolution bank: D = R, N = 256 R = 2^log2n, the channel filter g (float) whose response G is pushed, hist_slots = H
  bool fc = false;
  int log2n = 0, hist_slots = ASDR_TUNER_HIST_SLOTS;
  std::vector<float> gch;
  bool g_dirty = true;
  float *d_fc_tab = nullptr;          // [N] W_N, [256] W_256, [256] G (float pairs)
  // palette and gain (include/asdr_tuner.h, "Filter palette and gain"): slots 1 .. 63 (slot 0 is gch), every channel's slot and
  // gain in channel order, and how many channels are off (slot 0, gain 1): none -> the bank launches as a bank without a palette.
  // The device side is allocated by the first call that needs it; pal_dirty has a bit per slot whose row awaits its upload
  // (bit 0: set with g_dirty), sg_dirty says the same of the slot and gain arrays.
  struct PaletteSlot { std::vector<float> taps; bool cx = false; int n = 0; };   // n = Lg, 0 = undefined
  std::vector<PaletteSlot> pal;
  std::vector<int32_t> slot;
  std::vector<float> gain;
  int n_off = 0;
  uint64_t pal_dirty = 1;
  bool sg_dirty = true;
  float *d_pal_tab = nullptr;         // [64][256] float pairs
  int32_t *d_slot = nullptr;
  float *d_gain = nullptr;
  float *d_fc_x = nullptr;            // X, then the four-step scratch: [2][n_sources][n_frames][N] float pairs
  size_t fc_x_cap = 0;
  // monitors (fast-convolution banks; include/asdr_tuner.h, "Monitors"): spectrum [n_sources][B] and its frame count; levels
  // [n_channels], their count and the call's partials [n_frames][n_channels]
  int spec_bins = 0, spec_win = ASDR_TUNER_WIN_HANN, spec_mode = ASDR_TUNER_MON_SUM;
  long long spec_frames = 0;
  double *d_spec = nullptr;
  bool lev_on = false;
  long long lev_frames = 0;
  double *d_lev = nullptr;
  float *d_lev_part = nullptr;
  size_t lev_part_cap = 0;
  // source conditioning (include/asdr_tuner.h, "Source conditioning"): every source's correction and how many are off the identity
  // (none, with the statistics off: no pre-pass, nothing allocated); the device copy awaits its upload while corr_dirty; the
  // scratch of corrected rows [n_sources][the call's samples] grows as d_fc_x does; the statistics [n_sources][7] exist while on
  std::vector<asdr_tuner_iq_t> corr;
  int n_cond = 0;
  bool corr_dirty = true, iq_stats_on = false;
  long long cond_launches = 0;
  int32_t *d_corr = nullptr;
  void *d_cond = nullptr;
  size_t cond_cap = 0;
  unsigned long long *d_iq_stats = nullptr;
  // device
  asdr_tuner_state_t *d_chan = nullptr;
  int32_t *d_order = nullptr, *d_taps = nullptr, *d_hist[2] = {nullptr, nullptr};
  int cur = 0;                        // d_hist[cur] holds the samples before pos
  int n_rows = 1, n_pairs = 1;        // A, DP2 of the pushed taps
  void *d_io = nullptr;               // staging for the host-pointer entry points
  size_t io_cap = 0;
  // stage 2: taps [U][KP] + the lane table, the carry rows (double-buffered, allocated by the first stage-2 call), the intermediate
  int16_t *d_rs_taps = nullptr;
  int32_t *d_lane_qr = nullptr, *d_carry[2] = {nullptr, nullptr};
  int ccur = 0;                       // d_carry[ccur] holds the u samples before N_u
  int kp = 8;
  int16_t *d_mid = nullptr;           // [2][n][n_frames * 128]
  size_t mid_cap = 0;
  // state records (include/asdr_tuner.h, "State records"; the end of this file): pinned and device staging, allocated at first use;
  // st_ev is recorded behind the last asynchronous use of the pinned half
  uint8_t *st_h = nullptr, *st_d = nullptr;
  size_t st_h_cap = 0, st_d_cap = 0;
  hipEvent_t st_ev = nullptr;
  bool st_ev_pending = false;
};

namespace {
asdr_tuner_t *open_device(asdr_tuner_bank *t, int device);

asdr_tuner_state_t fresh_state() {
  asdr_tuner_state_t s;
  memset(&s, 0, sizeof s);
  return s;
}
uint32_t theta_at(const asdr_tuner_state_t &s, long long pos) { return s.ph_a + (uint32_t)(uint64_t)(pos - s.pos_a) * s.fw; }

// fast-convolution banks: coarse bin k0 = floor(((int32) fw + q / 2) / q) and residual rw = fw - k0 q, q = 2^32 / N
int coarse_bin(uint32_t fw, int log2n) {
  const int lq = 32 - log2n;
  return (int)(((int64_t)(int32_t)fw + (1LL << (lq - 1))) >> lq);
}
uint32_t residual(uint32_t fw, int log2n) { return fw - ((uint32_t)coarse_bin(fw, log2n) << (32 - log2n)); }
// the fine NCO's phase at pos
uint32_t fine_theta_at(const asdr_tuner_state_t &s, long long pos, int log2n) {
  return s.ph_a + (uint32_t)(uint64_t)(pos - s.pos_a) * residual(s.fw, log2n);
}

// one retune of channel `ch` (or every channel): re-anchor at P with a continuous phase, then apply f
template <typename F>
int retune(asdr_tuner_t *t, int ch, F f) {
  if (!t) return fail("null tuner bank");
  if (ch != ASDR_ALL && (ch < 0 || ch >= t->n)) return fail("bad channel");
  for (int i = (ch == ASDR_ALL ? 0 : ch); i < (ch == ASDR_ALL ? t->n : ch + 1); i++) {
    asdr_tuner_state_t &s = t->chan[i];
    s.ph_a = t->fc ? fine_theta_at(s, t->pos, t->log2n) : theta_at(s, t->pos);
    s.pos_a = t->pos;
    f(s);
  }
  t->chan_dirty = true;
  if (t->fc) t->order_dirty = true;   // sorted by (source, k0)
  return 0;
}

// G[m] = sum_n g[n] e^{-j 2 pi m n / 256} in float64, at m' = m mod 256, each part rounded to float; g real [n] or complex [n][2]
void response(const float *g, int n_taps, bool cx, float *G) {
  const double pi = 3.14159265358979323846;
  for (int mp = 0; mp < 256; mp++) {
    const int m = mp < 128 ? mp : mp - 256;
    double re = 0.0, im = 0.0;
    for (int n = 0; n < n_taps; n++) {
      const double a = 2.0 * pi * (double)(((m * n) % 256 + 256) % 256) / 256.0;
      if (cx) {   // (gr + j gi) (cos a - j sin a)
        re += (double)g[2 * n] * std::cos(a) + (double)g[2 * n + 1] * std::sin(a);
        im += (double)g[2 * n + 1] * std::cos(a) - (double)g[2 * n] * std::sin(a);
      } else {
        re += (double)g[n] * std::cos(a);
        im -= (double)g[n] * std::sin(a);
      }
    }
    G[2 * mp] = (float)re; G[2 * mp + 1] = (float)im;
  }
}

// a fast-convolution bank with a channel off (slot 0, gain 1): its channel step is asdr_tuner_palette.hip's
bool palette_in_use(const asdr_tuner_t *t) { return t->fc && t->n_off > 0; }

int push(asdr_tuner_t *t, hipStream_t stream) {
  const bool pal_push = palette_in_use(t) && (t->pal_dirty || t->sg_dirty || !t->d_pal_tab || !t->d_slot || !t->d_gain);
  if (!t->chan_dirty && !t->order_dirty && !t->taps_dirty && !(t->fc && t->g_dirty) && !pal_push) return 0;
  if (t->order_dirty) {
    t->order.resize(t->n);
    for (int i = 0; i < t->n; i++) t->order[i] = i;
    if (t->fc) {   // neighbouring waves gather overlapping bins of one source's X
      std::vector<int64_t> key(t->n);
      for (int i = 0; i < t->n; i++) key[i] = ((int64_t)t->chan[i].src << 32) + coarse_bin(t->chan[i].fw, t->log2n);
      std::stable_sort(t->order.begin(), t->order.end(), [&key](int a, int b) { return key[a] < key[b]; });
    } else {
      std::stable_sort(t->order.begin(), t->order.end(), [t](int a, int b) { return t->chan[a].src < t->chan[b].src; });
    }
    HIPCHK(hipMemcpyAsync(t->d_order, t->order.data(), t->n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  std::vector<float> G;
  if (t->fc && t->g_dirty) {
    G.assign(512, 0.0f);
    response(t->gch.data(), (int)t->gch.size(), false, G.data());
    HIPCHK(hipMemcpyAsync(t->d_fc_tab + 2 * ((1 << t->log2n) + 256), G.data(), G.size() * sizeof(float), hipMemcpyHostToDevice, stream));
  }
  std::vector<float> rows;
  if (pal_push) {   // the rows that changed since their last upload (all defined ones the first time), then the channels' arrays
    if (!t->d_pal_tab || !t->d_slot || !t->d_gain) {   // each under its own check: a failed allocation is tried again by the next call
      if (!t->d_pal_tab) HIPCHK(hipMalloc(&t->d_pal_tab, (size_t)ASDR_TUNER_FC_MAX_FILTERS * 512 * sizeof(float)));
      if (!t->d_slot) HIPCHK(hipMalloc(&t->d_slot, t->n * sizeof(int32_t)));
      if (!t->d_gain) HIPCHK(hipMalloc(&t->d_gain, t->n * sizeof(float)));
      t->sg_dirty = true;
    }
    int n_rows = 0;   // staging for the rows to upload only: a call that changed gains alone stages nothing
    for (int k = 0; k < ASDR_TUNER_FC_MAX_FILTERS; k++) n_rows += ((t->pal_dirty >> k) & 1) && (k == 0 || t->pal[k].n > 0);
    rows.resize((size_t)n_rows * 512);
    float *row = rows.data();
    for (int k = 0; k < ASDR_TUNER_FC_MAX_FILTERS; k++) {
      if (!((t->pal_dirty >> k) & 1) || (k > 0 && t->pal[k].n == 0)) continue;
      if (k == 0) response(t->gch.data(), (int)t->gch.size(), false, row);
      else response(t->pal[k].taps.data(), t->pal[k].n, t->pal[k].cx, row);
      HIPCHK(hipMemcpyAsync(t->d_pal_tab + (size_t)k * 512, row, 512 * sizeof(float), hipMemcpyHostToDevice, stream));
      row += 512;
    }
    if (t->sg_dirty) {
      HIPCHK(hipMemcpyAsync(t->d_slot, t->slot.data(), t->n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      HIPCHK(hipMemcpyAsync(t->d_gain, t->gain.data(), t->n * sizeof(float), hipMemcpyHostToDevice, stream));
    }
  }
  std::vector<int32_t> taps;
  if (t->taps_dirty && !t->fc) {
    const int D = t->D, L = (int)t->h.size();
    t->n_rows = (L + D - 1) / D;
    t->n_pairs = (D + 1) / 2;
    taps.assign((size_t)t->n_rows * t->n_pairs, 0);
    auto tap = [&](int k) -> int32_t { return (k >= 0 && k < L) ? (uint16_t)t->h[k] : 0; };
    for (int a = 0; a < t->n_rows; a++)
      for (int pp = 0; pp < t->n_pairs; pp++) {   // pairs with phases 2pp (low half) and 2pp + 1 (high half; zero pad for p = D)
        const int32_t lo = tap(a * D + D - 1 - 2 * pp), hi = (2 * pp + 1 < D) ? tap(a * D + D - 2 - 2 * pp) : 0;
        taps[(size_t)a * t->n_pairs + pp] = lo | (int32_t)((uint32_t)hi << 16);
      }
    HIPCHK(hipMemcpyAsync(t->d_taps, taps.data(), taps.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  if (t->chan_dirty) HIPCHK(hipMemcpyAsync(t->d_chan, t->chan.data(), t->n * sizeof(asdr_tuner_state_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));   // the host mirrors may change as soon as this returns
  t->chan_dirty = t->order_dirty = t->taps_dirty = false;
  if (t->fc) t->g_dirty = false;
  if (pal_push) { t->pal_dirty = 0; t->sg_dirty = false; }
  return 0;
}


// stage 2 is a pass-through (the output is u): U = M = 1, K = 1, h2 = {1 << s2}
bool pass_through(const asdr_tuner_t *t) {
  return t->up == 1 && t->down == 1 && t->h2.size() == 1 && t->g2 >= 1 && t->h2[0] == (1 << (15 - t->g2));
}

// b = floor(j M / U) and j M - b U without forming j M (exact for every j >= 0)
void split(long long j, int U, int M, long long &b, int &r) {
  const long long jq = j / U, jr = j % U;
  b = jq * M + (jr * M) / U;
  r = (int)((jr * M) % U);
}

// output blocks written by a call of n_frames frames: block J is out once b_{128 J + 127} <= N_u - 1, i.e.
// (128 J + 127) M <= N_u U - 1
long long blocks_after(const asdr_tuner_t *t, int n_frames) {
  const __int128 n_u = (__int128)(t->pos / t->D) + (__int128)128 * n_frames;
  const __int128 num = n_u * t->up - 1 - (__int128)127 * t->down;
  const long long j_next = t->out_pos / 128;
  const long long j_end = num < 0 ? 0 : (long long)(num / ((__int128)128 * t->down)) + 1;   // blocks 0 .. j_end - 1 are out
  return j_end > j_next ? j_end - j_next : 0;
}

int push_resampler(asdr_tuner_t *t, hipStream_t stream) {
  if (!t->rs_dirty) return 0;
  const int U = t->up, K = t->k2;
  t->kp = (K + 7) & ~7;
  std::vector<int16_t> taps((size_t)U * t->kp, 0);
  for (int ph = 0; ph < U; ph++)
    for (int k = 0; k < K; k++) taps[(size_t)ph * t->kp + k] = t->h2[(size_t)k * U + ph];
  std::vector<int32_t> qr(ASDR_TUNER_RS_OUT);
  for (int o = 0; o < ASDR_TUNER_RS_OUT; o++) qr[o] = ((o * t->down / U) << 11) | (o * t->down % U);
  HIPCHK(hipMemcpyAsync(t->d_rs_taps, taps.data(), taps.size() * sizeof(int16_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(t->d_lane_qr, qr.data(), qr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipStreamSynchronize(stream));
  t->rs_dirty = false;
  return 0;
}

const asdr_tuner_iq_t kIdentity = {0, 0, 0, 65536};
bool is_identity(const asdr_tuner_iq_t &c) { return c.dc_re == 0 && c.dc_im == 0 && c.cross_q16 == 0 && c.gain_q16 == 65536; }

// The pre-pass of a call (asdr_tuner_condition.hip) over n_in samples of every caller's row.  With a correction off the identity it
// writes x' of every source to the scratch and points in / in_stride / fmt at it (CS16, or RS16 for real rows); with only the
// statistics on it reads and sums, and the three stay the caller's; otherwise it does nothing at all.
int run_condition(asdr_tuner_t *t, const void *&in, long &in_stride, int &fmt, long long n_in, hipStream_t stream) {
  if (t->n_cond == 0 && !t->iq_stats_on) return 0;
  const bool write = t->n_cond > 0, real = fmt == ASDR_TUNER_IN_RS16;
  if (write) {
    if (stage_reserve(*t, &t->d_cond, &t->cond_cap, (size_t)t->n_src * n_in * (real ? 2 : 4)) != 0) return -1;
    if (t->corr_dirty || !t->d_corr) {
      if (!t->d_corr) HIPCHK(hipMalloc(&t->d_corr, (size_t)t->n_src * sizeof(asdr_tuner_iq_t)));
      HIPCHK(hipMemcpyAsync(t->d_corr, t->corr.data(), (size_t)t->n_src * sizeof(asdr_tuner_iq_t), hipMemcpyHostToDevice, stream));
      HIPCHK(hipStreamSynchronize(stream));   // the host mirror may change as soon as this returns
      t->corr_dirty = false;
    }
  }
  ConditionArgs c;
  c.in = in; c.out = write ? t->d_cond : nullptr; c.corr = t->d_corr; c.stats = t->iq_stats_on ? t->d_iq_stats : nullptr;
  c.in_stride = in_stride; c.out_stride = n_in; c.n_samples = n_in; c.n_sources = t->n_src; c.fmt = fmt;
  c.aligned = (((uintptr_t)in | (uintptr_t)((unsigned long long)in_stride * ASDR_TUNER_FMT_BYTES(fmt))) & 15u) == 0;
  if (asdr_launch_tuner_condition(&c, stream) != 0) return fail("tuner conditioning kernel launch failed");
  t->cond_launches++;
  if (write) { in = t->d_cond; in_stride = (long)n_in; fmt = real ? ASDR_TUNER_IN_RS16 : ASDR_TUNER_IN_CS16; }
  return 0;
}

// A fast-convolution bank's stage 1 (asdr_tuner_fastconv.hip): n_frames frames of every channel into rows out_stride_blocks apart;
// fmt is the format of the rows at dIQ (the bank's, or the conditioning scratch's).
int run_fastconv(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int fmt, int16_t *dI, int16_t *dQ, int n_frames,
                 long out_stride_blocks, hipStream_t stream) {
  const int log2n = t->log2n, N = 1 << log2n, H = N / 2;
  const size_t x_floats = (size_t)t->n_src * n_frames * N * 2;
  const size_t x_bytes = (log2n > 12 ? 2 : 1) * x_floats * sizeof(float);
  const size_t part_bytes = t->lev_on ? (size_t)t->n * n_frames * sizeof(float) : 0;
  if (stage_reserve(*t, (void **)&t->d_fc_x, &t->fc_x_cap, x_bytes) != 0 ||   // X and the scratch; the levels' partials
      stage_reserve(*t, (void **)&t->d_lev_part, &t->lev_part_cap, part_bytes) != 0)
    return -1;
  FcForwardArgs f;
  f.in = (const int32_t *)dIQ; f.hist_rd = t->d_hist[t->cur]; f.hist_wr = t->d_hist[t->cur ^ 1];
  f.tw = t->d_fc_tab; f.x = t->d_fc_x; f.scratch = t->d_fc_x + x_floats;
  f.in_stride = in_stride_samples; f.n_sources = t->n_src; f.n_frames = n_frames; f.hop = H;
  const int log2t = fmt == ASDR_TUNER_IN_RS16 ? log2n - 1 : log2n;   // RS16: a transform of N / 2 points, then the untangle
  f.log2n = log2n; f.log2n1 = (log2t + 1) / 2; f.log2n2 = log2t - f.log2n1;
  f.pass = log2n > 12 ? 1 : 0;
  f.fmt = fmt;
  FcChannelArgs c;
  c.x = t->d_fc_x; c.tw256 = t->d_fc_tab + 2 * N; c.g = t->d_fc_tab + 2 * (N + 256);
  c.chan = t->d_chan; c.order = t->d_order; c.out_i = dI; c.out_q = dQ;
  c.pos = t->pos; c.out_stride = (int64_t)out_stride_blocks * 128;
  c.n_channels = t->n; c.n_frames = n_frames; c.hop = H; c.log2n = log2n; c.decimation = t->D;
  FcSpectrumArgs sp;
  sp.x = t->d_fc_x; sp.acc = t->d_spec; sp.n_sources = t->n_src; sp.n_frames = n_frames; sp.log2n = log2n;
  for (sp.log2b = 0; (1 << sp.log2b) < t->spec_bins; sp.log2b++) {}
  sp.window = t->spec_win; sp.mode = t->spec_mode;
  FcLevelArgs lv;
  lv.part = t->d_lev_part; lv.acc = t->d_lev;
  if (palette_in_use(t)) {   // push() has brought the table and the channels' slots and gains up to date
    FcPaletteArgs pal;
    pal.tab = t->d_pal_tab; pal.slot = t->d_slot; pal.gain = t->d_gain;
    if (asdr_launch_tuner_fastconv_palette(&f, &c, t->spec_bins ? &sp : nullptr, t->lev_on ? &lv : nullptr, &pal, stream) != 0)
      return fail("fast-convolution kernel launch failed");
  } else if (asdr_launch_tuner_fastconv(&f, &c, t->spec_bins ? &sp : nullptr, t->lev_on ? &lv : nullptr, stream) != 0) {
    return fail("fast-convolution kernel launch failed");
  }
  if (t->spec_bins) t->spec_frames += n_frames;
  if (t->lev_on) t->lev_frames += n_frames;
  t->pos += (long long)n_frames * H;
  t->cur ^= 1;
  return 0;
}

// The stage-1 launch of a call: n_blocks blocks of every channel into rows out_stride_blocks apart, then P advances.
int run_stage1(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int16_t *dI, int16_t *dQ, int n_blocks,
               long out_stride_blocks, hipStream_t stream) {
  int fmt = t->fmt;
  if (run_condition(t, dIQ, in_stride_samples, fmt, (long long)n_blocks * 128 * t->D, stream) != 0) return -1;
  if (t->fc) return run_fastconv(t, dIQ, in_stride_samples, fmt, dI, dQ, n_blocks, out_stride_blocks, stream);
  TunerArgs a;
  a.in = (const int32_t *)dIQ; a.hist_rd = t->d_hist[t->cur]; a.hist_wr = t->d_hist[t->cur ^ 1];
  a.chan = t->d_chan; a.order = t->d_order; a.taps = t->d_taps; a.out_i = dI; a.out_q = dQ;
  a.pos = t->pos; a.in_stride = in_stride_samples; a.out_stride = (int64_t)out_stride_blocks * 128;
  a.n_channels = t->n; a.n_sources = t->n_src; a.n_blocks = n_blocks; a.decimation = t->D;
  a.n_phase_rows = t->n_rows; a.n_phase_pairs = t->n_pairs;
  a.shift = 15 - t->g; a.round = a.shift ? 1 << (a.shift - 1) : 0;
  a.fmt = fmt;
  if (asdr_launch_tuner(&a, stream) != 0) return fail("tuner kernel launch failed");
  t->pos += (long long)n_blocks * 128 * t->D;
  t->cur ^= 1;
  return 0;
}

// The argument checks shared by the update entry points (n_blocks = stage-1 blocks = frames, out_blocks = output row length).
int check_io(const asdr_tuner_t *t, const void *dIQ, long in_stride_samples, const int16_t *dI, const int16_t *dQ, int n_blocks,
             long out_stride_blocks, long out_blocks) {
  if (n_blocks > 65535 || (long long)n_blocks * 128 * t->D > (1LL << 30)) return fail("too many blocks in one call");
  const long long n_in = (long long)n_blocks * 128 * t->D;
  if (in_stride_samples < n_in) return fail("input row stride shorter than n_blocks * 128 * D samples");
  if (out_stride_blocks < out_blocks) return fail("output row stride shorter than n_blocks");
  if (in_stride_samples > (1LL << 40) || out_stride_blocks > (1LL << 30)) return fail("row stride too large");
  if ((((uintptr_t)dIQ | (uintptr_t)dI | (uintptr_t)dQ) & 15u) != 0) return fail("device pointers must be 16-byte aligned");
  const size_t in_bytes = ((size_t)(t->n_src - 1) * in_stride_samples + n_in) * ASDR_TUNER_FMT_BYTES(t->fmt);
  const size_t out_bytes = ((size_t)(t->n - 1) * out_stride_blocks + out_blocks) * 128 * 2;
  if (overlap((uintptr_t)dI, out_bytes, (uintptr_t)dIQ, in_bytes) || overlap((uintptr_t)dQ, out_bytes, (uintptr_t)dIQ, in_bytes))
    return fail("output span overlaps the input span");
  if (overlap((uintptr_t)dI, out_bytes, (uintptr_t)dQ, out_bytes)) return fail("I and Q output spans overlap");
  return 0;
}

// the checks every create starts with
int check_create(int n_channels, int n_sources) {
  if (stage_check_create(n_channels) != 0) return -1;
  return n_sources <= 0 || n_sources > 65535 ? fail("n_sources must be in 1..65535") : 0;
}

// a bank of either kind before its filters: geometry, ratio U / M, channels and sources in creation state
asdr_tuner_bank *new_bank(int n_channels, int n_sources, long long fs_in, int dr, long long up, long long down) {
  asdr_tuner_bank *t = new asdr_tuner_bank();
  t->n = n_channels; t->n_src = n_sources; t->D = dr;
  t->fs_in = fs_in; t->up = (int)up; t->down = (int)down;
  t->chan.assign(n_channels, fresh_state());
  t->corr.assign(n_sources, kIdentity);
  return t;
}

asdr_tuner_t *create_bank(int n_channels, int n_sources, long long fs_in, int decimation, int device) {
  if (check_create(n_channels, n_sources) != 0) return nullptr;
  if (decimation < 1 || decimation > ASDR_TUNER_MAX_DECIMATION) { fail("decimation must be in 1..64"); return nullptr; }
  if (fs_in <= 0) { fail("input rate Fs_in must be positive"); return nullptr; }
  if (fs_in % decimation != 0) { fail("input rate Fs_in is not a multiple of the decimation D"); return nullptr; }
  const long long fs_mid = fs_in / decimation;
  if (fs_mid < 44100 || fs_mid > 4 * 44100) { fail("Fs_in / D must lie in [44100, 176400] Hz"); return nullptr; }
  const long long gd = gcd_ll(44100, fs_mid);
  if (44100 / gd > ASDR_TUNER_MAX_UP) { fail("44100 / (Fs_in / D) in lowest terms needs U > 2048"); return nullptr; }
  asdr_tuner_bank *t = new_bank(n_channels, n_sources, fs_in, decimation, 44100 / gd, fs_mid / gd);
  default_rate_filter(decimation, fs_mid, t->h, t->g);
  default_resampler(t->up, t->down, fs_mid, t->h2, t->g2);
  t->k2 = (int)t->h2.size() / t->up;
  return open_device(t, device);
}

// The device side of a new bank (nothing for ASDR_NO_DEVICE); destroys the bank and returns NULL on failure.
asdr_tuner_t *open_device(asdr_tuner_bank *t, int device) {
  const int n_sources = t->n_src, n_channels = t->n;
  if (device == ASDR_NO_DEVICE) return t;
  if (stage_open(*t, device, "tuner bank", true) != 0) { asdr_tuner_destroy(t); return nullptr; }
  const size_t hist = (size_t)n_sources * t->hist_slots * sizeof(int32_t);
  if (hipMalloc(&t->d_chan, n_channels * sizeof(asdr_tuner_state_t)) != hipSuccess ||
      hipMalloc(&t->d_order, n_channels * sizeof(int32_t)) != hipSuccess || hipMalloc(&t->d_taps, kTapWords * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&t->d_hist[0], hist) != hipSuccess || hipMalloc(&t->d_hist[1], hist) != hipSuccess ||
      hipMalloc(&t->d_rs_taps, (size_t)t->up * ASDR_TUNER_MAX_RESAMPLER_TAPS * sizeof(int16_t)) != hipSuccess ||
      hipMalloc(&t->d_lane_qr, ASDR_TUNER_RS_OUT * sizeof(int32_t)) != hipSuccess ||
      hipMemset(t->d_hist[0], 0, hist) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fail("tuner bank: device allocation failed");
    asdr_tuner_destroy(t);
    return nullptr;
  }
  if (t->fc) {   // twiddles W_N^j, W_256^j from float64; G follows with the first push
    const int N = 1 << t->log2n;
    const double pi = 3.14159265358979323846;
    std::vector<float> tab(2 * ((size_t)N + 512), 0.0f);
    for (int j = 0; j < N; j++) { tab[2 * j] = (float)std::cos(2.0 * pi * j / N); tab[2 * j + 1] = (float)-std::sin(2.0 * pi * j / N); }
    for (int j = 0; j < 256; j++) {
      tab[2 * (N + j)] = (float)std::cos(2.0 * pi * j / 256); tab[2 * (N + j) + 1] = (float)-std::sin(2.0 * pi * j / 256);
    }
    if (hipMalloc(&t->d_fc_tab, tab.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(t->d_fc_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      fail("tuner bank: device allocation failed");
      asdr_tuner_destroy(t);
      return nullptr;
    }
  }
  return t;
}

asdr_tuner_t *create_fastconv(int n_channels, int n_sources, long long fs_in, int R, int device) {
  if (check_create(n_channels, n_sources) != 0) return nullptr;
  if (R < 2 || R > ASDR_TUNER_FC_MAX_R || (R & (R - 1)) != 0) { fail("R must be a power of two in 2..1024"); return nullptr; }
  if (fs_in <= 0) { fail("input rate Fs_in must be positive"); return nullptr; }
  if (fs_in < 44100LL * R || fs_in > 176400LL * R) { fail("Fs_in / R must lie in [44100, 176400] Hz"); return nullptr; }
  const long long gd = gcd_ll(44100LL * R, fs_in);
  if (44100LL * R / gd > ASDR_TUNER_MAX_UP) { fail("44100 R / Fs_in in lowest terms needs U > 2048"); return nullptr; }
  asdr_tuner_bank *t = new_bank(n_channels, n_sources, fs_in, R, 44100LL * R / gd, fs_in / gd);
  t->fc = true;
  for (t->log2n = 0; (1 << t->log2n) < 256 * R; t->log2n++) {}
  t->hist_slots = 128 * R;
  t->pal.resize(ASDR_TUNER_FC_MAX_FILTERS);
  t->slot.assign(n_channels, 0);
  t->gain.assign(n_channels, 1.0f);
  default_channel_filter((double)fs_in / R, t->gch);
  default_fastconv_resampler(t->up, t->down, fs_in, R, t->h2, t->g2);
  t->k2 = (int)t->h2.size() / t->up;
  return open_device(t, device);
}

// the int16 entry points on a bank of another format: fail before anything is read
bool wrong_format(const asdr_tuner_t *t, const char *entry) {
  if (t->fmt == ASDR_TUNER_IN_CS16) return false;
  fail(std::string(entry) + " takes CS16 rows and this bank's input format is " + kFormatNames[t->fmt] +
       ": use asdr_tuner_update_samples_device / asdr_tuner_update_samples");
  return true;
}

// The staging of the host-pointer entry points, one kept buffer: the call's input rows at its front, on their way there on the bank's
// stream when this returns; the output rows *dI and *dQ, out_bytes each, behind them from a 256-byte boundary ...
int io_in(asdr_tuner_t *t, const void *in, size_t in_bytes, size_t out_bytes, int16_t **dI, int16_t **dQ) {
  const size_t in_pad = (in_bytes + 255) & ~(size_t)255;
  HIPCHK(hipSetDevice(t->device));
  if (stage_reserve(*t, &t->d_io, &t->io_cap, in_pad + 2 * out_bytes) != 0) return -1;
  *dI = (int16_t *)((char *)t->d_io + in_pad); *dQ = (int16_t *)((char *)t->d_io + in_pad + out_bytes);
  HIPCHK(hipMemcpyAsync(t->d_io, in, in_bytes, hipMemcpyHostToDevice, t->stream));
  return 0;
}
// ... and back to the host behind the call's launches; waits for them
int io_out(asdr_tuner_t *t, int16_t *I, int16_t *Q, const int16_t *dI, const int16_t *dQ, size_t out_bytes) {
  if (out_bytes) {
    HIPCHK(hipMemcpyAsync(I, dI, out_bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipMemcpyAsync(Q, dQ, out_bytes, hipMemcpyDeviceToHost, t->stream));
  }
  HIPCHK(hipStreamSynchronize(t->stream));
  return 0;
}

int pass_device(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int16_t *dI, int16_t *dQ, int n_blocks,
                long out_stride_blocks, void *stream_);
int rate_device(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int n_frames, int16_t *dI, int16_t *dQ,
                int out_capacity_blocks, long out_stride_blocks, void *stream_);
int rate_host(asdr_tuner_t *t, const void *IQ, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks);
}  // namespace

extern "C" {

asdr_tuner_t *asdr_tuner_create(int n_channels, int n_sources, int decimation, int device) {
  if (decimation < 1 || decimation > ASDR_TUNER_MAX_DECIMATION) { fail("decimation must be in 1..64"); return nullptr; }
  return create_bank(n_channels, n_sources, 44100LL * decimation, decimation, device);
}

asdr_tuner_t *asdr_tuner_create_rate(int n_channels, int n_sources, long long fs_in_hz, int decimation, int device) {
  return create_bank(n_channels, n_sources, fs_in_hz, decimation, device);
}

asdr_tuner_t *asdr_tuner_create_fastconv(int n_channels, int n_sources, long long fs_in_hz, int R, int device) {
  return create_fastconv(n_channels, n_sources, fs_in_hz, R, device);
}

int asdr_tuner_fft_size(const asdr_tuner_t *t) { return t && t->fc ? 1 << t->log2n : 0; }

int asdr_tuner_set_channel_filter(asdr_tuner_t *t, const float *g, int n_taps) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail("only a fast-convolution bank has a channel filter: use asdr_tuner_set_filter");
  if (!g) return fail("null taps");
  if (n_taps < 1 || n_taps > ASDR_TUNER_FC_MAX_TAPS) return fail("channel filter length must be in 1..129");
  for (int k = 0; k < n_taps; k++)
    if (!std::isfinite(g[k])) return fail("channel filter taps must be finite");
  t->gch.assign(g, g + n_taps);
  t->g_dirty = true;
  t->pal_dirty |= 1;   // slot 0 of the palette's table
  return 0;
}

int asdr_tuner_get_channel_filter(const asdr_tuner_t *t, float *g, int cap) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail("only a fast-convolution bank has a channel filter: use asdr_tuner_get_filter");
  const int L = (int)t->gch.size();
  if (g) for (int k = 0; k < L && k < cap; k++) g[k] = t->gch[k];
  return L;
}

void asdr_tuner_destroy(asdr_tuner_t *t) {
  if (!t) return;
  stage_close(*t, {t->d_chan, t->d_order, t->d_taps, t->d_hist[0], t->d_hist[1], t->d_io, t->d_rs_taps, t->d_lane_qr, t->d_carry[0],
                   t->d_carry[1], t->d_mid, t->d_fc_tab, t->d_fc_x, t->d_spec, t->d_lev, t->d_lev_part, t->d_pal_tab, t->d_slot,
                   t->d_gain, t->d_corr, t->d_cond, t->d_iq_stats, t->st_d});
  if (t->st_h) hipHostFree(t->st_h);   // (both exist on a device bank only, and nothing uses them behind stage_close's wait)
  if (t->st_ev) hipEventDestroy(t->st_ev);
  delete t;
}

int asdr_tuner_reset(asdr_tuner_t *t) {
  if (!t) return fail("null tuner bank");
  if (t->device != ASDR_NO_DEVICE) {
    if (asdr_tuner_synchronize(t) != 0) return -1;
    HIPCHK(hipMemset(t->d_hist[t->cur], 0, (size_t)t->n_src * t->hist_slots * sizeof(int32_t)));
    if (t->d_carry[t->ccur]) HIPCHK(hipMemset(t->d_carry[t->ccur], 0, (size_t)t->n * ASDR_TUNER_CARRY * sizeof(int32_t)));
    if (t->d_spec) HIPCHK(hipMemset(t->d_spec, 0, (size_t)t->n_src * t->spec_bins * sizeof(double)));
    if (t->d_lev) HIPCHK(hipMemset(t->d_lev, 0, (size_t)t->n * sizeof(double)));
    if (t->d_iq_stats) HIPCHK(hipMemset(t->d_iq_stats, 0, (size_t)t->n_src * sizeof(asdr_tuner_iq_stats_t)));
    HIPCHK(hipDeviceSynchronize());
  }
  t->spec_frames = t->lev_frames = 0;
  t->pos = 0;
  t->out_pos = 0;
  t->carry_stale = false;
  std::fill(t->chan.begin(), t->chan.end(), fresh_state());
  t->chan_dirty = t->order_dirty = true;
  if (t->fc) {   // every channel back to slot 0 and gain 1; the palette's slots stay
    std::fill(t->slot.begin(), t->slot.end(), 0);
    std::fill(t->gain.begin(), t->gain.end(), 1.0f);
    t->n_off = 0;
    t->sg_dirty = true;
  }
  return 0;
}

long long asdr_tuner_position(const asdr_tuner_t *t) { return t ? t->pos : -1; }
int asdr_tuner_n_channels(const asdr_tuner_t *t) { return t ? t->n : 0; }
int asdr_tuner_n_sources(const asdr_tuner_t *t) { return t ? t->n_src : 0; }
int asdr_tuner_decimation(const asdr_tuner_t *t) { return t ? t->D : 0; }

int asdr_tuner_set_source(asdr_tuner_t *t, int ch, int source) {
  if (t && (source < 0 || source >= t->n_src)) return fail("source index out of range");
  if (retune(t, ch, [source](asdr_tuner_state_t &s) { s.src = source; }) != 0) return -1;
  t->order_dirty = true;
  return 0;
}

int asdr_tuner_set_frequency(asdr_tuner_t *t, int ch, double hz) {
  if (!t) return fail("null tuner bank");
  const double fs = (double)t->fs_in;
  if (!(hz >= -0.5 * fs && hz <= 0.5 * fs)) return fail("frequency outside [-Fs_in/2, Fs_in/2]");
  const uint32_t fw = (uint32_t)(int64_t)std::llround(hz * 4294967296.0 / fs);
  return retune(t, ch, [fw](asdr_tuner_state_t &s) { s.fw = fw; });
}

int asdr_tuner_set_frequency_word(asdr_tuner_t *t, int ch, uint32_t fw) {
  return retune(t, ch, [fw](asdr_tuner_state_t &s) { s.fw = fw; });
}

int asdr_tuner_set_phase(asdr_tuner_t *t, int ch, uint32_t phase) {
  return retune(t, ch, [phase](asdr_tuner_state_t &s) { s.ph_a = phase; });
}

int asdr_tuner_set_filter(asdr_tuner_t *t, const int16_t *h, int n_taps, int gain_shift) {
  if (!t) return fail("null tuner bank");
  if (t->fc) return fail("a fast-convolution bank has a float channel filter: use asdr_tuner_set_channel_filter");
  if (!h) return fail("null taps");
  if (n_taps < 1 || n_taps > ASDR_TUNER_MAX_TAPS) return fail("filter length must be in 1..1024");
  if (gain_shift < 0 || gain_shift > ASDR_TUNER_MAX_GAIN_SHIFT) return fail("gain shift must be in 0..15");
  long sum = 0;
  for (int k = 0; k < n_taps; k++) sum += std::labs((long)h[k]);
  if (sum > 65535) return fail("sum of |h| exceeds 65535");
  t->h.assign(h, h + n_taps);
  t->g = gain_shift;
  t->taps_dirty = true;
  return 0;
}

int asdr_tuner_get_filter(const asdr_tuner_t *t, int16_t *h, int cap, int *gain_shift) {
  if (!t) return fail("null tuner bank");
  if (t->fc) return fail("a fast-convolution bank has a float channel filter: use asdr_tuner_get_channel_filter");
  const int L = (int)t->h.size();
  if (h) for (int k = 0; k < L && k < cap; k++) h[k] = t->h[k];
  if (gain_shift) *gain_shift = t->g;
  return L;
}

int asdr_tuner_read_state(const asdr_tuner_t *t, asdr_tuner_state_t *dst) {
  if (!t) return fail("null tuner bank");
  if (!dst) return fail("null destination");
  memcpy(dst, t->chan.data(), t->n * sizeof(asdr_tuner_state_t));
  return 0;
}

int asdr_tuner_update_device(asdr_tuner_t *t, const int16_t *dIQ, long in_stride_samples, int16_t *dI, int16_t *dQ, int n_blocks,
                             long out_stride_blocks, void *stream_) {
  if (!t) return fail("null tuner bank");
  if (wrong_format(t, "asdr_tuner_update_device")) return -1;
  return pass_device(t, dIQ, in_stride_samples, dI, dQ, n_blocks, out_stride_blocks, stream_);
}

}  // extern "C"

namespace {
// asdr_tuner_update_device on rows of the bank's format
int pass_device(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int16_t *dI, int16_t *dQ, int n_blocks,
                long out_stride_blocks, void *stream_) {
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!pass_through(t)) return fail("stage 2 of this bank resamples: use asdr_tuner_update_rate_device / asdr_tuner_update_rate");
  if (!dIQ || !dI || !dQ) return fail("null device pointer");
  if (n_blocks <= 0) return 0;
  if (check_io(t, dIQ, in_stride_samples, dI, dQ, n_blocks, out_stride_blocks, n_blocks) != 0) return -1;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*t, stream) != 0 || push(t, stream) != 0 || stage_mark_start(*t, stream) != 0) return -1;
  if (run_stage1(t, dIQ, in_stride_samples, dI, dQ, n_blocks, out_stride_blocks, stream) != 0) return -1;
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->out_pos += (long long)n_blocks * 128;   // a pass-through stage 2 writes every u sample at once
  t->carry_stale = true;                      // and keeps no history
  return 0;
}
}  // namespace

extern "C" {

int asdr_tuner_update(asdr_tuner_t *t, const int16_t *IQ, int16_t *I, int16_t *Q, int n_blocks) {
  if (!t) return fail("null tuner bank");
  if (wrong_format(t, "asdr_tuner_update")) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!pass_through(t)) return fail("stage 2 of this bank resamples: use asdr_tuner_update_rate_device / asdr_tuner_update_rate");
  if (!IQ || !I || !Q) return fail("null host pointer");
  if (n_blocks <= 0) return 0;
  if (n_blocks > 65535) return fail("too many blocks in one call");
  const size_t n_in = (size_t)n_blocks * 128 * t->D, out_bytes = (size_t)t->n * n_blocks * 128 * 2;
  int16_t *dI, *dQ;
  if (io_in(t, IQ, (size_t)t->n_src * n_in * 4, out_bytes, &dI, &dQ) != 0) return -1;
  if (asdr_tuner_update_device(t, (const int16_t *)t->d_io, (long)n_in, dI, dQ, n_blocks, n_blocks, t->stream) != 0) return -1;
  return io_out(t, I, Q, dI, dQ, out_bytes);
}

long long asdr_tuner_rate(const asdr_tuner_t *t) { return t ? t->fs_in : 0; }

int asdr_tuner_ratio(const asdr_tuner_t *t, int *up, int *down) {
  if (!t) return fail("null tuner bank");
  if (up) *up = t->up;
  if (down) *down = t->down;
  return 0;
}

long long asdr_tuner_output_position(const asdr_tuner_t *t) { return t ? t->out_pos : -1; }

int asdr_tuner_set_resampler(asdr_tuner_t *t, const int16_t *h2, int n_taps, int gain_shift) {
  if (!t) return fail("null tuner bank");
  const std::string e = resampler_error(t->up, h2, n_taps, gain_shift);
  if (!e.empty()) return fail(e);
  t->h2.assign(h2, h2 + n_taps);
  t->g2 = gain_shift;
  t->k2 = n_taps / t->up;
  t->rs_dirty = true;
  return 0;
}

int asdr_tuner_get_resampler(const asdr_tuner_t *t, int16_t *h2, int cap, int *gain_shift) {
  if (!t) return fail("null tuner bank");
  const int L = (int)t->h2.size();
  if (h2) for (int k = 0; k < L && k < cap; k++) h2[k] = t->h2[k];
  if (gain_shift) *gain_shift = t->g2;
  return L;
}

int asdr_tuner_out_blocks(const asdr_tuner_t *t, int n_frames) {
  if (!t) return fail("null tuner bank");
  if (n_frames < 0 || n_frames > 65535) return fail("n_frames must be in 0..65535");
  return (int)blocks_after(t, n_frames);
}

int asdr_tuner_update_rate_device(asdr_tuner_t *t, const int16_t *dIQ, long in_stride_samples, int n_frames, int16_t *dI,
                                  int16_t *dQ, int out_capacity_blocks, long out_stride_blocks, void *stream_) {
  if (!t) return fail("null tuner bank");
  if (wrong_format(t, "asdr_tuner_update_rate_device")) return -1;
  return rate_device(t, dIQ, in_stride_samples, n_frames, dI, dQ, out_capacity_blocks, out_stride_blocks, stream_);
}

int asdr_tuner_update_rate(asdr_tuner_t *t, const int16_t *IQ, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks) {
  if (!t) return fail("null tuner bank");
  if (wrong_format(t, "asdr_tuner_update_rate")) return -1;
  return rate_host(t, IQ, n_frames, I, Q, out_capacity_blocks);
}

int asdr_tuner_set_input_format(asdr_tuner_t *t, int format) {
  if (!t) return fail("null tuner bank");
  if (format < ASDR_TUNER_IN_CS16 || format > ASDR_TUNER_IN_RS16) return fail("unknown input format (ASDR_TUNER_IN_CS16 .. ASDR_TUNER_IN_RS16)");
  t->fmt = format;
  return 0;
}

int asdr_tuner_input_format(const asdr_tuner_t *t) { return t ? t->fmt : -1; }

int asdr_tuner_update_samples_device(asdr_tuner_t *t, const void *dIn, long in_stride_samples, int n_frames, int16_t *dI, int16_t *dQ,
                                     int out_capacity_blocks, long out_stride_blocks, void *stream_) {
  if (!t) return fail("null tuner bank");
  const long long bps = ASDR_TUNER_FMT_BYTES(t->fmt);
  if (!dIn || !dI || !dQ) return fail("null device pointer");
  if (in_stride_samples < 0) return fail("input row stride is negative");
  if (((uintptr_t)dIn & 15u) != 0 || ((unsigned long long)in_stride_samples * bps) % 16 != 0)
    return fail(std::string("input rows must start 16-byte aligned: the base pointer, and the row stride a multiple of ") +
                std::to_string(16 / bps) + " " + kFormatNames[t->fmt] + " samples");
  return rate_device(t, dIn, in_stride_samples, n_frames, dI, dQ, out_capacity_blocks, out_stride_blocks, stream_);
}

int asdr_tuner_update_samples(asdr_tuner_t *t, const void *In, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks) {
  if (!t) return fail("null tuner bank");
  return rate_host(t, In, n_frames, I, Q, out_capacity_blocks);
}

}  // extern "C"

namespace {
// asdr_tuner_update_rate_device on rows of the bank's format
int rate_device(asdr_tuner_t *t, const void *dIQ, long in_stride_samples, int n_frames, int16_t *dI, int16_t *dQ,
                int out_capacity_blocks, long out_stride_blocks, void *stream_) {
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!dIQ || !dI || !dQ) return fail("null device pointer");
  if (n_frames < 0 || n_frames > 65535) return fail("n_frames must be in 0..65535");
  if (n_frames == 0) return 0;
  const long long nb = blocks_after(t, n_frames);
  if (nb > out_capacity_blocks)
    return fail("output capacity of " + std::to_string(out_capacity_blocks) + " blocks: this call writes " + std::to_string(nb));
  if (out_stride_blocks < out_capacity_blocks) return fail("output row stride shorter than the output capacity");
  if (check_io(t, dIQ, in_stride_samples, dI, dQ, n_frames, out_stride_blocks, out_capacity_blocks) != 0) return -1;
  if (pass_through(t))
    return pass_device(t, dIQ, in_stride_samples, dI, dQ, n_frames, out_stride_blocks, stream_) == 0 ? n_frames : -1;
  hipStream_t stream = (hipStream_t)stream_;
  const size_t row = (size_t)n_frames * 128, mid_bytes = 2 * (size_t)t->n * row * sizeof(int16_t);
  if (stage_reserve(*t, (void **)&t->d_mid, &t->mid_cap, mid_bytes) != 0) return -1;
  if (!t->d_carry[0]) {   // the first stage-2 call allocates the carry: nothing of ours may be in flight
    const size_t cb = (size_t)t->n * ASDR_TUNER_CARRY * sizeof(int32_t);
    if (stage_quiesce(*t) != 0) return -1;
    HIPCHK(hipMalloc(&t->d_carry[0], cb));
    HIPCHK(hipMalloc(&t->d_carry[1], cb));
    HIPCHK(hipMemset(t->d_carry[t->ccur], 0, cb));
    HIPCHK(hipDeviceSynchronize());
    t->carry_stale = false;
  }
  if (stage_before_launch(*t, stream) != 0 || push(t, stream) != 0 || push_resampler(t, stream) != 0 ||
      stage_mark_start(*t, stream) != 0)
    return -1;
  if (t->carry_stale) {   // the pass-through calls before this one kept no stage-2 history (asdr_tuner.h)
    HIPCHK(hipMemsetAsync(t->d_carry[t->ccur], 0, (size_t)t->n * ASDR_TUNER_CARRY * sizeof(int32_t), stream));
    t->carry_stale = false;
  }
  const long long n_u = t->pos / t->D;
  int16_t *mid_i = t->d_mid, *mid_q = t->d_mid + (size_t)t->n * row;
  if (run_stage1(t, dIQ, in_stride_samples, mid_i, mid_q, n_frames, n_frames, stream) != 0) return -1;
  ResampleArgs r;
  r.mid_i = mid_i; r.mid_q = mid_q;
  r.carry_rd = t->d_carry[t->ccur]; r.carry_wr = t->d_carry[t->ccur ^ 1];
  r.taps = t->d_rs_taps; r.lane_qr = t->d_lane_qr; r.out_i = dI; r.out_q = dQ;
  r.out_stride = (int64_t)out_stride_blocks * 128;
  r.n_channels = t->n; r.n_frames = n_frames; r.n_out = (int)(nb * 128);
  r.up = t->up; r.down = t->down; r.k = t->k2; r.kp = t->kp;
  long long b0;
  split(t->out_pos, t->up, t->down, b0, r.r0);
  r.q0 = (int)(b0 - (n_u - ASDR_TUNER_CARRY));
  r.tile_q = ASDR_TUNER_RS_OUT * t->down / t->up; r.tile_r = ASDR_TUNER_RS_OUT * t->down % t->up;
  r.shift = 15 - t->g2; r.round = r.shift ? 1 << (r.shift - 1) : 0;
  if (r.q0 - (r.k - 1) < 0) return fail("internal: stage-2 window starts before the carry");
  if (asdr_launch_tuner_resample(&r, stream) != 0) return fail("tuner resampler kernel launch failed");
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->ccur ^= 1;
  t->out_pos += nb * 128;
  return (int)nb;
}

// asdr_tuner_update_rate on rows of the bank's format
int rate_host(asdr_tuner_t *t, const void *IQ, int n_frames, int16_t *I, int16_t *Q, int out_capacity_blocks) {
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!IQ || !I || !Q) return fail("null host pointer");
  if (n_frames < 0 || n_frames > 65535) return fail("n_frames must be in 0..65535");
  if (n_frames == 0) return 0;
  const long long nb = blocks_after(t, n_frames);
  if (nb > out_capacity_blocks)
    return fail("output capacity of " + std::to_string(out_capacity_blocks) + " blocks: this call writes " + std::to_string(nb));
  const size_t n_in = (size_t)n_frames * 128 * t->D, out_bytes = (size_t)t->n * nb * 128 * 2;
  int16_t *dI, *dQ;
  if (io_in(t, IQ, (size_t)t->n_src * n_in * ASDR_TUNER_FMT_BYTES(t->fmt), out_bytes, &dI, &dQ) != 0) return -1;
  const int got = rate_device(t, t->d_io, (long)n_in, n_frames, dI, dQ, (int)nb, (long)nb, t->stream);
  return got < 0 || io_out(t, I, Q, dI, dQ, out_bytes) != 0 ? -1 : got;
}
}  // namespace

extern "C" {

int asdr_tuner_synchronize(asdr_tuner_t *t) {
  return t ? stage_quiesce(*t) : fail("null tuner bank");
}

float asdr_tuner_last_kernel_ms(asdr_tuner_t *t) { return t ? stage_last_ms(*t) : -1.0f; }

}  // extern "C"

// ---- monitors (include/asdr_tuner.h, "Monitors")
namespace {
const char *kNoMonitor = "only a fast-convolution bank has monitors: a direct-form or rate bank computes no spectrum X";

// (re)allocate a monitor's accumulator of n doubles (n = 0: free it) and zero it; nothing of ours is in flight afterwards
int monitor_alloc(asdr_tuner_t *t, double **acc, size_t n) {
  if (t->device == ASDR_NO_DEVICE) return 0;
  if (asdr_tuner_synchronize(t) != 0) return -1;
  double *fresh = nullptr;
  if (n) {
    HIPCHK(hipMalloc(&fresh, n * sizeof(double)));
    if (hipMemset(fresh, 0, n * sizeof(double)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      hipFree(fresh);
      return fail("tuner monitor: clearing the accumulators failed");
    }
  }
  if (*acc) hipFree(*acc);
  *acc = fresh;
  return 0;
}

// the shared read: wait, copy n doubles and the count out, clear on request
int monitor_read(asdr_tuner_t *t, double *acc, size_t n, long long *count, double *dst, long long *frames, int clear) {
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (asdr_tuner_synchronize(t) != 0) return -1;
  if (dst) HIPCHK(hipMemcpy(dst, acc, n * sizeof(double), hipMemcpyDeviceToHost));
  if (frames) *frames = *count;
  if (clear) {
    HIPCHK(hipMemset(acc, 0, n * sizeof(double)));
    HIPCHK(hipDeviceSynchronize());
    *count = 0;
  }
  return 0;
}
}  // namespace

extern "C" {

int asdr_tuner_spectrum_enable(asdr_tuner_t *t, int n_bins, int window, int mode) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoMonitor);
  if (n_bins != 0) {
    if (n_bins < 256 || n_bins > (1 << t->log2n) || (n_bins & (n_bins - 1)) != 0)
      return fail("spectrum bins must be 0 (off) or a power of two in 256.." + std::to_string(1 << t->log2n) + " (the FFT size)");
    if (window != ASDR_TUNER_WIN_RECT && window != ASDR_TUNER_WIN_HANN) return fail("unknown spectrum window (ASDR_TUNER_WIN_RECT, ASDR_TUNER_WIN_HANN)");
    if (mode != ASDR_TUNER_MON_SUM && mode != ASDR_TUNER_MON_PEAK) return fail("unknown spectrum mode (ASDR_TUNER_MON_SUM, ASDR_TUNER_MON_PEAK)");
  }
  if (monitor_alloc(t, &t->d_spec, (size_t)t->n_src * n_bins) != 0) return -1;
  t->spec_bins = n_bins;
  if (n_bins) { t->spec_win = window; t->spec_mode = mode; }
  t->spec_frames = 0;
  return 0;
}

int asdr_tuner_spectrum_bins(const asdr_tuner_t *t) { return t && t->fc ? t->spec_bins : 0; }
int asdr_tuner_spectrum_window(const asdr_tuner_t *t) { return t && t->fc && t->spec_bins ? t->spec_win : -1; }
int asdr_tuner_spectrum_mode(const asdr_tuner_t *t) { return t && t->fc && t->spec_bins ? t->spec_mode : -1; }
long long asdr_tuner_spectrum_frames(const asdr_tuner_t *t) { return t && t->fc && t->spec_bins ? t->spec_frames : -1; }

int asdr_tuner_spectrum_read(asdr_tuner_t *t, double *dst, long long *frames, int clear) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoMonitor);
  if (!t->spec_bins) return fail("the spectrum monitor is off: asdr_tuner_spectrum_enable");
  return monitor_read(t, t->d_spec, (size_t)t->n_src * t->spec_bins, &t->spec_frames, dst, frames, clear);
}

const double *asdr_tuner_spectrum_device(asdr_tuner_t *t) {
  if (!t) { fail("null tuner bank"); return nullptr; }
  if (!t->fc) { fail(kNoMonitor); return nullptr; }
  if (!t->spec_bins) { fail("the spectrum monitor is off: asdr_tuner_spectrum_enable"); return nullptr; }
  if (t->device == ASDR_NO_DEVICE) { fail(kNoDevice); return nullptr; }
  return t->d_spec;
}

int asdr_tuner_spectrum_clear(asdr_tuner_t *t) { return asdr_tuner_spectrum_read(t, nullptr, nullptr, 1); }

int asdr_tuner_levels_enable(asdr_tuner_t *t, int on) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoMonitor);
  if (monitor_alloc(t, &t->d_lev, on ? (size_t)t->n : 0) != 0) return -1;
  t->lev_on = on != 0;
  t->lev_frames = 0;
  return 0;
}

int asdr_tuner_levels_enabled(const asdr_tuner_t *t) { return t && t->fc && t->lev_on ? 1 : 0; }
long long asdr_tuner_levels_frames(const asdr_tuner_t *t) { return t && t->fc && t->lev_on ? t->lev_frames : -1; }

int asdr_tuner_levels_read(asdr_tuner_t *t, double *dst, long long *frames, int clear) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoMonitor);
  if (!t->lev_on) return fail("the level monitor is off: asdr_tuner_levels_enable");
  return monitor_read(t, t->d_lev, (size_t)t->n, &t->lev_frames, dst, frames, clear);
}

const double *asdr_tuner_levels_device(asdr_tuner_t *t) {
  if (!t) { fail("null tuner bank"); return nullptr; }
  if (!t->fc) { fail(kNoMonitor); return nullptr; }
  if (!t->lev_on) { fail("the level monitor is off: asdr_tuner_levels_enable"); return nullptr; }
  if (t->device == ASDR_NO_DEVICE) { fail(kNoDevice); return nullptr; }
  return t->d_lev;
}

int asdr_tuner_levels_clear(asdr_tuner_t *t) { return asdr_tuner_levels_read(t, nullptr, nullptr, 1); }

}  // extern "C"

// ---- filter palette and gain (include/asdr_tuner.h, "Filter palette and gain")
namespace {
const char *kNoPalette = "only a fast-convolution bank has a filter palette and channel gains: a direct-form or rate bank has one integer filter";

bool channel_off(const asdr_tuner_t *t, int c) { return t->slot[c] != 0 || t->gain[c] != 1.0f; }

// f(c) on channel `ch` or on every channel, keeping the count of channels off (slot 0, gain 1)
template <typename F>
int each_channel(asdr_tuner_t *t, int ch, F f) {
  if (ch != ASDR_ALL && (ch < 0 || ch >= t->n)) return fail("bad channel");
  for (int c = (ch == ASDR_ALL ? 0 : ch); c < (ch == ASDR_ALL ? t->n : ch + 1); c++) {
    t->n_off -= channel_off(t, c);
    f(c);
    t->n_off += channel_off(t, c);
  }
  t->sg_dirty = true;
  return 0;
}
}  // namespace

extern "C" {

int asdr_tuner_palette_set(asdr_tuner_t *t, int slot, const float *taps, int n_taps, int is_complex) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (slot == 0) return fail("palette slot 0 is the bank's channel filter: use asdr_tuner_set_channel_filter");
  if (slot < 0 || slot >= ASDR_TUNER_FC_MAX_FILTERS) return fail("palette slot must be in 1..63");
  if (!taps) return fail("null taps");
  if (n_taps < 1 || n_taps > ASDR_TUNER_FC_MAX_TAPS) return fail("palette filter length must be in 1..129");
  const int n_values = is_complex ? 2 * n_taps : n_taps;
  for (int k = 0; k < n_values; k++)
    if (!std::isfinite(taps[k])) return fail("palette filter taps must be finite");
  asdr_tuner_bank::PaletteSlot &p = t->pal[slot];
  p.taps.assign(taps, taps + n_values);
  p.cx = is_complex != 0;
  p.n = n_taps;
  t->pal_dirty |= 1ull << slot;
  return 0;
}

int asdr_tuner_palette_get(const asdr_tuner_t *t, int slot, float *taps, int cap, int *is_complex) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (slot < 0 || slot >= ASDR_TUNER_FC_MAX_FILTERS) return fail("palette slot must be in 0..63");
  const bool cx = slot != 0 && t->pal[slot].cx;
  const int L = slot == 0 ? (int)t->gch.size() : t->pal[slot].n;
  const float *src = slot == 0 ? t->gch.data() : t->pal[slot].taps.data();
  const int per = cx ? 2 : 1;
  if (taps) for (int k = 0; k < per * L && k < per * cap; k++) taps[k] = src[k];
  if (is_complex) *is_complex = cx ? 1 : 0;
  return L;
}

int asdr_tuner_palette_clear(asdr_tuner_t *t, int slot) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (slot == 0) return fail("palette slot 0 is the bank's channel filter and cannot be cleared");
  if (slot < 0 || slot >= ASDR_TUNER_FC_MAX_FILTERS) return fail("palette slot must be in 1..63");
  for (int c = 0; c < t->n; c++)
    if (t->slot[c] == slot) return fail("palette slot " + std::to_string(slot) + " is in use by channel " + std::to_string(c));
  t->pal[slot] = asdr_tuner_bank::PaletteSlot();
  return 0;
}

int asdr_tuner_set_channel_slot(asdr_tuner_t *t, int ch, int slot) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (slot < 0 || slot >= ASDR_TUNER_FC_MAX_FILTERS) return fail("palette slot must be in 0..63");
  if (slot != 0 && t->pal[slot].n == 0) return fail("palette slot " + std::to_string(slot) + " is undefined: asdr_tuner_palette_set");
  return each_channel(t, ch, [t, slot](int c) { t->slot[c] = slot; });
}

int asdr_tuner_read_slots(const asdr_tuner_t *t, int32_t *dst) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (!dst) return fail("null destination");
  memcpy(dst, t->slot.data(), t->n * sizeof(int32_t));
  return 0;
}

int asdr_tuner_set_channel_gain(asdr_tuner_t *t, int ch, float gain) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (!std::isfinite(gain) || std::fabs(gain) > ASDR_TUNER_FC_MAX_GAIN) return fail("channel gain must be finite with |gain| <= 32768");
  return each_channel(t, ch, [t, gain](int c) { t->gain[c] = gain; });
}

int asdr_tuner_read_gains(const asdr_tuner_t *t, float *dst) {
  if (!t) return fail("null tuner bank");
  if (!t->fc) return fail(kNoPalette);
  if (!dst) return fail("null destination");
  memcpy(dst, t->gain.data(), t->n * sizeof(float));
  return 0;
}

}  // extern "C"

// ---- source conditioning (include/asdr_tuner.h, "Source conditioning")
static_assert(sizeof(asdr_tuner_iq_t) == 4 * sizeof(int32_t), "the kernel reads a correction as four int32");
static_assert(sizeof(asdr_tuner_iq_stats_t) == ASDR_TUNER_IQ_STATS_WORDS * sizeof(int64_t), "the kernel adds into seven int64 per source");

namespace {
std::string correction_error(const asdr_tuner_iq_t &c) {
  if (c.dc_re < -32768 || c.dc_re > 32767 || c.dc_im < -32768 || c.dc_im > 32767) return "dc_re and dc_im must be in -32768..32767";
  if (c.cross_q16 < -32768 || c.cross_q16 > 32768) return "cross_q16 must be in -32768..32768";
  if (c.gain_q16 < 32768 || c.gain_q16 > 131072) return "gain_q16 must be in 32768..131072";
  return "";
}

void set_correction(asdr_tuner_t *t, int s, const asdr_tuner_iq_t &c) {
  t->n_cond -= !is_identity(t->corr[s]);
  t->corr[s] = c;
  t->n_cond += !is_identity(c);
  t->corr_dirty = true;
}

// wait for the bank's work, copy the statistics out (dst may be NULL), clear them on request
int stats_read(asdr_tuner_t *t, asdr_tuner_iq_stats_t *dst, int clear) {
  if (!t->iq_stats_on) return fail("the I/Q statistics are off: asdr_tuner_iq_stats_enable");
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (asdr_tuner_synchronize(t) != 0) return -1;
  const size_t bytes = (size_t)t->n_src * sizeof(asdr_tuner_iq_stats_t);
  if (dst) HIPCHK(hipMemcpy(dst, t->d_iq_stats, bytes, hipMemcpyDeviceToHost));
  if (clear) {
    HIPCHK(hipMemset(t->d_iq_stats, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  return 0;
}
}  // namespace

extern "C" {

int asdr_tuner_set_iq_correction(asdr_tuner_t *t, int source, const asdr_tuner_iq_t *c) {
  if (!t) return fail("null tuner bank");
  if (!c) return fail("null correction");
  if (source != ASDR_ALL && (source < 0 || source >= t->n_src)) return fail("source index out of range");
  const std::string e = correction_error(*c);
  if (!e.empty()) return fail(e);
  for (int s = (source == ASDR_ALL ? 0 : source); s < (source == ASDR_ALL ? t->n_src : source + 1); s++) set_correction(t, s, *c);
  return 0;
}

int asdr_tuner_get_iq_correction(const asdr_tuner_t *t, int source, asdr_tuner_iq_t *c) {
  if (!t) return fail("null tuner bank");
  if (!c) return fail("null destination");
  if (source < 0 || source >= t->n_src) return fail("source index out of range");
  *c = t->corr[source];
  return 0;
}

int asdr_tuner_iq_stats_enable(asdr_tuner_t *t, int on) {
  if (!t) return fail("null tuner bank");
  if (t->device != ASDR_NO_DEVICE) {   // (re)allocate cleared, or free: nothing of ours may be in flight
    if (asdr_tuner_synchronize(t) != 0) return -1;
    HIPCHK(hipSetDevice(t->device));
    unsigned long long *fresh = nullptr;
    if (on) {
      const size_t bytes = (size_t)t->n_src * sizeof(asdr_tuner_iq_stats_t);
      HIPCHK(hipMalloc(&fresh, bytes));
      if (hipMemset(fresh, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        hipFree(fresh);
        return fail("tuner I/Q statistics: clearing the sums failed");
      }
    }
    if (t->d_iq_stats) hipFree(t->d_iq_stats);
    t->d_iq_stats = fresh;
  }
  t->iq_stats_on = on != 0;
  return 0;
}

int asdr_tuner_iq_stats_enabled(const asdr_tuner_t *t) { return t && t->iq_stats_on ? 1 : 0; }

int asdr_tuner_iq_stats_read(asdr_tuner_t *t, asdr_tuner_iq_stats_t *dst, int clear) {
  if (!t) return fail("null tuner bank");
  if (!dst) return fail("null destination");
  return stats_read(t, dst, clear);
}

int asdr_tuner_iq_stats_clear(asdr_tuner_t *t) {
  if (!t) return fail("null tuner bank");
  return stats_read(t, nullptr, 1);
}

// The statement's order of operations, one rounding each: the library is built without FMA contraction.
int asdr_tuner_iq_estimate(const asdr_tuner_iq_stats_t *s, asdr_tuner_iq_t *c) {
  if (!s) return fail("null statistics");
  if (!c) return fail("null destination");
  if (s->n < 2) return fail("I/Q estimate: fewer than two samples");
  const double n = (double)s->n;
  const double m_r = (double)s->sum_re / n, m_i = (double)s->sum_im / n;
  asdr_tuner_iq_t out = kIdentity;
  double p = 0.0, g = 65536.0;
  if (s->sum_im != 0 || s->sum_im2 != 0 || s->sum_reim != 0) {
    const double v_rr = (double)s->sum_re2 / n - m_r * m_r;
    const double v_ii = (double)s->sum_im2 / n - m_i * m_i;
    const double v_ri = (double)s->sum_reim / n - m_r * m_i;
    if (!(v_rr > 0.0)) return fail("I/Q estimate: the real part has no variance");
    const double det = v_rr * v_ii - v_ri * v_ri;
    if (!(det > 0.0)) return fail("I/Q estimate: the parts are fully correlated (or the imaginary part has no variance)");
    const double gh = v_rr / std::sqrt(det);
    const double ph = -gh * v_ri / v_rr;
    p = std::rint(65536.0 * ph);
    g = std::rint(65536.0 * gh);
  }
  const double d_r = std::rint(m_r), d_i = std::rint(m_i);
  if (!(d_r >= -32768.0 && d_r <= 32767.0 && d_i >= -32768.0 && d_i <= 32767.0 && p >= -32768.0 && p <= 32768.0 && g >= 32768.0 &&
        g <= 131072.0))
    return fail("I/Q estimate: a word falls outside its range");
  out.dc_re = (int32_t)d_r; out.dc_im = (int32_t)d_i; out.cross_q16 = (int32_t)p; out.gain_q16 = (int32_t)g;
  *c = out;
  return 0;
}

int asdr_tuner_iq_track(asdr_tuner_t *t, int source) {
  if (!t) return fail("null tuner bank");
  if (source != ASDR_ALL && (source < 0 || source >= t->n_src)) return fail("source index out of range");
  std::vector<asdr_tuner_iq_stats_t> st(t->n_src);
  if (stats_read(t, st.data(), 1) != 0) return -1;
  int n_set = 0;
  for (int s = (source == ASDR_ALL ? 0 : source); s < (source == ASDR_ALL ? t->n_src : source + 1); s++) {
    asdr_tuner_iq_t c;
    if (asdr_tuner_iq_estimate(&st[s], &c) != 0) continue;   // this source keeps its correction
    set_correction(t, s, c);
    n_set++;
  }
  return n_set;
}

long long asdr_tuner_condition_launches(const asdr_tuner_t *t) { return t ? t->cond_launches : -1; }

}  // extern "C"

// ---- state records (include/asdr_tuner.h, "State records"; kernels: asdr_tuner_state.hip) -----------------------------------------
// A channel record = a 256-byte head (written and checked by the host) | the carry row (moved by the two kernels, which also move the
// level accumulator into / out of the head).  A bank-state blob is host work throughout: plain copies of the sources' rows.
namespace {

constexpr size_t kRec = ASDR_TUNER_CHANNEL_RECORD_BYTES, kHead = ASDR_TUNER_CHANNEL_OFF_CARRY;
constexpr int kRecChunk = 8192;   // records per staging round of the host forms (20 MB pinned + 20 MB of HBM)
static_assert(kRec == kHead + ASDR_TUNER_CARRY * sizeof(int32_t), "record layout");

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// a channel record's head, as the record has it
struct RecHead {
  uint32_t magic, version, bytes, content;
  int32_t kind, dr; int64_t fs_in; int32_t up, down; int64_t pos, out_pos; uint32_t pad0[2];
  int32_t src; uint32_t fw; int64_t pos_a; uint32_t ph_a; int32_t slot; float gain; uint32_t pad1;
  double level;
  uint32_t zero[38];
};
static_assert(sizeof(RecHead) == kHead && offsetof(RecHead, kind) == ASDR_TUNER_CHANNEL_OFF_ORIGIN &&
              offsetof(RecHead, src) == ASDR_TUNER_CHANNEL_OFF_CONTROL && offsetof(RecHead, level) == ASDR_TUNER_CHANNEL_OFF_LEVEL, "record head");

struct RecField { const char *name; int offset, count; };
const RecField kRecFields[] = {
  {"magic:u32", 0, 1}, {"version:u32", 4, 1}, {"bytes:u32", 8, 1}, {"content:u32", 12, 1},
  {"kind:i32", 16, 1}, {"decimation:i32", 20, 1}, {"fs_in:i64", 24, 1}, {"up:i32", 32, 1}, {"down:i32", 36, 1}, {"position:i64", 40, 1},
  {"output_position:i64", 48, 1}, {"pad0:u32", 56, 2},
  {"src:i32", 64, 1}, {"fw:u32", 68, 1}, {"pos_a:i64", 72, 1}, {"ph_a:u32", 80, 1}, {"slot:i32", 84, 1}, {"gain:f32", 88, 1}, {"pad1:u32", 92, 1},
  {"level:f64", 96, 1}, {"pad2:u32", 104, 38},
};

uint32_t rec_content(const asdr_tuner_t *t) {
  if (t->device == ASDR_NO_DEVICE) return 0u;
  return ASDR_TUNER_REC_HAS_SIGNAL | (pass_through(t) ? 0u : ASDR_TUNER_REC_HAS_CARRY) | (t->lev_on ? ASDR_TUNER_REC_HAS_LEVEL : 0u);
}

void head_of(const asdr_tuner_t *t, int ch, uint8_t *dst) {
  RecHead h;
  memset(&h, 0, sizeof h);
  h.magic = ASDR_TUNER_CHANNEL_MAGIC; h.version = ASDR_TUNER_STATE_VERSION; h.bytes = (uint32_t)kRec; h.content = rec_content(t);
  h.kind = t->fc ? 1 : 0; h.dr = t->D; h.fs_in = t->fs_in; h.up = t->up; h.down = t->down; h.pos = t->pos; h.out_pos = t->out_pos;
  const asdr_tuner_state_t &s = t->chan[ch];
  h.src = s.src; h.fw = s.fw; h.pos_a = s.pos_a; h.ph_a = s.ph_a;
  h.slot = t->fc ? t->slot[ch] : 0; h.gain = t->fc ? t->gain[ch] : 1.0f;
  memcpy(dst, &h, sizeof h);
}

// what keeps the record at p out of bank t, or ""
std::string head_error(const asdr_tuner_t *t, const uint8_t *p) {
  RecHead h;
  memcpy(&h, p, sizeof h);
  if (h.magic != ASDR_TUNER_CHANNEL_MAGIC) return "bad magic";
  if (h.version != ASDR_TUNER_STATE_VERSION) return "version mismatch (records are not portable across versions)";
  if (h.bytes != (uint32_t)kRec) return "wrong size in the `bytes` word";
  if (h.content & ~(ASDR_TUNER_REC_HAS_SIGNAL | ASDR_TUNER_REC_HAS_CARRY | ASDR_TUNER_REC_HAS_LEVEL)) return "unknown content bits";
  if ((h.content & (ASDR_TUNER_REC_HAS_CARRY | ASDR_TUNER_REC_HAS_LEVEL)) && !(h.content & ASDR_TUNER_REC_HAS_SIGNAL))
    return "content: carry or level flag without the signal part";
  if (h.kind != (t->fc ? 1 : 0)) return "taken from a bank of another kind (direct / rate against fast-convolution)";
  if (h.dr != t->D) return std::string("taken at another ") + (t->fc ? "R" : "decimation D");
  if (h.fs_in != t->fs_in) return "taken at another input rate Fs_in";
  if (h.up != t->up || h.down != t->down) return "taken at another resampling ratio U / M";
  if (h.pos != t->pos)
    return "taken at position P = " + std::to_string(h.pos) + ", the bank is at " + std::to_string(t->pos) + " (records move between banks at equal positions only)";
  if (h.out_pos != t->out_pos)
    return "taken at output position " + std::to_string(h.out_pos) + ", the bank is at " + std::to_string(t->out_pos);
  if (h.src < 0 || h.src >= t->n_src) return "source " + std::to_string(h.src) + " out of range (the bank has " + std::to_string(t->n_src) + ")";
  if (h.pos_a < 0 || h.pos_a > t->pos) return "anchor position outside 0 .. P";
  if (!std::isfinite(h.gain) || std::fabs(h.gain) > ASDR_TUNER_FC_MAX_GAIN) return "gain must be finite with |gain| <= 32768";
  if (t->fc) {
    if (h.slot < 0 || h.slot >= ASDR_TUNER_FC_MAX_FILTERS) return "palette slot must be in 0..63";
    if (h.slot != 0 && t->pal[h.slot].n == 0) return "palette slot " + std::to_string(h.slot) + " is undefined in this bank";
  } else {
    if (h.slot != 0) return "palette slot must be 0 on a bank without a palette";
    if (h.gain != 1.0f) return "gain must be 1 on a bank without channel gains";
  }
  return "";
}

// index checks of a call
int rec_indices(const asdr_tuner_t *t, const int *channels, int n, bool no_duplicates) {
  if (n < 1) return fail("n must be at least 1");
  if (!channels) return n > t->n ? fail("n exceeds the bank's channel count (channels == NULL names channels 0 .. n-1)") : 0;
  if (no_duplicates && n > t->n) return fail("more records than channels: a destination would be named twice");
  std::vector<uint8_t> seen(no_duplicates ? (size_t)t->n : 0, 0);
  for (int i = 0; i < n; i++) {
    const int c = channels[i];
    if (c < 0 || c >= t->n)
      return fail("record " + std::to_string(i) + ": channel " + std::to_string(c) + " out of range (0.." + std::to_string(t->n - 1) + ")");
    if (no_duplicates) {
      if (seen[c]) return fail("record " + std::to_string(i) + ": channel " + std::to_string(c) + " named twice");
      seen[c] = 1;
    }
  }
  return 0;
}

// every head of a call ([record i] at heads + i * stride) against the bank
int rec_check_all(const asdr_tuner_t *t, const int *channels, int n, const uint8_t *heads, size_t stride) {
  for (int i = 0; i < n; i++) {
    const std::string why = head_error(t, heads + (size_t)i * stride);
    if (!why.empty()) return fail("record " + std::to_string(i) + " (channel " + std::to_string(channels ? channels[i] : i) + "): " + why);
  }
  return 0;
}

// the host half of an import (every record has been checked): rows, slots, gains, dirty marks
void rec_host_half(asdr_tuner_t *t, const int *channels, int n, const uint8_t *heads, size_t stride) {
  for (int i = 0; i < n; i++) {
    RecHead h;
    memcpy(&h, heads + (size_t)i * stride, sizeof h);
    const int c = channels ? channels[i] : i;
    asdr_tuner_state_t s = fresh_state();
    s.src = h.src; s.fw = h.fw; s.pos_a = h.pos_a; s.ph_a = h.ph_a;
    t->chan[c] = s;
    if (t->fc) { t->slot[c] = h.slot; t->gain[c] = h.gain; }
  }
  t->chan_dirty = t->order_dirty = true;
  if (t->fc) {
    t->sg_dirty = true;
    t->n_off = 0;
    for (int c = 0; c < t->n; c++) t->n_off += (t->slot[c] != 0 || t->gain[c] != 1.0f);
  }
}

int rec_stage_reserve(asdr_tuner_t *t, size_t h_bytes, size_t d_bytes) {
  if (!t->st_ev) HIPCHK(hipEventCreateWithFlags(&t->st_ev, hipEventDisableTiming));
  if (t->st_ev_pending) { HIPCHK(hipEventSynchronize(t->st_ev)); t->st_ev_pending = false; }   // the pinned half is free again
  if (h_bytes > t->st_h_cap) {
    if (t->st_h) { HIPCHK(hipHostFree(t->st_h)); t->st_h = nullptr; t->st_h_cap = 0; }
    HIPCHK(hipHostMalloc((void **)&t->st_h, h_bytes, hipHostMallocDefault));
    t->st_h_cap = h_bytes;
  }
  return stage_reserve(*t, (void **)&t->st_d, &t->st_d_cap, d_bytes);
}

// behind a device form's work on `stream`, which stage_before_launch put in the bank's stream order: the next call on any stream is
// ordered after it.  On a bank that never launched this records the start event too (asdr_tuner_last_kernel_ms reads both)
int rec_order_out(asdr_tuner_t *t, hipStream_t stream) {
  if (!t->ev_valid && stage_mark_start(*t, stream) != 0) return -1;
  return stage_after_launch(*t, stream);
}

// the carry the gather reads: the current rows, or none while they are logically zero or do not exist
int32_t *live_carry(const asdr_tuner_t *t) { return (!pass_through(t) && !t->carry_stale) ? t->d_carry[t->ccur] : nullptr; }

// entries e0 .. e0 + m - 1 of an export into records rec0 .. of d_records, on `stream` (which is in the bank's order)
int rec_gather(asdr_tuner_t *t, const int *channels, int e0, int m, int rec0, void *d_records, hipStream_t stream) {
  const size_t head_bytes = (size_t)m * kHead, list_bytes = channels ? (size_t)m * 2 * sizeof(int) : 0;
  if (rec_stage_reserve(t, head_bytes + list_bytes, head_bytes + list_bytes) != 0) return -1;
  for (int i = 0; i < m; i++) head_of(t, channels ? channels[e0 + i] : e0 + i, t->st_h + (size_t)i * kHead);
  int *list = reinterpret_cast<int *>(t->st_h + head_bytes);
  if (channels) for (int i = 0; i < m; i++) { list[2 * i] = channels[e0 + i]; list[2 * i + 1] = rec0 + i; }
  HIPCHK(hipMemcpyAsync(t->st_d, t->st_h, head_bytes + list_bytes, hipMemcpyHostToDevice, stream));
  TunerStateArgs a;
  a.carry = live_carry(t); a.level = t->lev_on ? t->d_lev : nullptr;
  if (asdr_launch_tuner_state_gather(&a, channels ? reinterpret_cast<const int *>(t->st_d + head_bytes) : nullptr, m, e0, rec0, d_records, t->st_d, stream) != 0)
    return fail("tuner state gather kernel launch failed");
  HIPCHK(hipEventRecord(t->st_ev, stream)); t->st_ev_pending = true;
  return 0;
}

// Before the scatter of an import into a bank with a real stage 2: the carry exists and holds what it logically holds.
int rec_carry_ready(asdr_tuner_t *t, hipStream_t stream) {
  const size_t cb = (size_t)t->n * ASDR_TUNER_CARRY * sizeof(int32_t);
  if (!t->d_carry[0] || !t->d_carry[1]) {   // as rate_device allocates it: nothing of ours may be in flight
    if (asdr_tuner_synchronize(t) != 0) return -1;
    if (!t->d_carry[0]) HIPCHK(hipMalloc(&t->d_carry[0], cb));
    if (!t->d_carry[1]) HIPCHK(hipMalloc(&t->d_carry[1], cb));
    HIPCHK(hipMemset(t->d_carry[t->ccur], 0, cb));
    HIPCHK(hipDeviceSynchronize());
    t->carry_stale = false;
  } else if (t->carry_stale) {
    HIPCHK(hipMemsetAsync(t->d_carry[t->ccur], 0, cb, stream));
    t->carry_stale = false;
  }
  return 0;
}

// entries e0 .. e0 + m - 1 of an import from records rec0 .. of d_records, on `stream`; the list (if any) goes through the staging
// area past `keep` bytes of it
int rec_scatter(asdr_tuner_t *t, const int *channels, int e0, int m, int rec0, const void *d_records, size_t keep, hipStream_t stream) {
  const size_t list_bytes = channels ? (size_t)m * 2 * sizeof(int) : 0;
  if (list_bytes) {
    int *list = reinterpret_cast<int *>(t->st_h + keep);
    for (int i = 0; i < m; i++) { list[2 * i] = channels[e0 + i]; list[2 * i + 1] = rec0 + i; }
    HIPCHK(hipMemcpyAsync(t->st_d + keep, list, list_bytes, hipMemcpyHostToDevice, stream));
  }
  TunerStateArgs a;
  a.carry = pass_through(t) ? nullptr : t->d_carry[t->ccur]; a.level = t->lev_on ? t->d_lev : nullptr;
  if (!a.carry && !a.level) return 0;   // nothing of the channel lives on the device
  if (asdr_launch_tuner_state_scatter(&a, list_bytes ? reinterpret_cast<const int *>(t->st_d + keep) : nullptr, m, e0, rec0, d_records, stream) != 0)
    return fail("tuner state scatter kernel launch failed");
  if (list_bytes) { HIPCHK(hipEventRecord(t->st_ev, stream)); t->st_ev_pending = true; }
  return 0;
}

// ---- the bank-state blob
constexpr size_t kBlobHead = ASDR_TUNER_BLOB_HEADER_BYTES, kPalEntry = 16 + 2 * ASDR_TUNER_FC_MAX_TAPS * sizeof(float) + 8;   // 1056
enum { BS_FILTER, BS_RESAMPLER, BS_PALETTE, BS_CORR, BS_STATS, BS_SPECTRUM, BS_HISTORY, BS_UNUSED, BS_COUNT };
struct BlobHead {
  uint32_t magic, version; uint64_t bytes;
  uint32_t content; int32_t kind, dr, n_src;
  int64_t fs_in; int32_t up, down; int64_t pos, out_pos;
  int32_t fmt, hist_slots, g, n_taps, g2, k2;
  int32_t spec_bins, spec_win, spec_mode, lev_on;
  int64_t spec_frames, lev_frames; int32_t iq_stats_on; uint32_t pad;
  struct { uint64_t offset, bytes; } dir[BS_COUNT];
};
static_assert(sizeof(BlobHead) == kBlobHead && offsetof(BlobHead, dir) == 128 && offsetof(BlobHead, fmt) == 64 &&
              offsetof(BlobHead, spec_frames) == 104, "blob header");
static_assert(kPalEntry % 16 == 0, "palette entry");

// the directory that the header's own fields ask for (offsets back to back from kBlobHead); returns the total size
uint64_t blob_layout(BlobHead &h) {
  const bool fc = h.kind == 1, sig = (h.content & ASDR_TUNER_BLOB_HAS_SIGNAL) != 0u;
  uint64_t sz[BS_COUNT];
  sz[BS_FILTER] = fc ? up16(ASDR_TUNER_FC_MAX_TAPS * sizeof(float)) : ASDR_TUNER_MAX_TAPS * sizeof(int16_t);
  sz[BS_RESAMPLER] = (uint64_t)h.up * ASDR_TUNER_MAX_RESAMPLER_TAPS * sizeof(int16_t);
  sz[BS_PALETTE] = fc ? (ASDR_TUNER_FC_MAX_FILTERS - 1) * kPalEntry : 0;
  sz[BS_CORR] = (uint64_t)h.n_src * sizeof(asdr_tuner_iq_t);
  sz[BS_STATS] = sig && h.iq_stats_on ? up16((uint64_t)h.n_src * sizeof(asdr_tuner_iq_stats_t)) : 0;
  sz[BS_SPECTRUM] = sig ? (uint64_t)h.n_src * (uint64_t)h.spec_bins * sizeof(double) : 0;
  sz[BS_HISTORY] = sig ? (uint64_t)h.n_src * (uint64_t)h.hist_slots * sizeof(int32_t) : 0;
  sz[BS_UNUSED] = 0;
  uint64_t off = kBlobHead;
  for (int k = 0; k < BS_COUNT; k++) {
    h.dir[k].offset = sz[k] ? off : 0; h.dir[k].bytes = sz[k];
    off += up16(sz[k]);
  }
  return off;
}

void blob_header(const asdr_tuner_t *t, BlobHead &h) {
  memset(&h, 0, sizeof h);
  h.magic = ASDR_TUNER_BANK_MAGIC; h.version = ASDR_TUNER_STATE_VERSION;
  h.content = (t->device != ASDR_NO_DEVICE ? ASDR_TUNER_BLOB_HAS_SIGNAL : 0u) | (t->carry_stale ? ASDR_TUNER_BLOB_CARRY_STALE : 0u);
  h.kind = t->fc ? 1 : 0; h.dr = t->D; h.n_src = t->n_src;
  h.fs_in = t->fs_in; h.up = t->up; h.down = t->down; h.pos = t->pos; h.out_pos = t->out_pos;
  h.fmt = t->fmt; h.hist_slots = t->hist_slots; h.g = t->fc ? 0 : t->g; h.n_taps = (int32_t)(t->fc ? t->gch.size() : t->h.size());
  h.g2 = t->g2; h.k2 = t->k2;
  h.spec_bins = t->spec_bins; h.spec_win = t->spec_bins ? t->spec_win : 0; h.spec_mode = t->spec_bins ? t->spec_mode : 0;
  h.lev_on = t->lev_on ? 1 : 0;
  h.spec_frames = t->spec_bins ? t->spec_frames : 0; h.lev_frames = t->lev_on ? t->lev_frames : 0; h.iq_stats_on = t->iq_stats_on ? 1 : 0;
  h.bytes = blob_layout(h);
}

// what is wrong with the blob (for a bank of this geometry: t may be NULL, create_from_bank_state checks the geometry by creating), or ""
std::string blob_error(const asdr_tuner_t *t, const uint8_t *p, size_t bytes) {
  if (bytes < kBlobHead) return "truncated: shorter than the header";
  BlobHead h;
  memcpy(&h, p, sizeof h);
  if (h.magic != ASDR_TUNER_BANK_MAGIC) return "bad magic";
  if (h.version != ASDR_TUNER_STATE_VERSION) return "version mismatch (blobs are not portable across versions)";
  if (h.content & ~(ASDR_TUNER_BLOB_HAS_SIGNAL | ASDR_TUNER_BLOB_CARRY_STALE)) return "unknown content bits";
  if (h.kind != 0 && h.kind != 1) return "unknown bank kind";
  if (h.n_src < 1 || h.n_src > 65535) return "n_sources out of range";
  if (h.up < 1 || h.up > ASDR_TUNER_MAX_UP || h.down < 1) return "resampling ratio out of range";
  if (h.dr < 1 || h.dr > ASDR_TUNER_FC_MAX_R) return "decimation out of range";
  if (t) {
    if (h.kind != (t->fc ? 1 : 0)) return "taken from a bank of another kind (direct / rate against fast-convolution)";
    if (h.dr != t->D) return std::string("taken at another ") + (t->fc ? "R" : "decimation D");
    if (h.fs_in != t->fs_in) return "taken at another input rate Fs_in";
    if (h.up != t->up || h.down != t->down) return "taken at another resampling ratio U / M";
    if (h.n_src != t->n_src) return "taken from a bank of " + std::to_string(h.n_src) + " sources, this one has " + std::to_string(t->n_src);
  }
  const bool fc = h.kind == 1;
  if (h.hist_slots != (fc ? 128 * h.dr : ASDR_TUNER_HIST_SLOTS)) return "history length does not follow the geometry";
  if (h.spec_bins < 0 || h.spec_bins > 256 * ASDR_TUNER_FC_MAX_R) return "spectrum bins out of range";
  BlobHead want = h;
  const uint64_t total = blob_layout(want);
  if (h.bytes != total) return "the `bytes` word does not follow the header's fields";
  if (bytes < total) return "truncated: " + std::to_string(bytes) + " bytes of " + std::to_string(total);
  if (memcmp(want.dir, h.dir, sizeof h.dir) != 0) return "the section directory does not follow the header's fields";
  if (h.fmt < ASDR_TUNER_IN_CS16 || h.fmt > ASDR_TUNER_IN_RS16) return "unknown input format";
  const long long frame = 128LL * h.dr;
  if (h.pos < 0 || h.pos % frame != 0) return "position P is not a frame boundary";
  if (h.out_pos < 0 || h.out_pos % 128 != 0) return "output position is not a block boundary";
  if (h.pad != 0) return "pad word not zero";
  if (fc) {
    if (h.n_taps < 1 || h.n_taps > ASDR_TUNER_FC_MAX_TAPS) return "channel filter length must be in 1..129";
    if (h.g != 0) return "a fast-convolution bank has no stage-1 gain shift";
    const float *g = reinterpret_cast<const float *>(p + h.dir[BS_FILTER].offset);
    for (int k = 0; k < h.n_taps; k++) if (!std::isfinite(g[k])) return "channel filter taps must be finite";
    for (int k = 1; k < ASDR_TUNER_FC_MAX_FILTERS; k++) {
      const uint8_t *e = p + h.dir[BS_PALETTE].offset + (size_t)(k - 1) * kPalEntry;
      int32_t n, cx;
      memcpy(&n, e, 4); memcpy(&cx, e + 4, 4);
      if (n < 0 || n > ASDR_TUNER_FC_MAX_TAPS || (cx != 0 && cx != 1)) return "palette slot " + std::to_string(k) + ": tap count or complex flag out of range";
      const float *taps = reinterpret_cast<const float *>(e + 16);
      for (int i = 0; i < (cx ? 2 * n : n); i++) if (!std::isfinite(taps[i])) return "palette slot " + std::to_string(k) + ": taps must be finite";
    }
    if (h.spec_bins != 0) {
      if (h.spec_bins < 256 || h.spec_bins > 256 * h.dr || (h.spec_bins & (h.spec_bins - 1)) != 0) return "spectrum bins must be 0 or a power of two in 256..N";
      if (h.spec_win != ASDR_TUNER_WIN_RECT && h.spec_win != ASDR_TUNER_WIN_HANN) return "unknown spectrum window";
      if (h.spec_mode != ASDR_TUNER_MON_SUM && h.spec_mode != ASDR_TUNER_MON_PEAK) return "unknown spectrum mode";
    }
  } else {
    if (h.n_taps < 1 || h.n_taps > ASDR_TUNER_MAX_TAPS) return "filter length must be in 1..1024";
    if (h.g < 0 || h.g > ASDR_TUNER_MAX_GAIN_SHIFT) return "gain shift must be in 0..15";
    const int16_t *f = reinterpret_cast<const int16_t *>(p + h.dir[BS_FILTER].offset);
    long sum = 0;
    for (int k = 0; k < h.n_taps; k++) sum += std::labs((long)f[k]);
    if (sum > 65535) return "sum of |h| exceeds 65535";
    if (h.spec_bins != 0 || h.lev_on != 0) return "only a fast-convolution bank has monitors";
  }
  if (h.lev_on != 0 && h.lev_on != 1) return "the levels switch is neither 0 nor 1";
  if (h.iq_stats_on != 0 && h.iq_stats_on != 1) return "the statistics switch is neither 0 nor 1";
  if (h.spec_frames < 0 || h.lev_frames < 0) return "negative frame count";
  if (h.k2 < 1 || h.k2 > ASDR_TUNER_MAX_RESAMPLER_TAPS) return "resampler taps per phase (K) must be in 1..64";
  const std::string e2 = resampler_error(h.up, reinterpret_cast<const int16_t *>(p + h.dir[BS_RESAMPLER].offset), h.up * h.k2, h.g2);
  if (!e2.empty()) return e2;
  for (int s = 0; s < h.n_src; s++) {
    asdr_tuner_iq_t c;
    memcpy(&c, p + h.dir[BS_CORR].offset + (size_t)s * sizeof c, sizeof c);
    const std::string ec = correction_error(c);
    if (!ec.empty()) return "source " + std::to_string(s) + ": " + ec;
  }
  return "";
}

}  // namespace

extern "C" {

size_t asdr_tuner_channel_record_bytes(void) { return kRec; }

const char *asdr_tuner_channel_record_field(int i, int *offset, int *count) {
  if (i < 0 || i >= (int)(sizeof kRecFields / sizeof kRecFields[0])) return nullptr;
  if (offset) *offset = kRecFields[i].offset;
  if (count) *count = kRecFields[i].count;
  return kRecFields[i].name;
}

int asdr_tuner_export_channels(asdr_tuner_t *t, const int *channels, int n, void *host_records) {
  if (!t) return fail("null tuner bank");
  if (rec_indices(t, channels, n, false) != 0) return -1;
  if (!host_records) return fail("null records");
  uint8_t *out = static_cast<uint8_t *>(host_records);
  if (t->device == ASDR_NO_DEVICE) {
    for (int i = 0; i < n; i++) {
      head_of(t, channels ? channels[i] : i, out + (size_t)i * kRec);
      memset(out + (size_t)i * kRec + kHead, 0, kRec - kHead);
    }
    return 0;
  }
  HIPCHK(hipSetDevice(t->device));
  if (asdr_tuner_synchronize(t) != 0) return -1;
  for (int e0 = 0; e0 < n; e0 += kRecChunk) {
    const int m = std::min(kRecChunk, n - e0);
    const size_t rec_bytes = (size_t)m * kRec, extra = up16((size_t)m * (kHead + 2 * sizeof(int)));
    if (rec_stage_reserve(t, rec_bytes + extra, rec_bytes + extra) != 0) return -1;
    // heads and list behind the chunk's records in both staging halves: rec_gather stages at the front, so gather into the back
    uint8_t *d_rec = t->st_d + extra;
    if (rec_gather(t, channels, e0, m, 0, d_rec, t->stream) != 0) return -1;
    HIPCHK(hipMemcpyAsync(t->st_h + extra, d_rec, rec_bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    memcpy(out + (size_t)e0 * kRec, t->st_h + extra, rec_bytes);
  }
  return 0;
}

int asdr_tuner_export_channels_device(asdr_tuner_t *t, const int *channels, int n, void *d_records, void *stream_) {
  if (!t) return fail("null tuner bank");
  if (rec_indices(t, channels, n, false) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail("control-plane-only tuner bank (ASDR_NO_DEVICE) has no device: use asdr_tuner_export_channels");
  if (!d_records || ((uintptr_t)d_records & 15u) != 0) return fail("device records: null or not 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(t->device));
  if (rec_stage_reserve(t, (size_t)n * (kHead + 2 * sizeof(int)), (size_t)n * (kHead + 2 * sizeof(int))) != 0) return -1;
  if (stage_before_launch(*t, stream) != 0) return -1;
  if (rec_gather(t, channels, 0, n, 0, d_records, stream) != 0) return -1;
  return rec_order_out(t, stream);
}

int asdr_tuner_import_channels(asdr_tuner_t *t, const int *channels, int n, const void *host_records) {
  if (!t) return fail("null tuner bank");
  if (rec_indices(t, channels, n, true) != 0) return -1;
  if (!host_records) return fail("null records");
  const uint8_t *in = static_cast<const uint8_t *>(host_records);
  if (rec_check_all(t, channels, n, in, kRec) != 0) return -1;
  if (t->device != ASDR_NO_DEVICE && (!pass_through(t) || t->lev_on)) {
    HIPCHK(hipSetDevice(t->device));
    if (asdr_tuner_synchronize(t) != 0) return -1;
    if (!pass_through(t) && rec_carry_ready(t, t->stream) != 0) return -1;
    for (int e0 = 0; e0 < n; e0 += kRecChunk) {
      const int m = std::min(kRecChunk, n - e0);
      const size_t rec_bytes = (size_t)m * kRec, list_bytes = (size_t)m * 2 * sizeof(int);
      if (rec_stage_reserve(t, rec_bytes + list_bytes, rec_bytes + list_bytes) != 0) return -1;
      memcpy(t->st_h, in + (size_t)e0 * kRec, rec_bytes);
      HIPCHK(hipMemcpyAsync(t->st_d, t->st_h, rec_bytes, hipMemcpyHostToDevice, t->stream));
      if (rec_scatter(t, channels, e0, m, 0, t->st_d, rec_bytes, t->stream) != 0) return -1;
      HIPCHK(hipStreamSynchronize(t->stream));
    }
  }
  rec_host_half(t, channels, n, in, kRec);
  return 0;
}

int asdr_tuner_import_channels_device(asdr_tuner_t *t, const int *channels, int n, const void *d_records, void *stream_) {
  if (!t) return fail("null tuner bank");
  if (rec_indices(t, channels, n, true) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail("control-plane-only tuner bank (ASDR_NO_DEVICE) has no device: use asdr_tuner_import_channels");
  if (!d_records || ((uintptr_t)d_records & 15u) != 0) return fail("device records: null or not 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(t->device));
  const size_t head_bytes = (size_t)n * kHead, list_bytes = (size_t)n * 2 * sizeof(int);
  if (rec_stage_reserve(t, head_bytes + list_bytes, head_bytes + list_bytes) != 0) return -1;
  // every record's head to the host: validated before any launch (this waits for the work in front of it on `stream`)
  HIPCHK(hipMemcpy2DAsync(t->st_h, kHead, d_records, kRec, kHead, (size_t)n, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (rec_check_all(t, channels, n, t->st_h, kHead) != 0) return -1;
  if (!pass_through(t) || t->lev_on) {
    if (stage_before_launch(*t, stream) != 0) return -1;
    if (!pass_through(t) && rec_carry_ready(t, stream) != 0) return -1;
    if (rec_scatter(t, channels, 0, n, 0, d_records, head_bytes, stream) != 0) return -1;
    if (rec_order_out(t, stream) != 0) return -1;
  }
  rec_host_half(t, channels, n, t->st_h, kHead);
  return 0;
}

size_t asdr_tuner_bank_state_bytes(const asdr_tuner_t *t) {
  if (!t) return 0;
  BlobHead h;
  blob_header(t, h);
  return (size_t)h.bytes;
}

int asdr_tuner_export_bank_state(asdr_tuner_t *t, void *host, size_t capacity) {
  if (!t) return fail("null tuner bank");
  if (!host) return fail("null destination");
  BlobHead h;
  blob_header(t, h);
  if (capacity < h.bytes) return fail("bank state: capacity of " + std::to_string(capacity) + " bytes, the blob has " + std::to_string(h.bytes));
  uint8_t *p = static_cast<uint8_t *>(host);
  if (t->device != ASDR_NO_DEVICE) {
    HIPCHK(hipSetDevice(t->device));
    if (asdr_tuner_synchronize(t) != 0) return -1;
  }
  memset(p, 0, (size_t)h.dir[BS_HISTORY].bytes ? (size_t)h.dir[BS_HISTORY].offset : (size_t)h.bytes);   // pads and unused taps (the history has none)
  memcpy(p, &h, sizeof h);
  if (t->fc) {
    memcpy(p + h.dir[BS_FILTER].offset, t->gch.data(), t->gch.size() * sizeof(float));
    for (int k = 1; k < ASDR_TUNER_FC_MAX_FILTERS; k++) {
      const asdr_tuner_bank::PaletteSlot &s = t->pal[k];
      uint8_t *e = p + h.dir[BS_PALETTE].offset + (size_t)(k - 1) * kPalEntry;
      const int32_t n = s.n, cx = s.n && s.cx ? 1 : 0;
      memcpy(e, &n, 4); memcpy(e + 4, &cx, 4);
      if (n) memcpy(e + 16, s.taps.data(), (size_t)(cx ? 2 * n : n) * sizeof(float));
    }
  } else {
    memcpy(p + h.dir[BS_FILTER].offset, t->h.data(), t->h.size() * sizeof(int16_t));
  }
  memcpy(p + h.dir[BS_RESAMPLER].offset, t->h2.data(), t->h2.size() * sizeof(int16_t));
  memcpy(p + h.dir[BS_CORR].offset, t->corr.data(), (size_t)t->n_src * sizeof(asdr_tuner_iq_t));
  if (h.dir[BS_STATS].bytes) HIPCHK(hipMemcpy(p + h.dir[BS_STATS].offset, t->d_iq_stats, (size_t)t->n_src * sizeof(asdr_tuner_iq_stats_t), hipMemcpyDeviceToHost));
  if (h.dir[BS_SPECTRUM].bytes) HIPCHK(hipMemcpy(p + h.dir[BS_SPECTRUM].offset, t->d_spec, (size_t)h.dir[BS_SPECTRUM].bytes, hipMemcpyDeviceToHost));
  if (h.dir[BS_HISTORY].bytes) HIPCHK(hipMemcpy(p + h.dir[BS_HISTORY].offset, t->d_hist[t->cur], (size_t)h.dir[BS_HISTORY].bytes, hipMemcpyDeviceToHost));
  return 0;
}

int asdr_tuner_import_bank_state(asdr_tuner_t *t, const void *host, size_t bytes) {
  if (!t) return fail("null tuner bank");
  if (!host) return fail("null bank state");
  const uint8_t *p = static_cast<const uint8_t *>(host);
  const std::string why = blob_error(t, p, bytes);
  if (!why.empty()) return fail("bank state: " + why);
  BlobHead h;
  memcpy(&h, p, sizeof h);
  const bool dev = t->device != ASDR_NO_DEVICE, sig = (h.content & ASDR_TUNER_BLOB_HAS_SIGNAL) != 0u;
  if (asdr_tuner_reset(t) != 0) return -1;
  // the monitors and the statistics first: what can fail here (an allocation) fails with the bank in its reset state
  if (asdr_tuner_iq_stats_enable(t, h.iq_stats_on) != 0) return -1;
  if (t->fc) {
    if (asdr_tuner_spectrum_enable(t, h.spec_bins, h.spec_win, h.spec_mode) != 0) return -1;
    if (asdr_tuner_levels_enable(t, h.lev_on) != 0) return -1;
  }
  t->pos = h.pos; t->out_pos = h.out_pos; t->fmt = h.fmt;
  t->carry_stale = (h.content & ASDR_TUNER_BLOB_CARRY_STALE) != 0u;
  if (t->fc) {
    const float *g = reinterpret_cast<const float *>(p + h.dir[BS_FILTER].offset);
    t->gch.assign(g, g + h.n_taps);
    t->g_dirty = true;
    for (int k = 1; k < ASDR_TUNER_FC_MAX_FILTERS; k++) {
      const uint8_t *e = p + h.dir[BS_PALETTE].offset + (size_t)(k - 1) * kPalEntry;
      int32_t n, cx;
      memcpy(&n, e, 4); memcpy(&cx, e + 4, 4);
      asdr_tuner_bank::PaletteSlot s;
      if (n) { const float *taps = reinterpret_cast<const float *>(e + 16); s.taps.assign(taps, taps + (cx ? 2 * n : n)); s.cx = cx != 0; s.n = n; }
      t->pal[k] = s;
    }
    t->pal_dirty = ~0ull;
    t->spec_frames = h.spec_bins ? h.spec_frames : 0; t->lev_frames = h.lev_on ? h.lev_frames : 0;
  } else {
    const int16_t *f = reinterpret_cast<const int16_t *>(p + h.dir[BS_FILTER].offset);
    t->h.assign(f, f + h.n_taps);
    t->g = h.g;
    t->taps_dirty = true;
  }
  const int16_t *h2 = reinterpret_cast<const int16_t *>(p + h.dir[BS_RESAMPLER].offset);
  t->h2.assign(h2, h2 + (size_t)h.up * h.k2);
  t->g2 = h.g2; t->k2 = h.k2; t->rs_dirty = true;
  for (int s = 0; s < t->n_src; s++) {
    asdr_tuner_iq_t c;
    memcpy(&c, p + h.dir[BS_CORR].offset + (size_t)s * sizeof c, sizeof c);
    set_correction(t, s, c);
  }
  if (dev && sig) {
    HIPCHK(hipSetDevice(t->device));
    if (h.dir[BS_STATS].bytes) HIPCHK(hipMemcpy(t->d_iq_stats, p + h.dir[BS_STATS].offset, (size_t)t->n_src * sizeof(asdr_tuner_iq_stats_t), hipMemcpyHostToDevice));
    if (h.dir[BS_SPECTRUM].bytes) HIPCHK(hipMemcpy(t->d_spec, p + h.dir[BS_SPECTRUM].offset, (size_t)h.dir[BS_SPECTRUM].bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(t->d_hist[t->cur], p + h.dir[BS_HISTORY].offset, (size_t)h.dir[BS_HISTORY].bytes, hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
  }
  return 0;
}

asdr_tuner_t *asdr_tuner_create_from_bank_state(const void *host, size_t bytes, int n_channels, int device) {
  if (!host) { fail("null bank state"); return nullptr; }
  const uint8_t *p = static_cast<const uint8_t *>(host);
  const std::string why = blob_error(nullptr, p, bytes);
  if (!why.empty()) { fail("bank state: " + why); return nullptr; }
  BlobHead h;
  memcpy(&h, p, sizeof h);
  asdr_tuner_t *t = h.kind == 1 ? create_fastconv(n_channels, h.n_src, h.fs_in, h.dr, device) : create_bank(n_channels, h.n_src, h.fs_in, h.dr, device);
  if (!t) return nullptr;
  if (asdr_tuner_import_bank_state(t, host, bytes) != 0) { asdr_tuner_destroy(t); return nullptr; }   // (this checks U / M against the new bank's)
  return t;
}

}  // extern "C"
