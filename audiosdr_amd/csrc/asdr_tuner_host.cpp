// asdr_tuner_host.cpp -- host side + C ABI (include/asdr_tuner.h) of the digital tuner bank.  The control plane lives in a host
// mirror (channel anchors, the source-sorted schedule, the polyphase taps) that is pushed before a launch when a setter touched it;
// the per-source history rows live on the device only, double-buffered so that the launch that reads one writes the other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "asdr_tuner_device.h"

int asdr_internal_fail(const std::string &m);   // asdr_host.cpp: sets the thread's asdr_last_error() text, returns -1

namespace {
int fail(const std::string &m) { return asdr_internal_fail(m); }
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

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

// The default filter (asdr_tuner.h): D = 1 -> {16384}, g = 1; D >= 2 -> a Kaiser-windowed sinc of 12 D + 1 taps (beta 9, cut-off
// midway between 11.2 kHz and 32.1 kHz), normalised to unit DC gain and rounded to Q15, g = 0.  Its measured response: DESIGN.md 3.8.
void default_filter(int D, std::vector<int16_t> &h, int &g) {
  if (D == 1) { h.assign(1, 16384); g = 1; return; }
  const int L = 12 * D + 1, M = L - 1;
  const double fc = 0.5 * (11200.0 + 32100.0) / (44100.0 * D), beta = 9.0, pi = 3.14159265358979323846;
  std::vector<double> w(L);
  double sum = 0.0;
  for (int n = 0; n < L; n++) {
    const double x = n - 0.5 * M, u = 2.0 * n / M - 1.0;
    const double s = (x == 0.0) ? 2.0 * fc : std::sin(2.0 * pi * fc * x) / (pi * x);
    w[n] = s * bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - u * u))) / bessel_i0(beta);
    sum += w[n];
  }
  h.resize(L);
  for (int n = 0; n < L; n++) h[n] = (int16_t)std::llround(32768.0 * w[n] / sum);
  g = 0;
}
}  // namespace

struct asdr_tuner_bank {
  int n = 0, n_src = 0, D = 1, device = ASDR_NO_DEVICE;
  long long pos = 0;
  std::vector<asdr_tuner_state_t> chan;
  std::vector<int32_t> order;
  std::vector<int16_t> h;
  int g = 0;
  bool chan_dirty = true, order_dirty = true, taps_dirty = true;
  // device
  asdr_tuner_state_t *d_chan = nullptr;
  int32_t *d_order = nullptr, *d_taps = nullptr, *d_hist[2] = {nullptr, nullptr};
  int cur = 0;                        // d_hist[cur] holds the samples before pos
  int n_rows = 1, n_pairs = 1;        // A, DP2 of the pushed taps
  hipStream_t stream = nullptr, last_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_valid = false;
  void *d_io = nullptr;               // staging for asdr_tuner_update
  size_t io_cap = 0;
};

namespace {
asdr_tuner_state_t fresh_state() {
  asdr_tuner_state_t s;
  memset(&s, 0, sizeof s);
  return s;
}
uint32_t theta_at(const asdr_tuner_state_t &s, long long pos) { return s.ph_a + (uint32_t)(uint64_t)(pos - s.pos_a) * s.fw; }

// one retune of channel `ch` (or every channel): re-anchor at P with a continuous phase, then apply f
template <typename F>
int retune(asdr_tuner_t *t, int ch, F f) {
  if (!t) return fail("null tuner bank");
  if (ch != ASDR_ALL && (ch < 0 || ch >= t->n)) return fail("bad channel");
  for (int i = (ch == ASDR_ALL ? 0 : ch); i < (ch == ASDR_ALL ? t->n : ch + 1); i++) {
    asdr_tuner_state_t &s = t->chan[i];
    s.ph_a = theta_at(s, t->pos);
    s.pos_a = t->pos;
    f(s);
  }
  t->chan_dirty = true;
  return 0;
}

int push(asdr_tuner_t *t, hipStream_t stream) {
  if (!t->chan_dirty && !t->order_dirty && !t->taps_dirty) return 0;
  if (t->order_dirty) {
    t->order.resize(t->n);
    for (int i = 0; i < t->n; i++) t->order[i] = i;
    std::stable_sort(t->order.begin(), t->order.end(), [t](int a, int b) { return t->chan[a].src < t->chan[b].src; });
    HIPCHK(hipMemcpyAsync(t->d_order, t->order.data(), t->n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  }
  std::vector<int32_t> taps;
  if (t->taps_dirty) {
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
  return 0;
}

bool overlap(uintptr_t a0, size_t an, uintptr_t b0, size_t bn) { return a0 < b0 + bn && b0 < a0 + an; }
}  // namespace

extern "C" {

asdr_tuner_t *asdr_tuner_create(int n_channels, int n_sources, int decimation, int device) {
  if (n_channels <= 0 || n_channels > (1 << 20)) { fail("n_channels must be in 1..1048576"); return nullptr; }
  if (n_sources <= 0 || n_sources > 65535) { fail("n_sources must be in 1..65535"); return nullptr; }
  if (decimation < 1 || decimation > ASDR_TUNER_MAX_DECIMATION) { fail("decimation must be in 1..64"); return nullptr; }
  asdr_tuner_bank *t = new asdr_tuner_bank();
  t->n = n_channels; t->n_src = n_sources; t->D = decimation; t->device = device;
  t->chan.assign(n_channels, fresh_state());
  default_filter(decimation, t->h, t->g);
  if (device == ASDR_NO_DEVICE) return t;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { fail("no HIP device: this library has no CPU fallback"); delete t; return nullptr; }
  if (device < 0 || device >= count) { fail("bad device index"); delete t; return nullptr; }
  const size_t hist = (size_t)n_sources * ASDR_TUNER_HIST_SLOTS * sizeof(int32_t);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&t->stream) != hipSuccess || hipEventCreate(&t->ev0) != hipSuccess ||
      hipEventCreate(&t->ev1) != hipSuccess || hipMalloc(&t->d_chan, n_channels * sizeof(asdr_tuner_state_t)) != hipSuccess ||
      hipMalloc(&t->d_order, n_channels * sizeof(int32_t)) != hipSuccess || hipMalloc(&t->d_taps, kTapWords * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&t->d_hist[0], hist) != hipSuccess || hipMalloc(&t->d_hist[1], hist) != hipSuccess ||
      hipMemset(t->d_hist[0], 0, hist) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fail("tuner bank: device allocation failed");
    asdr_tuner_destroy(t);
    return nullptr;
  }
  return t;
}

void asdr_tuner_destroy(asdr_tuner_t *t) {
  if (!t) return;
  if (t->device != ASDR_NO_DEVICE) {
    hipSetDevice(t->device);
    hipDeviceSynchronize();
    hipFree(t->d_chan); hipFree(t->d_order); hipFree(t->d_taps); hipFree(t->d_hist[0]); hipFree(t->d_hist[1]); hipFree(t->d_io);
    if (t->ev0) hipEventDestroy(t->ev0);
    if (t->ev1) hipEventDestroy(t->ev1);
    if (t->stream) hipStreamDestroy(t->stream);
  }
  delete t;
}

int asdr_tuner_reset(asdr_tuner_t *t) {
  if (!t) return fail("null tuner bank");
  if (t->device != ASDR_NO_DEVICE) {
    if (asdr_tuner_synchronize(t) != 0) return -1;
    HIPCHK(hipMemset(t->d_hist[t->cur], 0, (size_t)t->n_src * ASDR_TUNER_HIST_SLOTS * sizeof(int32_t)));
    HIPCHK(hipDeviceSynchronize());
  }
  t->pos = 0;
  std::fill(t->chan.begin(), t->chan.end(), fresh_state());
  t->chan_dirty = t->order_dirty = true;
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
  const double fs = 44100.0 * t->D;
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
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!dIQ || !dI || !dQ) return fail("null device pointer");
  if (n_blocks <= 0) return 0;
  if (n_blocks > 65535 || (long long)n_blocks * 128 * t->D > (1LL << 30)) return fail("too many blocks in one call");
  const long long n_in = (long long)n_blocks * 128 * t->D;
  if (in_stride_samples < n_in) return fail("input row stride shorter than n_blocks * 128 * D samples");
  if (out_stride_blocks < n_blocks) return fail("output row stride shorter than n_blocks");
  if (in_stride_samples > (1LL << 40) || out_stride_blocks > (1LL << 30)) return fail("row stride too large");
  if ((((uintptr_t)dIQ | (uintptr_t)dI | (uintptr_t)dQ) & 15u) != 0) return fail("device pointers must be 16-byte aligned");
  const size_t in_bytes = ((size_t)(t->n_src - 1) * in_stride_samples + n_in) * 4;
  const size_t out_bytes = ((size_t)(t->n - 1) * out_stride_blocks + n_blocks) * 128 * 2;
  if (overlap((uintptr_t)dI, out_bytes, (uintptr_t)dIQ, in_bytes) || overlap((uintptr_t)dQ, out_bytes, (uintptr_t)dIQ, in_bytes))
    return fail("output span overlaps the input span");
  if (overlap((uintptr_t)dI, out_bytes, (uintptr_t)dQ, out_bytes)) return fail("I and Q output spans overlap");
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(t->device));
  if (t->ev_valid && stream != t->last_stream) HIPCHK(hipStreamWaitEvent(stream, t->ev1, 0));
  if (push(t, stream) != 0) return -1;
  TunerArgs a;
  a.in = (const int32_t *)dIQ; a.hist_rd = t->d_hist[t->cur]; a.hist_wr = t->d_hist[t->cur ^ 1];
  a.chan = t->d_chan; a.order = t->d_order; a.taps = t->d_taps; a.out_i = dI; a.out_q = dQ;
  a.pos = t->pos; a.in_stride = in_stride_samples; a.out_stride = (int64_t)out_stride_blocks * 128;
  a.n_channels = t->n; a.n_sources = t->n_src; a.n_blocks = n_blocks; a.decimation = t->D;
  a.n_phase_rows = t->n_rows; a.n_phase_pairs = t->n_pairs;
  a.shift = 15 - t->g; a.round = a.shift ? 1 << (a.shift - 1) : 0;
  HIPCHK(hipEventRecord(t->ev0, stream));
  if (asdr_launch_tuner(&a, stream) != 0) return fail("tuner kernel launch failed");
  HIPCHK(hipEventRecord(t->ev1, stream));
  t->ev_valid = true; t->last_stream = stream;
  t->pos += n_in;
  t->cur ^= 1;
  return 0;
}

int asdr_tuner_update(asdr_tuner_t *t, const int16_t *IQ, int16_t *I, int16_t *Q, int n_blocks) {
  if (!t) return fail("null tuner bank");
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!IQ || !I || !Q) return fail("null host pointer");
  if (n_blocks <= 0) return 0;
  if (n_blocks > 65535) return fail("too many blocks in one call");
  const size_t n_in = (size_t)n_blocks * 128 * t->D, in_bytes = (size_t)t->n_src * n_in * 4;
  const size_t out_bytes = (size_t)t->n * n_blocks * 128 * 2, in_pad = (in_bytes + 255) & ~(size_t)255;
  HIPCHK(hipSetDevice(t->device));
  if (in_pad + 2 * out_bytes > t->io_cap) {
    if (asdr_tuner_synchronize(t) != 0) return -1;
    if (t->d_io) HIPCHK(hipFree(t->d_io));
    t->d_io = nullptr; t->io_cap = 0;
    HIPCHK(hipMalloc(&t->d_io, in_pad + 2 * out_bytes));
    t->io_cap = in_pad + 2 * out_bytes;
  }
  char *base = (char *)t->d_io;
  int16_t *dI = (int16_t *)(base + in_pad), *dQ = (int16_t *)(base + in_pad + out_bytes);
  HIPCHK(hipMemcpyAsync(base, IQ, in_bytes, hipMemcpyHostToDevice, t->stream));
  if (asdr_tuner_update_device(t, (const int16_t *)base, (long)n_in, dI, dQ, n_blocks, n_blocks, t->stream) != 0) return -1;
  HIPCHK(hipMemcpyAsync(I, dI, out_bytes, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipMemcpyAsync(Q, dQ, out_bytes, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  return 0;
}

int asdr_tuner_synchronize(asdr_tuner_t *t) {
  if (!t) return fail("null tuner bank");
  if (t->device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipSetDevice(t->device));
  if (t->ev_valid) HIPCHK(hipEventSynchronize(t->ev1));
  HIPCHK(hipStreamSynchronize(t->stream));
  return 0;
}

float asdr_tuner_last_kernel_ms(asdr_tuner_t *t) {
  if (!t || !t->ev_valid) return -1.0f;
  float ms = -1.0f;
  if (hipEventSynchronize(t->ev1) != hipSuccess) return -1.0f;
  if (hipEventElapsedTime(&ms, t->ev0, t->ev1) != hipSuccess) return -1.0f;
  return ms;
}

}  // extern "C"
