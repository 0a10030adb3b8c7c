// asdr_spectrogram_host.cpp -- host side + C ABI (include/asdr_spectrogram.h) of the audio spectrogram.  The window lives in a host
// copy (what get_window returns) and on the device beside the float64-built twiddle table W_N; the state records live on the device
// only, in a double buffer whose halves a call reads and writes (an ASDR_NO_DEVICE spectrogram keeps them on the host instead).  The
// position T and everything a call derives from it (frame counts, the first frame's offset) is 64-bit host arithmetic.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "asdr_spectrogram_device.h"
#include "asdr_stage_host.h"

struct asdr_spectrogram : StageDev {
  int N = 0, log2n = 0, hop = 0, k0 = 0, bins = 0, window_kind = ASDR_SPECTROGRAM_RECT, kind = ASDR_SPECTROGRAM_POWER;
  std::vector<float> window;                   // [N]
  long long pos = 0;                           // T
  CarryPair carry;                             // the state records
  float *d_window = nullptr, *d_tw = nullptr;
};

namespace {
const char *kNoDevice = "control-plane-only spectrogram (ASDR_NO_DEVICE): the signal path needs a HIP device";
const char *kNull = "null spectrogram";

// F(T): the frames that lie wholly in the first T samples
long long frames_at(const asdr_spectrogram_t *s, long long t) { return t < s->N ? 0 : (t - s->N) / s->hop + 1; }

int push_window(asdr_spectrogram_t *s) {
  HIPCHK(hipMemcpy(s->d_window, s->window.data(), s->window.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// W_N^k = e^{-j 2 pi k / N}, k = 0 .. N - 1, formed in float64
int push_twiddles(asdr_spectrogram_t *s) {
  const double pi = 3.14159265358979323846;
  std::vector<float> tw((size_t)2 * s->N);
  for (int k = 0; k < s->N; k++) {
    const double ph = -2.0 * pi * k / s->N;
    tw[2 * k] = (float)std::cos(ph); tw[2 * k + 1] = (float)std::sin(ph);
  }
  HIPCHK(hipMemcpy(s->d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}
}  // namespace

extern "C" {

asdr_spectrogram_t *asdr_spectrogram_create(int n_channels, int n_fft, int hop, int first_bin, int n_bins, int window, int kind, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  int log2n = 0;
  while ((1 << log2n) < n_fft && log2n < 30) log2n++;
  if (n_fft < ASDR_SPECTROGRAM_MIN_N || n_fft > ASDR_SPECTROGRAM_MAX_N || (1 << log2n) != n_fft) {
    fail("spectrogram: N must be a power of two in 128..8192");
    return nullptr;
  }
  if (hop > n_fft || hop < 1 || (long long)hop * ASDR_SPECTROGRAM_MAX_OVERLAP < n_fft) { fail("spectrogram: the hop must be in N/16..N"); return nullptr; }
  if (first_bin < 0 || n_bins < 1 || (long long)first_bin + n_bins > n_fft / 2 + 1) {
    fail("spectrogram: the band must satisfy 0 <= k0, 1 <= B, k0 + B <= N/2 + 1");
    return nullptr;
  }
  if (window != ASDR_SPECTROGRAM_RECT && window != ASDR_SPECTROGRAM_HANN) { fail("spectrogram: the window must be rect or hann (custom: set_window)"); return nullptr; }
  if (kind != ASDR_SPECTROGRAM_POWER && kind != ASDR_SPECTROGRAM_COMPLEX) { fail("spectrogram: the output kind must be power or complex"); return nullptr; }
  asdr_spectrogram *s = new asdr_spectrogram;
  s->n = n_channels; s->N = n_fft; s->log2n = log2n; s->hop = hop; s->k0 = first_bin; s->bins = n_bins;
  s->window_kind = window; s->kind = kind;
  s->window.assign(n_fft, 1.0f);
  if (window == ASDR_SPECTROGRAM_HANN) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < n_fft; i++) s->window[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * i / n_fft));
  }
  s->carry.samples = n_fft;
  if (device == ASDR_NO_DEVICE) {
    s->carry.reset(*s);
    return s;
  }
  const size_t rec = (size_t)n_channels * n_fft * sizeof(int16_t);
  if (stage_open(*s, device, "spectrogram") != 0) { asdr_spectrogram_destroy(s); return nullptr; }
  if (hipMalloc(&s->carry.d[0], rec) != hipSuccess || hipMalloc(&s->carry.d[1], rec) != hipSuccess ||
      hipMalloc(&s->d_window, (size_t)n_fft * sizeof(float)) != hipSuccess || hipMalloc(&s->d_tw, (size_t)2 * n_fft * sizeof(float)) != hipSuccess ||
      hipMemset(s->carry.d[0], 0, rec) != hipSuccess || hipMemset(s->carry.d[1], 0, rec) != hipSuccess ||
      push_window(s) != 0 || push_twiddles(s) != 0 || hipDeviceSynchronize() != hipSuccess) {
    fail("spectrogram: device allocation failed");
    asdr_spectrogram_destroy(s);
    return nullptr;
  }
  return s;
}

void asdr_spectrogram_destroy(asdr_spectrogram_t *s) {
  if (!s) return;
  stage_close(*s, {s->carry.d[0], s->carry.d[1], s->d_window, s->d_tw});
  delete s;
}

int asdr_spectrogram_n_channels(const asdr_spectrogram_t *s) { return s ? s->n : fail(kNull); }
int asdr_spectrogram_n_fft(const asdr_spectrogram_t *s) { return s ? s->N : fail(kNull); }
int asdr_spectrogram_hop(const asdr_spectrogram_t *s) { return s ? s->hop : fail(kNull); }
int asdr_spectrogram_first_bin(const asdr_spectrogram_t *s) { return s ? s->k0 : fail(kNull); }
int asdr_spectrogram_n_bins(const asdr_spectrogram_t *s) { return s ? s->bins : fail(kNull); }
int asdr_spectrogram_window_kind(const asdr_spectrogram_t *s) { return s ? s->window_kind : fail(kNull); }
int asdr_spectrogram_output_kind(const asdr_spectrogram_t *s) { return s ? s->kind : fail(kNull); }

int asdr_spectrogram_get_window(const asdr_spectrogram_t *s, float *w) {
  if (!s) return fail(kNull);
  if (!w) return fail("null destination");
  std::memcpy(w, s->window.data(), s->window.size() * sizeof(float));
  return 0;
}

int asdr_spectrogram_set_window(asdr_spectrogram_t *s, const float *w) {
  if (!s) return fail(kNull);
  if (!w) return fail("null window");
  for (int i = 0; i < s->N; i++)
    if (!std::isfinite(w[i])) return fail("spectrogram: window value " + std::to_string(i) + " is not finite");
  if (stage_quiesce(*s) != 0) return -1;
  s->window.assign(w, w + s->N);
  s->window_kind = ASDR_SPECTROGRAM_CUSTOM;
  return s->device == ASDR_NO_DEVICE ? 0 : push_window(s);
}

long long asdr_spectrogram_position(const asdr_spectrogram_t *s) { return s ? s->pos : (long long)fail(kNull); }
long long asdr_spectrogram_frame_position(const asdr_spectrogram_t *s) { return s ? frames_at(s, s->pos) : (long long)fail(kNull); }

long asdr_spectrogram_out_frames(const asdr_spectrogram_t *s, long n_samples) {
  if (!s) return fail(kNull);
  if (n_samples < 0 || n_samples > ASDR_SPECTROGRAM_MAX_SAMPLES) return fail("n_samples must be in 0..2^24");
  return (long)(frames_at(s, s->pos + n_samples) - frames_at(s, s->pos));
}

int asdr_spectrogram_set_position(asdr_spectrogram_t *s, long long t) {
  if (!s) return fail(kNull);
  if (t < 0 || t > ASDR_SPECTROGRAM_MAX_POSITION) return fail("spectrogram: position must be in 0..2^50");
  if (stage_quiesce(*s) != 0) return -1;
  s->pos = t;
  return 0;
}

long asdr_spectrogram_update_device(asdr_spectrogram_t *s, const int16_t *dAudio, long stride_samples, long n_samples, float *dOut,
                                    long out_stride_frames, const int32_t *dIndex, const int32_t *dCount, int capacity_rows, void *stream_) {
  if (!s) return fail(kNull);
  if (s->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!dAudio || !dOut) return fail("null device pointer");
  if (n_samples < 0 || n_samples > ASDR_SPECTROGRAM_MAX_SAMPLES) return fail("n_samples must be in 0..2^24");
  if (stride_samples < n_samples) return fail("row stride shorter than n_samples");
  if (stride_samples > (1L << 40)) return fail("row stride too large");
  if (((uintptr_t)dAudio & 1u) != 0) return fail("the audio rows must be 2-byte aligned");
  if (((uintptr_t)dOut & 3u) != 0) return fail("the output rows must be 4-byte aligned");
  if (dIndex && !dCount) return fail("an index needs a count");
  if (dIndex && capacity_rows < 0) return fail("capacity_rows is negative");
  if (n_samples == 0) return 0;
  const long long t0 = s->pos, t1 = t0 + n_samples;             // <= 2^50 + 2^24 per call; checked below
  if (t1 > (1LL << 62)) return fail("spectrogram: position past 2^62");
  const long long f0 = frames_at(s, t0), f1 = frames_at(s, t1);
  const long long n_frames = f1 - f0;
  if (out_stride_frames < n_frames) return fail("output row stride shorter than the call's frame count");
  if (out_stride_frames > (1L << 40)) return fail("output row stride too large");
  const int grid_rows = dIndex ? std::min(capacity_rows, s->n) : s->n;
  const size_t per_frame = (size_t)s->bins * (s->kind == ASDR_SPECTROGRAM_COMPLEX ? 2 : 1) * sizeof(float);
  if (grid_rows > 0 && n_frames > 0) {
    const size_t audio_bytes = ((size_t)(s->n - 1) * stride_samples + n_samples) * 2;
    const size_t out_bytes = ((size_t)(grid_rows - 1) * out_stride_frames + n_frames) * per_frame;
    if (overlap((uintptr_t)dAudio, audio_bytes, (uintptr_t)dOut, out_bytes)) return fail("output span overlaps the audio span");
  }
  if ((long long)std::max(grid_rows, 1) * n_frames >= (1LL << 31) - ASDR_SPECTROGRAM_THREADS)
    return fail("spectrogram: the call is too large for one launch; split it");

  SpectrogramArgs a;
  a.audio = dAudio; a.stride = stride_samples;
  a.carry = s->carry.current(); a.carry_next = s->carry.next();
  a.out = dOut; a.out_stride = out_stride_frames;
  a.index = dIndex; a.count = dCount;
  a.window = s->d_window; a.tw = s->d_tw;
  a.n_channels = s->n; a.n_samples = (int32_t)n_samples; a.grid_rows = grid_rows; a.capacity_rows = dIndex ? capacity_rows : s->n;
  a.log2n = s->log2n; a.hop = s->hop; a.k0 = s->k0; a.n_bins = s->bins; a.complex_out = s->kind == ASDR_SPECTROGRAM_COMPLEX;
  a.n_frames = (int32_t)n_frames;
  const long long first = f0 * s->hop - t0;                     // frame f0 is not complete at T0: first > -N; H <= N: first <= 0
  a.first = (int32_t)first;
  a.scale = 1.0f / (float)s->N;
  if (first <= -(long long)s->N || first > 0 || (n_frames > 0 && first + (n_frames - 1) * s->hop + s->N > n_samples))
    return fail("internal: spectrogram launch geometry out of range");

  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*s, stream) != 0) return -1;
  if (asdr_launch_spectrogram(&a, stream) != 0) return fail("spectrogram kernel launch failed");
  if (asdr_launch_spectrogram_carry(&a, stream) != 0) return fail("spectrogram carry kernel launch failed");
  if (stage_after_launch(*s, stream) != 0) return -1;
  s->carry.flip();
  s->pos = t1;
  return (long)n_frames;
}

int asdr_spectrogram_read_state(asdr_spectrogram_t *s, int16_t *dst) {
  if (!s) return fail(kNull);
  return s->carry.read(*s, dst);
}

int asdr_spectrogram_write_state(asdr_spectrogram_t *s, const int *channels, int n, const int16_t *src) {
  if (!s) return fail(kNull);
  return s->carry.write(*s, channels, n, src);
}

int asdr_spectrogram_reset(asdr_spectrogram_t *s) {
  if (!s) return fail(kNull);
  if (s->carry.reset(*s) != 0) return -1;
  s->pos = 0;
  return 0;
}

int asdr_spectrogram_synchronize(asdr_spectrogram_t *s) {
  if (!s) return fail(kNull);
  return stage_quiesce(*s);
}

}  // extern "C"
