// asdr_stage_host.h -- what the host sides of every handle but the receiver batch share (the audio stages: gate, resampler, codec,
// spectrogram, FM demodulator, tone squelch, DCS squelch, packet decoder; the tuner bank; the front end's three batches): the device, stream and events of a
// handle and the rules that order its work (a launch on another stream than the last waits for the last; whatever frees or rewrites
// what a launch may still use waits for the handle's work first), the kept grow-on-demand buffer, the record I/O of read_state /
// write_state, and the double buffer of carry rows.  The tuner bank and the front end also time a call's launches (*_last_kernel_ms)
// between a start event, which only a handle opened `timed` has, and the event behind the launches.  An ASDR_NO_DEVICE handle never
// reaches HIP through these.
// Internal and header-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>

#include "../../include/asdr.h"

int asdr_internal_fail(const std::string &m);   // asdr_host.cpp: sets the thread's asdr_last_error() text, returns -1

static inline int fail(const std::string &m) { return asdr_internal_fail(m); }
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

static inline bool overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }

static inline int stage_check_create(int n_channels) {
  return n_channels <= 0 || n_channels > (1 << 20) ? fail("n_channels must be in 1..1048576") : 0;
}

static inline int stage_check_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail("no HIP device: this library has no CPU fallback");
  if (device < 0 || device >= count) return fail("bad device index");
  return 0;
}

struct StageDev {
  int n = 0, device = ASDR_NO_DEVICE;
  hipStream_t stream = nullptr, last_stream = nullptr;   // the handle's own stream; the stream of the last launch
  hipEvent_t ev = nullptr;                               // recorded behind every launch
  hipEvent_t ev_start = nullptr;                         // timed handles: recorded in front of a call's launches
  bool ev_valid = false;
};

// the device of a handle that is not ASDR_NO_DEVICE, its stream and its event (a timed handle's two); `what` names the stage in the
// error text.  A handle whose device index was refused stays ASDR_NO_DEVICE, so that stage_close leaves HIP alone
static inline int stage_open(StageDev &d, int device, const char *what, bool timed = false) {
  if (stage_check_device(device) != 0) return -1;
  d.device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&d.stream) != hipSuccess || hipEventCreate(&d.ev) != hipSuccess ||
      (timed && hipEventCreate(&d.ev_start) != hipSuccess))
    return fail(std::string(what) + ": device allocation failed");
  return 0;
}

// waits for the handle's work (nothing for ASDR_NO_DEVICE)
static inline int stage_quiesce(StageDev &d) {
  if (d.device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipSetDevice(d.device));
  if (d.ev_valid) HIPCHK(hipEventSynchronize(d.ev));
  HIPCHK(hipStreamSynchronize(d.stream));
  return 0;
}

// around the launches of a call on `stream`: they run behind the last call's, whatever stream that was on
static inline int stage_before_launch(StageDev &d, hipStream_t stream) {
  HIPCHK(hipSetDevice(d.device));
  if (d.ev_valid && stream != d.last_stream) HIPCHK(hipStreamWaitEvent(stream, d.ev, 0));
  return 0;
}
static inline int stage_after_launch(StageDev &d, hipStream_t stream) {
  HIPCHK(hipEventRecord(d.ev, stream));
  d.ev_valid = true; d.last_stream = stream;
  return 0;
}

// a timed handle: between the pushes of a call and its launches; stage_last_ms is the time between this and stage_after_launch's
// event, -1 without a recorded pair
static inline int stage_mark_start(StageDev &d, hipStream_t stream) {
  if (d.ev_start) HIPCHK(hipEventRecord(d.ev_start, stream));
  return 0;
}
static inline float stage_last_ms(StageDev &d) {
  if (!d.ev_start || !d.ev_valid) return -1.0f;
  float ms = -1.0f;
  if (hipEventSynchronize(d.ev) != hipSuccess) return -1.0f;
  if (hipEventElapsedTime(&ms, d.ev_start, d.ev) != hipSuccess) return -1.0f;
  return ms;
}

// a device buffer of at least `bytes`, kept; growing waits for the work that may still use the old one
static inline int stage_reserve(StageDev &d, void **p, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  if (stage_quiesce(d) != 0) return -1;
  if (*p) HIPCHK(hipFree(*p));
  *p = nullptr; *cap = 0;
  HIPCHK(hipMalloc(p, bytes));
  *cap = bytes;
  return 0;
}

// waits for the handle's work, then frees its buffers, its events and its stream
static inline void stage_close(StageDev &d, std::initializer_list<void *> buffers) {
  if (d.device == ASDR_NO_DEVICE) return;
  hipSetDevice(d.device);
  if (d.ev_valid) hipEventSynchronize(d.ev);
  if (d.stream) hipStreamSynchronize(d.stream);
  for (void *p : buffers)
    if (p) hipFree(p);
  if (d.ev) hipEventDestroy(d.ev);
  if (d.ev_start) hipEventDestroy(d.ev_start);
  if (d.stream) hipStreamDestroy(d.stream);
}

// Record I/O: d.n records of `rec` bytes, in the host mirror `host` of an ASDR_NO_DEVICE handle and at `dev` of any other.
static inline int stage_read_state(StageDev &d, void *dst, size_t rec, const void *host, const void *dev) {
  if (!dst) return fail("null destination");
  if (d.device == ASDR_NO_DEVICE) { std::memcpy(dst, host, d.n * rec); return 0; }
  if (stage_quiesce(d) != 0) return -1;
  HIPCHK(hipMemcpy(dst, dev, d.n * rec, hipMemcpyDeviceToHost));
  return 0;
}

// record k of src goes to channel channels[k] (k without a list); `check(k, record)`, if given, refuses a record by failing.  Every
// record is checked before the first is written
static inline int stage_write_state(StageDev &d, const int *channels, int n, const void *src, size_t rec, void *host, void *dev,
                                    const std::function<int(int, const void *)> &check = nullptr) {
  if (n < 0) return fail("negative record count");
  if (n == 0) return 0;
  if (!src) return fail("null source");
  if (!channels && n > d.n) return fail("more records than channels");
  for (int k = 0; k < n; k++) {
    const int c = channels ? channels[k] : k;
    if (c < 0 || c >= d.n) return fail("record " + std::to_string(k) + ": bad channel");
    if (check && check(k, (const char *)src + k * rec) != 0) return -1;
  }
  if (stage_quiesce(d) != 0) return -1;
  if (!channels && d.device != ASDR_NO_DEVICE) {
    HIPCHK(hipMemcpy(dev, src, n * rec, hipMemcpyHostToDevice));
    return 0;
  }
  for (int k = 0; k < n; k++) {
    const size_t c = channels ? channels[k] : k;
    if (d.device == ASDR_NO_DEVICE) std::memcpy((char *)host + c * rec, (const char *)src + k * rec, rec);
    else HIPCHK(hipMemcpy((char *)dev + c * rec, (const char *)src + k * rec, rec, hipMemcpyHostToDevice));
  }
  return 0;
}

// The double buffer of carry rows (resampler, spectrogram): a call reads current() and writes next(), then flips.
struct CarryPair {
  int16_t *d[2] = {nullptr, nullptr};
  int cur = 0;
  int16_t *current() const { return d[cur]; }
  int16_t *next() const { return d[cur ^ 1]; }
  void flip() { cur ^= 1; }
  int reset(StageDev &dev, size_t bytes) {   // zero records, behind the handle's work
    if (stage_quiesce(dev) != 0) return -1;
    HIPCHK(hipMemsetAsync(current(), 0, bytes, dev.stream));
    HIPCHK(hipStreamSynchronize(dev.stream));
    return 0;
  }
};
