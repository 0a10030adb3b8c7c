// asdr_stage_host.h -- what the host sides of every handle but the receiver batch share (the audio stages: gate, resampler, codec,
// spectrogram, FM demodulator, tone squelch, DCS squelch, packet decoder, CW decoder; the tuner bank; the front end's three batches): the device, stream and events of a
// handle and the rules that order its work (a launch on another stream than the last waits for the last; whatever frees or rewrites
// what a launch may still use waits for the handle's work first), the kept grow-on-demand buffer, and the double buffer of carry rows.
// For the audio stages it also states, once each: the handle and channel check of a setter or getter (stage_check_channel), the
// refusals of a block-row call, which are the bounds checks of the kernels behind it (stage_check_block_rows), a stage's state
// records (StageRecords: read_state / write_state, the creation record, a rewrite of every record, the zero reset; the
// ASDR_NO_DEVICE / device split is decided there) and a mirrored table of settings (StageMirror: the host copy, its dirty flag and
// the push on a call's stream).  The tuner bank and the front end also time a call's launches (*_last_kernel_ms) between a start
// event, which only a handle opened `timed` has, and the event behind the launches.  An ASDR_NO_DEVICE handle never reaches HIP
// through these.
// Internal and header-only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <vector>

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

// a setter's or getter's handle and channel; `null_text` is the stage's "null ..." text, ASDR_ALL passes where `all_allowed`
static inline int stage_check_channel(const StageDev *d, int ch, bool all_allowed, const char *null_text) {
  if (!d) return fail(null_text);
  if (all_allowed && ch == ASDR_ALL) return 0;
  return ch < 0 || ch >= d->n ? fail("bad channel") : 0;
}

// Block rows of a call: `rows` int16 rows of stride_blocks blocks of 128 samples behind each pointer of p; a call touches the
// first n_blocks blocks of every row.
struct BlockRows {
  std::initializer_list<const void *> p;
  int rows;
  long stride_blocks;
  size_t bytes(int n_blocks) const { return ((size_t)(rows - 1) * stride_blocks + n_blocks) * 256; }
};

// The refusals of a block-row call, in this order: a null pointer, n_blocks outside 0..65535, a stride shorter than n_blocks, a
// stride above 2^30, a pointer off 16 bytes, and -- unless n_blocks is 0, when the call has nothing to do and the caller returns 0
// -- an output span that overlaps an input span (`overlap_text`).  The kernels behind it write out.bytes(n_blocks) bytes through
// the caller's pointers: these are their bounds checks.  `out` is {} for a call that writes no rows
static inline int stage_check_block_rows(const BlockRows &in, const BlockRows &out, int n_blocks, const char *overlap_text) {
  const bool has_out = out.p.size() != 0;
  bool null = false;
  uintptr_t bits = 0;
  for (const BlockRows *r : {&in, &out})
    for (const void *p : r->p) { null |= !p; bits |= (uintptr_t)p; }
  if (null) return fail("null device pointer");
  if (n_blocks < 0 || n_blocks > 65535) return fail("n_blocks must be in 0..65535");
  if (in.stride_blocks < n_blocks || (has_out && out.stride_blocks < n_blocks)) return fail("row stride shorter than n_blocks");
  if (in.stride_blocks > (1L << 30) || (has_out && out.stride_blocks > (1L << 30))) return fail("row stride too large");
  if ((bits & 15u) != 0) return fail("device pointers must be 16-byte aligned");
  if (n_blocks == 0) return 0;
  for (const void *a : in.p)
    for (const void *b : out.p)
      if (overlap((uintptr_t)a, in.bytes(n_blocks), (uintptr_t)b, out.bytes(n_blocks))) return fail(overlap_text);
  return 0;
}

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

// zeroes a device buffer behind the handle's work, on its stream; done on return (the zero reset of records and carry rows)
static inline int stage_zero(StageDev &d, void *p, size_t bytes) {
  if (stage_quiesce(d) != 0) return -1;
  HIPCHK(hipMemsetAsync(p, 0, bytes, d.stream));
  HIPCHK(hipStreamSynchronize(d.stream));
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

// A stage's state records: one Rec a channel, in `host` of an ASDR_NO_DEVICE handle and at `dev` of any other.
template <class Rec>
struct StageRecords {
  std::vector<Rec> host;
  Rec *dev = nullptr;
  static constexpr size_t kChunk = 4096;   // records per transfer of fill and rewrite

  int read(StageDev &d, Rec *dst) const { return stage_read_state(d, dst, sizeof(Rec), host.data(), dev); }
  // `check(k, record)`, if given, refuses record k beyond its channel
  int write(StageDev &d, const int *channels, int n, const Rec *src, const std::function<int(int, const Rec &)> &check = nullptr) {
    if (!check) return stage_write_state(d, channels, n, src, sizeof(Rec), host.data(), dev);
    return stage_write_state(d, channels, n, src, sizeof(Rec), host.data(), dev, [&](int k, const void *rec) { return check(k, *(const Rec *)rec); });
  }
  // `rec` into every channel, behind the handle's work: creation and the reset of a stage whose creation record is not all zero
  int fill(StageDev &d, const Rec &rec) {
    if (d.device == ASDR_NO_DEVICE) { host.assign(d.n, rec); return 0; }
    if (stage_quiesce(d) != 0) return -1;
    const std::vector<Rec> buf(std::min((size_t)d.n, kChunk), rec);
    for (size_t c = 0; c < (size_t)d.n; c += kChunk)
      HIPCHK(hipMemcpy(dev + c, buf.data(), std::min(kChunk, (size_t)d.n - c) * sizeof(Rec), hipMemcpyHostToDevice));
    return 0;
  }
  // the zero record into every channel: the reset of a stage whose creation record is all zero
  int zero(StageDev &d) {
    if (d.device == ASDR_NO_DEVICE) { host.assign(d.n, Rec{}); return 0; }
    return stage_zero(d, dev, (size_t)d.n * sizeof(Rec));
  }
  // every record through `change`, in chunks, behind the handle's work
  template <class F>
  int rewrite(StageDev &d, F change) {
    if (d.device == ASDR_NO_DEVICE) {
      for (Rec &r : host) change(r);
      return 0;
    }
    if (stage_quiesce(d) != 0) return -1;
    std::vector<Rec> buf(std::min((size_t)d.n, kChunk));
    for (size_t c = 0; c < (size_t)d.n; c += kChunk) {
      const size_t m = std::min(kChunk, (size_t)d.n - c);
      HIPCHK(hipMemcpy(buf.data(), dev + c, m * sizeof(Rec), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < m; k++) change(buf[k]);
      HIPCHK(hipMemcpy(dev + c, buf.data(), m * sizeof(Rec), hipMemcpyHostToDevice));
    }
    return 0;
  }
};

// A mirrored table of settings: the host copy that setters change and getters read, and the device copy that a call pushes on its
// stream, in front of its launches, when a setter touched the host's.
template <class Set>
struct StageMirror {
  std::vector<Set> host;
  Set *dev = nullptr;
  bool dirty = true;
  const Set &operator[](size_t k) const { return host[k]; }
  // one setter's change on entry ch or, for ASDR_ALL, on every entry
  template <class F>
  void apply(int ch, F change) {
    if (ch == ASDR_ALL) for (Set &s : host) change(s);
    else change(host[ch]);
    dirty = true;
  }
  int push(hipStream_t stream) {
    if (!dirty) return 0;
    HIPCHK(hipMemcpyAsync(dev, host.data(), host.size() * sizeof(Set), hipMemcpyHostToDevice, stream));
    dirty = false;
    return 0;
  }
};

// The records of the resampler and the spectrogram: one row of `samples` int16 a channel, on the device in a double buffer of which
// a call reads current() and writes next(), then flips.
struct CarryPair {
  size_t samples = 0;          // int16 per record
  std::vector<int16_t> host;   // ASDR_NO_DEVICE only
  int16_t *d[2] = {nullptr, nullptr};
  int cur = 0;
  int16_t *current() const { return d[cur]; }
  int16_t *next() const { return d[cur ^ 1]; }
  void flip() { cur ^= 1; }
  int read(StageDev &dev, int16_t *dst) const { return stage_read_state(dev, dst, samples * sizeof(int16_t), host.data(), current()); }
  int write(StageDev &dev, const int *channels, int n, const int16_t *src) {
    return stage_write_state(dev, channels, n, src, samples * sizeof(int16_t), host.data(), current());
  }
  int reset(StageDev &dev) {   // zero records, behind the handle's work
    if (dev.device == ASDR_NO_DEVICE) { host.assign((size_t)dev.n * samples, 0); return 0; }
    return stage_zero(dev, current(), (size_t)dev.n * samples * sizeof(int16_t));
  }
};
