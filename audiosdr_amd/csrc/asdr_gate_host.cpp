// asdr_gate_host.cpp -- host side + C ABI (include/asdr_gate.h) of the audio gate.  The settings live in a host mirror that is
// pushed before a launch when a setter touched it; the state rows, the delivered flags, count and index live on the device only
// (an ASDR_NO_DEVICE gate keeps the state rows on the host instead).  The scratch of block energies and deliver's packet buffer
// grow on demand and are kept.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "asdr_gate_device.h"

int asdr_internal_fail(const std::string &m);   // asdr_host.cpp: sets the thread's asdr_last_error() text, returns -1

static_assert(sizeof(asdr_gate_state_t) == 32, "asdr_gate_state_t is a 32-byte record");
static_assert(sizeof(GateSetting) == 24, "GateSetting is 24 bytes");

struct asdr_gate {
  int n = 0, device = ASDR_NO_DEVICE;
  std::vector<GateSetting> set;
  bool set_dirty = true;
  std::vector<asdr_gate_state_t> host_state;   // ASDR_NO_DEVICE only
  long long blocks = 0;
  hipStream_t stream = nullptr, last_stream = nullptr;
  hipEvent_t ev = nullptr;
  bool ev_valid = false;
  GateSetting *d_set = nullptr;
  asdr_gate_state_t *d_state = nullptr;
  uint8_t *d_flag = nullptr;
  int32_t *d_tile = nullptr, *d_count = nullptr, *d_index = nullptr;
  void *d_scr = nullptr, *d_rows = nullptr;
  size_t scr_cap = 0, rows_cap = 0;
};

namespace {
int fail(const std::string &m) { return asdr_internal_fail(m); }
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

const char *kNoDevice = "control-plane-only gate (ASDR_NO_DEVICE): the signal path needs a HIP device";

int n_tiles(const asdr_gate_t *g) { return (g->n + ASDR_GATE_TILE - 1) / ASDR_GATE_TILE; }

// waits for the gate's work (nothing for ASDR_NO_DEVICE)
int quiesce(asdr_gate_t *g) {
  if (g->device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipSetDevice(g->device));
  if (g->ev_valid) HIPCHK(hipEventSynchronize(g->ev));
  HIPCHK(hipStreamSynchronize(g->stream));
  return 0;
}

// a device buffer of at least `bytes`, kept; growing waits for the work that may still use the old one
int reserve(asdr_gate_t *g, void **p, size_t *cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  if (quiesce(g) != 0) return -1;
  if (*p) HIPCHK(hipFree(*p));
  *p = nullptr; *cap = 0;
  HIPCHK(hipMalloc(p, bytes));
  *cap = bytes;
  return 0;
}

GateArgs make_args(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dRows, int capacity_rows) {
  GateArgs a;
  a.audio = dAudio; a.stride_blocks = stride_blocks; a.n_channels = g->n; a.n_blocks = n_blocks;
  a.set = g->d_set; a.state = g->d_state;
  a.scr = (uint64_t *)g->d_scr;
  a.flag = g->d_flag; a.tile_count = g->d_tile; a.count = g->d_count; a.index = g->d_index;
  a.rows = dRows; a.capacity_rows = capacity_rows;
  return a;
}

int check_audio(const asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks) {
  if (g->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (!dAudio) return fail("null device pointer");
  if (n_blocks < 0 || n_blocks > 65535) return fail("n_blocks must be in 0..65535");
  if (stride_blocks < n_blocks) return fail("row stride shorter than n_blocks");
  if (stride_blocks > (1L << 30)) return fail("row stride too large");
  if (((uintptr_t)dAudio & 15u) != 0) return fail("device pointers must be 16-byte aligned");
  return 0;
}

bool overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }
}  // namespace

extern "C" {

uint64_t asdr_gate_energy_from_dbfs(double db) {
  const double v = std::floor(128.0 * 32767.0 * 32767.0 * std::pow(10.0, db / 10.0) + 0.5);
  if (!(v > 0.0)) return 0;   // NaN too
  return v >= (double)ASDR_GATE_MAX_ENERGY ? ASDR_GATE_MAX_ENERGY : (uint64_t)v;
}

asdr_gate_t *asdr_gate_create(int n_channels, int device) {
  if (n_channels <= 0 || n_channels > (1 << 20)) { fail("n_channels must be in 1..1048576"); return nullptr; }
  asdr_gate *g = new asdr_gate;
  g->n = n_channels; g->device = device;
  g->set.assign(n_channels, GateSetting{0, 0, 0, 0});
  if (device == ASDR_NO_DEVICE) {
    g->host_state.assign(n_channels, asdr_gate_state_t{});
    return g;
  }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { fail("no HIP device: this library has no CPU fallback"); delete g; return nullptr; }
  if (device < 0 || device >= count) { fail("bad device index"); delete g; return nullptr; }
  const size_t n = n_channels, tiles = n_tiles(g);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&g->stream) != hipSuccess || hipEventCreate(&g->ev) != hipSuccess ||
      hipMalloc(&g->d_set, n * sizeof(GateSetting)) != hipSuccess || hipMalloc(&g->d_state, n * sizeof(asdr_gate_state_t)) != hipSuccess ||
      hipMalloc(&g->d_flag, n) != hipSuccess || hipMalloc(&g->d_tile, tiles * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&g->d_count, sizeof(int32_t)) != hipSuccess || hipMalloc(&g->d_index, n * sizeof(int32_t)) != hipSuccess ||
      hipMemset(g->d_state, 0, n * sizeof(asdr_gate_state_t)) != hipSuccess || hipMemset(g->d_flag, 0, n) != hipSuccess ||
      hipMemset(g->d_tile, 0, tiles * sizeof(int32_t)) != hipSuccess || hipMemset(g->d_count, 0, sizeof(int32_t)) != hipSuccess ||
      hipMemset(g->d_index, 0, n * sizeof(int32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fail("gate: device allocation failed");
    asdr_gate_destroy(g);
    return nullptr;
  }
  return g;
}

void asdr_gate_destroy(asdr_gate_t *g) {
  if (!g) return;
  if (g->device != ASDR_NO_DEVICE) {
    hipSetDevice(g->device);
    if (g->ev_valid) hipEventSynchronize(g->ev);
    if (g->stream) hipStreamSynchronize(g->stream);
    for (void *p : {(void *)g->d_set, (void *)g->d_state, (void *)g->d_flag, (void *)g->d_tile, (void *)g->d_count, (void *)g->d_index,
                    g->d_scr, g->d_rows})
      if (p) hipFree(p);
    if (g->ev) hipEventDestroy(g->ev);
    if (g->stream) hipStreamDestroy(g->stream);
  }
  delete g;
}

int asdr_gate_n_channels(const asdr_gate_t *g) { return g ? g->n : fail("null gate"); }

int asdr_gate_set_squelch(asdr_gate_t *g, int ch, uint64_t open_energy, uint64_t close_energy, int hang_blocks) {
  if (!g) return fail("null gate");
  if (ch != ASDR_ALL && (ch < 0 || ch >= g->n)) return fail("bad channel");
  if (close_energy > open_energy) return fail("close_energy must not exceed open_energy");
  if (hang_blocks < 0 || hang_blocks > ASDR_GATE_MAX_HANG) return fail("hang_blocks must be in 0..65535");
  const GateSetting s{open_energy, close_energy, (uint32_t)hang_blocks, 0};
  if (ch == ASDR_ALL) std::fill(g->set.begin(), g->set.end(), s);
  else g->set[ch] = s;
  g->set_dirty = true;
  return 0;
}

int asdr_gate_get_squelch(const asdr_gate_t *g, int ch, uint64_t *open_energy, uint64_t *close_energy, int *hang_blocks) {
  if (!g) return fail("null gate");
  if (ch < 0 || ch >= g->n) return fail("bad channel");
  if (open_energy) *open_energy = g->set[ch].open_energy;
  if (close_energy) *close_energy = g->set[ch].close_energy;
  if (hang_blocks) *hang_blocks = (int)g->set[ch].hang_blocks;
  return 0;
}

int asdr_gate_update_device(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dRows, int capacity_rows,
                            void *stream_) {
  if (!g) return fail("null gate");
  if (check_audio(g, dAudio, stride_blocks, n_blocks) != 0) return -1;
  if (capacity_rows < 0) return fail("capacity_rows is negative");
  if (!dRows) capacity_rows = 0;
  if (capacity_rows == 0) dRows = nullptr;
  if (n_blocks == 0) return 0;
  const int grid_rows = std::min(capacity_rows, g->n);
  if (dRows) {
    if (((uintptr_t)dRows & 15u) != 0) return fail("device pointers must be 16-byte aligned");
    const size_t audio_bytes = ((size_t)(g->n - 1) * stride_blocks + n_blocks) * 256, rows_bytes = (size_t)grid_rows * n_blocks * 256;
    if (overlap((uintptr_t)dAudio, audio_bytes, (uintptr_t)dRows, rows_bytes)) return fail("packet span overlaps the audio span");
  }
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(g->device));
  if (n_blocks > 1 && reserve(g, &g->d_scr, &g->scr_cap, (size_t)g->n * n_blocks * sizeof(uint64_t)) != 0) return -1;
  if (g->ev_valid && stream != g->last_stream) HIPCHK(hipStreamWaitEvent(stream, g->ev, 0));
  if (g->set_dirty) {
    HIPCHK(hipMemcpyAsync(g->d_set, g->set.data(), g->set.size() * sizeof(GateSetting), hipMemcpyHostToDevice, stream));
    g->set_dirty = false;
  }
  const GateArgs a = make_args(g, dAudio, stride_blocks, n_blocks, dRows, grid_rows);
  if (asdr_launch_gate_pass(&a, stream) != 0) return fail("gate kernel launch failed");
  if (dRows && asdr_launch_gate_packet(&a, grid_rows, stream) != 0) return fail("gate packet kernel launch failed");
  HIPCHK(hipEventRecord(g->ev, stream));
  g->ev_valid = true; g->last_stream = stream;
  g->blocks += n_blocks;
  return 0;
}

const int32_t *asdr_gate_count_device(asdr_gate_t *g) {
  if (!g) { fail("null gate"); return nullptr; }
  if (g->device == ASDR_NO_DEVICE) { fail(kNoDevice); return nullptr; }
  return g->d_count;
}

const int32_t *asdr_gate_index_device(asdr_gate_t *g) {
  if (!g) { fail("null gate"); return nullptr; }
  if (g->device == ASDR_NO_DEVICE) { fail(kNoDevice); return nullptr; }
  return g->d_index;
}

int asdr_gate_deliver(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int32_t *host_index, int16_t *host_rows,
                      int capacity_rows, int *n_open) {
  if (!g) return fail("null gate");
  if (check_audio(g, dAudio, stride_blocks, n_blocks) != 0) return -1;
  if (!host_index) return fail("null host index");
  if (capacity_rows < 0) return fail("capacity_rows is negative");
  if (capacity_rows > 0 && !host_rows) return fail("null host rows with capacity_rows > 0");
  if (n_open) *n_open = 0;
  if (n_blocks == 0) return 0;
  if (asdr_gate_update_device(g, dAudio, stride_blocks, n_blocks, nullptr, 0, g->stream) != 0) return -1;
  int32_t count = 0;
  HIPCHK(hipMemcpyAsync(&count, g->d_count, sizeof(count), hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  if (count < 0 || count > g->n) return fail("internal: gate count out of range");
  if (n_open) *n_open = count;
  if (count == 0) return 0;
  const int rows = std::min(count, capacity_rows);
  const size_t rows_bytes = (size_t)rows * n_blocks * 256;
  HIPCHK(hipMemcpyAsync(host_index, g->d_index, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
  if (rows > 0) {
    if (reserve(g, &g->d_rows, &g->rows_cap, rows_bytes) != 0) return -1;
    if (overlap((uintptr_t)dAudio, ((size_t)(g->n - 1) * stride_blocks + n_blocks) * 256, (uintptr_t)g->d_rows, rows_bytes))
      return fail("internal: packet buffer overlaps the audio span");
    const GateArgs a = make_args(g, dAudio, stride_blocks, n_blocks, (int16_t *)g->d_rows, rows);
    if (asdr_launch_gate_packet(&a, rows, g->stream) != 0) return fail("gate packet kernel launch failed");
    HIPCHK(hipMemcpyAsync(host_rows, g->d_rows, rows_bytes, hipMemcpyDeviceToHost, g->stream));
  }
  HIPCHK(hipStreamSynchronize(g->stream));
  return rows;
}

int asdr_gate_read_state(asdr_gate_t *g, asdr_gate_state_t *dst) {
  if (!g) return fail("null gate");
  if (!dst) return fail("null destination");
  if (g->device == ASDR_NO_DEVICE) {
    std::memcpy(dst, g->host_state.data(), g->n * sizeof(asdr_gate_state_t));
    return 0;
  }
  if (quiesce(g) != 0) return -1;
  HIPCHK(hipMemcpy(dst, g->d_state, g->n * sizeof(asdr_gate_state_t), hipMemcpyDeviceToHost));
  return 0;
}

int asdr_gate_write_state(asdr_gate_t *g, const int *channels, int n, const asdr_gate_state_t *src) {
  if (!g) return fail("null gate");
  if (n < 0) return fail("negative record count");
  if (n == 0) return 0;
  if (!src) return fail("null source");
  if (!channels && n > g->n) return fail("more records than channels");
  for (int k = 0; k < n; k++) {
    const int c = channels ? channels[k] : k;
    if (c < 0 || c >= g->n) return fail("record " + std::to_string(k) + ": bad channel");
    if (src[k].open > 1) return fail("record " + std::to_string(k) + ": open must be 0 or 1");
    if (src[k].reserved != 0) return fail("record " + std::to_string(k) + ": reserved byte must be 0");
  }
  if (g->device != ASDR_NO_DEVICE && quiesce(g) != 0) return -1;
  for (int k = 0; k < n; k++) {
    const int c = channels ? channels[k] : k;
    if (g->device == ASDR_NO_DEVICE) g->host_state[c] = src[k];
    else HIPCHK(hipMemcpy(g->d_state + c, src + k, sizeof(asdr_gate_state_t), hipMemcpyHostToDevice));
  }
  return 0;
}

int asdr_gate_clear(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  std::vector<asdr_gate_state_t> st(g->n);
  if (asdr_gate_read_state(g, st.data()) != 0) return -1;
  for (asdr_gate_state_t &s : st) {
    asdr_gate_state_t z{};
    z.hang_left = s.hang_left; z.open = s.open;
    s = z;
  }
  if (g->device == ASDR_NO_DEVICE) g->host_state = st;
  else HIPCHK(hipMemcpy(g->d_state, st.data(), g->n * sizeof(asdr_gate_state_t), hipMemcpyHostToDevice));
  g->blocks = 0;
  return 0;
}

int asdr_gate_reset(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  if (g->device == ASDR_NO_DEVICE) {
    g->host_state.assign(g->n, asdr_gate_state_t{});
  } else {
    if (quiesce(g) != 0) return -1;
    HIPCHK(hipMemsetAsync(g->d_state, 0, g->n * sizeof(asdr_gate_state_t), g->stream));
    HIPCHK(hipMemsetAsync(g->d_count, 0, sizeof(int32_t), g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
  }
  g->blocks = 0;
  return 0;
}

long long asdr_gate_blocks(const asdr_gate_t *g) { return g ? g->blocks : -1; }

int asdr_gate_synchronize(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  return quiesce(g);
}

}  // extern "C"
