// asdr_gate_host.cpp -- host side + C ABI (include/asdr_gate.h) of the audio gate.  The settings live in a host mirror that is
// pushed before a launch when a setter touched it; the state rows, the delivered flags, count and index live on the device only
// (an ASDR_NO_DEVICE gate keeps the state rows on the host instead).  The scratch of block energies and deliver's packet buffer
// grow on demand and are kept.
#include <algorithm>
#include <cmath>
#include <vector>

#include "asdr_gate_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_gate_state_t) == 32, "asdr_gate_state_t is a 32-byte record");
static_assert(sizeof(GateSetting) == 24, "GateSetting is 24 bytes");

struct asdr_gate : StageDev {
  StageMirror<GateSetting> set;
  StageRecords<asdr_gate_state_t> state;
  long long blocks = 0;
  uint8_t *d_flag = nullptr;
  int32_t *d_tile = nullptr, *d_count = nullptr, *d_index = nullptr;
  void *d_scr = nullptr, *d_rows = nullptr;
  size_t scr_cap = 0, rows_cap = 0;
};

namespace {
const char *kNoDevice = "control-plane-only gate (ASDR_NO_DEVICE): the signal path needs a HIP device";

int n_tiles(const asdr_gate_t *g) { return (g->n + ASDR_GATE_TILE - 1) / ASDR_GATE_TILE; }

GateArgs make_args(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dRows, int capacity_rows) {
  GateArgs a;
  a.audio = dAudio; a.stride_blocks = stride_blocks; a.n_channels = g->n; a.n_blocks = n_blocks;
  a.set = g->set.dev; a.state = g->state.dev;
  a.scr = (uint64_t *)g->d_scr;
  a.flag = g->d_flag; a.tile_count = g->d_tile; a.count = g->d_count; a.index = g->d_index;
  a.rows = dRows; a.capacity_rows = capacity_rows;
  return a;
}

int check_audio(const asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks) {
  if (g->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  return stage_check_block_rows({{dAudio}, g->n, stride_blocks}, {}, n_blocks, nullptr);
}

// write_state's check of record k beyond its channel
int check_record(int k, const asdr_gate_state_t &s) {
  if (s.open > 1) return fail("record " + std::to_string(k) + ": open must be 0 or 1");
  if (s.reserved != 0) return fail("record " + std::to_string(k) + ": reserved byte must be 0");
  return 0;
}
}  // namespace

extern "C" {

uint64_t asdr_gate_energy_from_dbfs(double db) {
  const double v = std::floor(128.0 * 32767.0 * 32767.0 * std::pow(10.0, db / 10.0) + 0.5);
  if (!(v > 0.0)) return 0;   // NaN too
  return v >= (double)ASDR_GATE_MAX_ENERGY ? ASDR_GATE_MAX_ENERGY : (uint64_t)v;
}

asdr_gate_t *asdr_gate_create(int n_channels, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  asdr_gate *g = new asdr_gate;
  g->n = n_channels;
  g->set.host.assign(n_channels, GateSetting{0, 0, 0, 0});
  if (device == ASDR_NO_DEVICE) {
    g->state.zero(*g);
    return g;
  }
  const size_t n = n_channels, tiles = n_tiles(g);
  if (stage_open(*g, device, "gate") != 0) { asdr_gate_destroy(g); return nullptr; }
  if (hipMalloc(&g->set.dev, n * sizeof(GateSetting)) != hipSuccess || hipMalloc(&g->state.dev, n * sizeof(asdr_gate_state_t)) != hipSuccess ||
      hipMalloc(&g->d_flag, n) != hipSuccess || hipMalloc(&g->d_tile, tiles * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&g->d_count, sizeof(int32_t)) != hipSuccess || hipMalloc(&g->d_index, n * sizeof(int32_t)) != hipSuccess ||
      hipMemset(g->state.dev, 0, n * sizeof(asdr_gate_state_t)) != hipSuccess || hipMemset(g->d_flag, 0, n) != hipSuccess ||
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
  stage_close(*g, {g->set.dev, g->state.dev, g->d_flag, g->d_tile, g->d_count, g->d_index, g->d_scr, g->d_rows});
  delete g;
}

int asdr_gate_n_channels(const asdr_gate_t *g) { return g ? g->n : fail("null gate"); }

int asdr_gate_set_squelch(asdr_gate_t *g, int ch, uint64_t open_energy, uint64_t close_energy, int hang_blocks) {
  if (stage_check_channel(g, ch, true, "null gate") != 0) return -1;
  if (close_energy > open_energy) return fail("close_energy must not exceed open_energy");
  if (hang_blocks < 0 || hang_blocks > ASDR_GATE_MAX_HANG) return fail("hang_blocks must be in 0..65535");
  const GateSetting s{open_energy, close_energy, (uint32_t)hang_blocks, 0};
  g->set.apply(ch, [=](GateSetting &v) { v = s; });
  return 0;
}

int asdr_gate_get_squelch(const asdr_gate_t *g, int ch, uint64_t *open_energy, uint64_t *close_energy, int *hang_blocks) {
  if (stage_check_channel(g, ch, false, "null gate") != 0) return -1;
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
  // the packet: grid_rows dense rows; their pointer's alignment and the overlap are what this call can still refuse
  if (dRows && stage_check_block_rows({{dAudio}, g->n, stride_blocks}, {{dRows}, grid_rows, n_blocks}, n_blocks, "packet span overlaps the audio span") != 0)
    return -1;
  hipStream_t stream = (hipStream_t)stream_;
  if (n_blocks > 1 && stage_reserve(*g, &g->d_scr, &g->scr_cap, (size_t)g->n * n_blocks * sizeof(uint64_t)) != 0) return -1;
  if (stage_before_launch(*g, stream) != 0 || g->set.push(stream) != 0) return -1;
  const GateArgs a = make_args(g, dAudio, stride_blocks, n_blocks, dRows, grid_rows);
  if (asdr_launch_gate_pass(&a, stream) != 0) return fail("gate kernel launch failed");
  if (dRows && asdr_launch_gate_packet(&a, grid_rows, stream) != 0) return fail("gate packet kernel launch failed");
  if (stage_after_launch(*g, stream) != 0) return -1;
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
    if (stage_reserve(*g, &g->d_rows, &g->rows_cap, rows_bytes) != 0) return -1;
    if (overlap((uintptr_t)dAudio, BlockRows{{dAudio}, g->n, stride_blocks}.bytes(n_blocks), (uintptr_t)g->d_rows, rows_bytes))
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
  return g->state.read(*g, dst);
}

int asdr_gate_write_state(asdr_gate_t *g, const int *channels, int n, const asdr_gate_state_t *src) {
  if (!g) return fail("null gate");
  return g->state.write(*g, channels, n, src, check_record);
}

int asdr_gate_clear(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  auto keep_squelch = [](asdr_gate_state_t &s) {
    asdr_gate_state_t z{};
    z.hang_left = s.hang_left; z.open = s.open;
    s = z;
  };
  if (g->state.rewrite(*g, keep_squelch) != 0) return -1;
  g->blocks = 0;
  return 0;
}

int asdr_gate_reset(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  if (g->state.zero(*g) != 0) return -1;
  if (g->device != ASDR_NO_DEVICE && stage_zero(*g, g->d_count, sizeof(int32_t)) != 0) return -1;
  g->blocks = 0;
  return 0;
}

long long asdr_gate_blocks(const asdr_gate_t *g) { return g ? g->blocks : -1; }

int asdr_gate_synchronize(asdr_gate_t *g) {
  if (!g) return fail("null gate");
  return stage_quiesce(*g);
}

}  // extern "C"
