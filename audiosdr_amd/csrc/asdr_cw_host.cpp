// asdr_cw_host.cpp -- host side + C ABI (include/asdr_cw.h) of the CW decoder.  The per-channel settings live in a host mirror that
// is pushed on the call's stream before a launch when a setter touched it; the state records, the rings and their bookkeeping live on
// the device only (an ASDR_NO_DEVICE handle keeps the records and an all-empty bookkeeping on the host instead).  The mixer's table
// is computed once, from its formula, and uploaded at creation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "asdr_cw_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_cw_state_t) == 80 && offsetof(asdr_cw_state_t, reserved) == ASDR_CW_LOADED_BYTES, "asdr_cw_state_t is an 80-byte record");
static_assert(offsetof(asdr_cw_state_t, hi) == 28 && offsetof(asdr_cw_state_t, D) == 36 && offsetof(asdr_cw_state_t, cnt) == 60, "the record's offsets");
static_assert(sizeof(asdr_cw_event_t) == 16 && offsetof(asdr_cw_event_t, ch) == 12, "asdr_cw_event_t is a 16-byte slot");
static_assert(sizeof(CwRing) == 16 && sizeof(CwSetting) == 16, "CwRing and CwSetting are 16 bytes");

struct asdr_cw : StageDev {
  int ring = 0;
  StageMirror<CwSetting> set;
  StageRecords<asdr_cw_state_t> state;
  long long blocks = 0;
  uint32_t *d_table = nullptr, *d_tile_count = nullptr, *d_index = nullptr, *d_count = nullptr;
  CwRing *d_rings = nullptr;
  asdr_cw_event_t *d_slots = nullptr;
  void *d_events = nullptr;                      // deliver's, grown on demand
  size_t events_cap = 0;
};

namespace {
const char *kNoDevice = "control-plane-only CW decoder (ASDR_NO_DEVICE): the signal path and the delivery need a HIP device";
const char *kNull = "null CW decoder";

// C[j] = floor(1024 cos(2 pi j / 1024) + 0.5)
const std::vector<int16_t> &cos_table() {
  static const std::vector<int16_t> table = [] {
    std::vector<int16_t> c(ASDR_CW_TABLE_WORDS);
    for (int j = 0; j < ASDR_CW_TABLE_WORDS; j++) c[j] = (int16_t)std::floor(1024.0 * std::cos(2.0 * M_PI * j / 1024.0) + 0.5);
    return c;
  }();
  return table;
}

uint32_t step_of(double hz) { return (uint32_t)std::floor(hz * 4294967296.0 / 44100.0 + 0.5); }
uint32_t dit_of(int wpm) { return (uint32_t)((ASDR_CW_DIT_UNITS + wpm / 2) / wpm); }

asdr_cw_state_t creation_record() {
  asdr_cw_state_t s{};
  s.D = dit_of(ASDR_CW_WPM);
  s.sym = 1;
  return s;
}

int check_handle(const asdr_cw_t *t) { return t ? 0 : fail(kNull); }

int check_channel(const asdr_cw_t *t, int ch, bool all_allowed) { return stage_check_channel(t, ch, all_allowed, kNull); }

// the creation record into every channel (D and sym are not 0: records are written, not memset) and empty rings
int creation_state(asdr_cw_t *t) {
  if (t->state.fill(*t, creation_record()) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipMemsetAsync(t->d_rings, 0, (size_t)t->n * sizeof(CwRing), t->stream));
  HIPCHK(hipMemsetAsync(t->d_slots, 0, (size_t)t->n * t->ring * sizeof(asdr_cw_event_t), t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));   // the fills are done on return: a call on any stream may follow
  return 0;
}

int collect(asdr_cw_t *t, uint32_t *dCount, asdr_cw_event_t *dEvents, int max_events, hipStream_t stream) {
  if (stage_before_launch(*t, stream) != 0) return -1;
  CwCollectArgs a;
  a.n_channels = t->n; a.max_events = max_events; a.ring = (uint32_t)t->ring;
  a.rings = t->d_rings; a.slots = t->d_slots; a.tile_count = t->d_tile_count; a.index = t->d_index;
  a.count = dCount; a.events = dEvents;
  if (asdr_launch_cw_collect(&a, stream) != 0) return fail("CW collect launch failed");
  return stage_after_launch(*t, stream);
}

int check_max_events(int max_events) {
  return max_events < 0 || max_events > ASDR_CW_MAX_EVENTS ? fail("max_events must be in 0..67108864") : 0;
}
}  // namespace

extern "C" {

uint32_t asdr_cw_pitch_step(double hz) {
  if (!(hz >= 100.0 && hz <= 3000.0)) { fail("pitch must be in 100..3000 Hz"); return 0; }
  return step_of(hz);
}

int asdr_cw_cos(int j) { return cos_table()[j & (ASDR_CW_TABLE_WORDS - 1)]; }

asdr_cw_t *asdr_cw_create(int n_channels, int ring, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  if (ring < 1 || ring > ASDR_CW_MAX_RING) { fail("ring must be in 1..64"); return nullptr; }
  asdr_cw *t = new asdr_cw;
  t->n = n_channels;
  t->ring = ring;
  t->set.host.assign(n_channels, CwSetting{step_of(ASDR_CW_PITCH_HZ), ASDR_CW_MIN_POWER, ASDR_CW_GLITCH, 1u});
  if (device == ASDR_NO_DEVICE) {
    creation_state(t);
    return t;
  }
  const size_t n = n_channels, n_tiles = (n + ASDR_CW_TILE - 1) / ASDR_CW_TILE;
  std::vector<uint32_t> words(ASDR_CW_TABLE_WORDS);
  for (int j = 0; j < ASDR_CW_TABLE_WORDS; j++)
    words[j] = ((uint32_t)(uint16_t)cos_table()[j]) | ((uint32_t)(uint16_t)cos_table()[(j - 256) & (ASDR_CW_TABLE_WORDS - 1)] << 16);
  if (stage_open(*t, device, "CW") != 0) { asdr_cw_destroy(t); return nullptr; }
  if (hipMalloc(&t->set.dev, n * sizeof(CwSetting)) != hipSuccess || hipMalloc(&t->state.dev, n * sizeof(asdr_cw_state_t)) != hipSuccess ||
      hipMalloc(&t->d_rings, n * sizeof(CwRing)) != hipSuccess || hipMalloc(&t->d_slots, n * ring * sizeof(asdr_cw_event_t)) != hipSuccess ||
      hipMalloc(&t->d_tile_count, n_tiles * sizeof(uint32_t)) != hipSuccess || hipMalloc(&t->d_index, n * ring * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t->d_count, 16) != hipSuccess || hipMalloc(&t->d_table, words.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(t->d_table, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess || creation_state(t) != 0 ||
      hipDeviceSynchronize() != hipSuccess) {
    fail("CW: device allocation failed");
    asdr_cw_destroy(t);
    return nullptr;
  }
  return t;
}

void asdr_cw_destroy(asdr_cw_t *t) {
  if (!t) return;
  stage_close(*t, {t->set.dev, t->state.dev, t->d_rings, t->d_slots, t->d_tile_count, t->d_index, t->d_count, t->d_table, t->d_events});
  delete t;
}

int asdr_cw_n_channels(const asdr_cw_t *t) { return t ? t->n : fail(kNull); }

int asdr_cw_set_pitch_step(asdr_cw_t *t, int ch, uint32_t pitch_step) {
  if (check_channel(t, ch, true) != 0) return -1;
  t->set.apply(ch, [=](CwSetting &s) { s.pitch_step = pitch_step; });
  return 0;
}

int asdr_cw_set_min_power(asdr_cw_t *t, int ch, uint32_t min_power) {
  if (check_channel(t, ch, true) != 0) return -1;
  t->set.apply(ch, [=](CwSetting &s) { s.min_power = min_power; });
  return 0;
}

int asdr_cw_set_glitch(asdr_cw_t *t, int ch, int glitch) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (glitch < 1 || glitch > ASDR_CW_MAX_GLITCH) return fail("glitch must be in 1..16");
  t->set.apply(ch, [=](CwSetting &s) { s.glitch = (uint32_t)glitch; });
  return 0;
}

int asdr_cw_set_track(asdr_cw_t *t, int ch, int track) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (track != 0 && track != 1) return fail("track must be 0 or 1");
  t->set.apply(ch, [=](CwSetting &s) { s.track = (uint32_t)track; });
  return 0;
}

int asdr_cw_get_settings(const asdr_cw_t *t, int ch, uint32_t *pitch_step, uint32_t *min_power, int *glitch, int *track) {
  if (check_channel(t, ch, false) != 0) return -1;
  const CwSetting &s = t->set[ch];
  if (pitch_step) *pitch_step = s.pitch_step;
  if (min_power) *min_power = s.min_power;
  if (glitch) *glitch = (int)s.glitch;
  if (track) *track = (int)s.track;
  return 0;
}

int asdr_cw_set_speed(asdr_cw_t *t, int ch, int wpm) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (wpm < ASDR_CW_MIN_WPM || wpm > ASDR_CW_MAX_WPM) return fail("wpm must be in 5..60");
  const uint32_t D = dit_of(wpm);
  if (ch == ASDR_ALL) return t->state.rewrite(*t, [=](asdr_cw_state_t &s) { s.D = D; });
  if (t->device == ASDR_NO_DEVICE) { t->state.host[ch].D = D; return 0; }
  if (stage_quiesce(*t) != 0) return -1;
  HIPCHK(hipMemcpy(&t->state.dev[ch].D, &D, sizeof(D), hipMemcpyHostToDevice));
  return 0;
}

int asdr_cw_update_device(asdr_cw_t *t, const int16_t *dIn, long in_stride_blocks, int n_blocks, void *stream_) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (stage_check_block_rows({{dIn}, t->n, in_stride_blocks}, {}, n_blocks, nullptr) != 0) return -1;
  if (n_blocks == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*t, stream) != 0 || t->set.push(stream) != 0) return -1;
  CwArgs a;
  a.in = dIn; a.in_stride_blocks = in_stride_blocks;
  a.n_channels = t->n; a.n_blocks = n_blocks;
  a.ring = (uint32_t)t->ring; a.block0 = (uint32_t)t->blocks;
  a.set = t->set.dev; a.table = t->d_table; a.state = t->state.dev; a.rings = t->d_rings; a.slots = t->d_slots;
  if (asdr_launch_cw(&a, stream) != 0) return fail("CW kernel launch failed");
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->blocks += n_blocks;
  return 0;
}

int asdr_cw_collect_device(asdr_cw_t *t, uint32_t *dCount, asdr_cw_event_t *dEvents, int max_events, void *stream) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (check_max_events(max_events) != 0) return -1;
  if (!dCount || (!dEvents && max_events > 0)) return fail("null device pointer");
  if (((uintptr_t)dCount & 3u) != 0 || ((uintptr_t)dEvents & 15u) != 0) return fail("dCount must be 4-byte and dEvents 16-byte aligned");
  return collect(t, dCount, dEvents, max_events, (hipStream_t)stream);
}

int asdr_cw_deliver(asdr_cw_t *t, uint32_t *count, asdr_cw_event_t *host_events, int max_events) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (check_max_events(max_events) != 0) return -1;
  if (!count || (!host_events && max_events > 0)) return fail("null destination");
  const size_t rows = std::min((size_t)max_events, (size_t)t->n * t->ring);
  HIPCHK(hipSetDevice(t->device));
  if (stage_reserve(*t, &t->d_events, &t->events_cap, std::max(rows, (size_t)1) * sizeof(asdr_cw_event_t)) != 0) return -1;
  if (collect(t, t->d_count, (asdr_cw_event_t *)t->d_events, max_events, t->stream) != 0) return -1;
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, t->d_count, sizeof(n), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(host_events, t->d_events, (size_t)n * sizeof(asdr_cw_event_t), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
  }
  *count = n;
  return 0;
}

int asdr_cw_ring_state(asdr_cw_t *t, uint32_t *pending, uint32_t *lost) {
  if (check_handle(t) != 0) return -1;
  std::vector<CwRing> g(t->n, CwRing{0, 0, 0, 0});
  if (t->device != ASDR_NO_DEVICE) {
    if (stage_quiesce(*t) != 0) return -1;
    HIPCHK(hipMemcpy(g.data(), t->d_rings, g.size() * sizeof(CwRing), hipMemcpyDeviceToHost));
  }
  for (int c = 0; c < t->n; c++) {
    if (pending) pending[c] = g[c].head - g[c].taken;
    if (lost) lost[c] = g[c].lost;
  }
  return 0;
}

int asdr_cw_read_state(asdr_cw_t *t, asdr_cw_state_t *dst) {
  if (check_handle(t) != 0) return -1;
  return t->state.read(*t, dst);
}

int asdr_cw_write_state(asdr_cw_t *t, const int *channels, int n, const asdr_cw_state_t *src) {
  if (check_handle(t) != 0) return -1;
  auto check_record = [](int k, const asdr_cw_state_t &s) {
    const std::string r = "record " + std::to_string(k);
    if (s.D < ASDR_CW_MIN_D || s.D > ASDR_CW_MAX_D) return fail(r + ": D must be in 441..5292");
    if (s.key > 1) return fail(r + ": key must be 0 or 1");
    if (s.gap > 1) return fail(r + ": gap must be 0 or 1");
    if (s.cnt > ASDR_CW_MAX_GLITCH) return fail(r + ": cnt must be at most 16");
    for (int j = 0; j < 3; j++)
      if (s.prev_i[j] < -(1 << 20) || s.prev_i[j] > (1 << 20) || s.prev_q[j] < -(1 << 20) || s.prev_q[j] > (1 << 20))
        return fail(r + ": prev_i and prev_q must be within +-1048576");
    for (uint32_t v : s.reserved)
      if (v != 0) return fail(r + ": reserved fields must be 0");
    return 0;
  };
  return t->state.write(*t, channels, n, src, check_record);
}

int asdr_cw_clear(asdr_cw_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) {
    for (asdr_cw_state_t &s : t->state.host) s.marks = s.unknown = s.glitches = 0;
  } else {   // one launch zeroes the three counters and lost of every channel: all of it or, if the launch fails, none
    if (stage_quiesce(*t) != 0) return -1;
    if (asdr_launch_cw_clear(t->state.dev, t->d_rings, t->n, t->stream) != 0) return fail("CW clear launch failed");
    HIPCHK(hipStreamSynchronize(t->stream));
  }
  t->blocks = 0;
  return 0;
}

int asdr_cw_reset(asdr_cw_t *t) {
  if (check_handle(t) != 0) return -1;
  if (creation_state(t) != 0) return -1;
  t->blocks = 0;
  return 0;
}

long long asdr_cw_blocks(const asdr_cw_t *t) { return t ? t->blocks : -1; }

int asdr_cw_synchronize(asdr_cw_t *t) {
  if (check_handle(t) != 0) return -1;
  return stage_quiesce(*t);
}

}  // extern "C"
