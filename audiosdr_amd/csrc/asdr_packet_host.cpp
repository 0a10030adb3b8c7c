// asdr_packet_host.cpp -- host side + C ABI (include/asdr_packet.h) of the packet decoder.  The per-channel setting lives in a host
// mirror that is pushed on the call's stream before a launch when a setter touched it; the state records, the rings and their
// bookkeeping live on the device only (an ASDR_NO_DEVICE handle keeps the records and an all-empty bookkeeping on the host instead).
#include <algorithm>
#include <cstdio>
#include <vector>

#include "asdr_packet_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_packet_state_t) == 448 && offsetof(asdr_packet_state_t, buf) == 112, "asdr_packet_state_t is a 448-byte record");
static_assert(offsetof(asdr_packet_state_t, reserved) + 12 == ASDR_PACKET_LOADED_BYTES, "a call loads and stores the fields and three reserved words");
static_assert(sizeof(asdr_packet_frame_t) == 352 && sizeof(asdr_packet_frame_t) == 16 * ASDR_PACKET_SLOT_PIECES, "asdr_packet_frame_t is a 352-byte slot");
static_assert(sizeof(PacketRing) == 16, "PacketRing is 16 bytes");

struct asdr_packet : StageDev {
  int ring = 0;
  StageMirror<uint32_t> boost;
  StageRecords<asdr_packet_state_t> state;
  long long blocks = 0;
  uint32_t *d_tile_count = nullptr, *d_index = nullptr, *d_count = nullptr;
  PacketRing *d_rings = nullptr;
  asdr_packet_frame_t *d_slots = nullptr;
  void *d_frames = nullptr;                      // deliver's, grown on demand
  size_t frames_cap = 0;
};

namespace {
const char *kNoDevice = "control-plane-only packet decoder (ASDR_NO_DEVICE): the signal path and the delivery need a HIP device";

asdr_packet_state_t creation_record() {
  asdr_packet_state_t s{};
  s.crc = 0xFFFF;
  return s;
}

uint16_t crc_of(const uint8_t *bytes, size_t n) {
  uint32_t crc = 0xFFFFu;
  for (size_t k = 0; k < n; k++)
    for (int s = 0; s < 8; s++) crc = (crc >> 1) ^ (((crc ^ (bytes[k] >> s)) & 1u) ? 0x8408u : 0u);
  return (uint16_t)crc;
}

int check_handle(const asdr_packet_t *t) { return t ? 0 : fail("null packet decoder"); }

int check_channel(const asdr_packet_t *t, int ch, bool all_allowed) { return stage_check_channel(t, ch, all_allowed, "null packet decoder"); }

// the creation record into every channel (crc = 0xFFFF: records are written, not memset) and empty rings
int creation_state(asdr_packet_t *t) {
  if (t->state.fill(*t, creation_record()) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipMemsetAsync(t->d_rings, 0, (size_t)t->n * sizeof(PacketRing), t->stream));
  HIPCHK(hipMemsetAsync(t->d_slots, 0, (size_t)t->n * t->ring * sizeof(asdr_packet_frame_t), t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));   // the fills are done on return: a call on any stream may follow
  return 0;
}

int collect(asdr_packet_t *t, uint32_t *dCount, asdr_packet_frame_t *dFrames, int max_frames, hipStream_t stream) {
  if (stage_before_launch(*t, stream) != 0) return -1;
  PacketCollectArgs a;
  a.n_channels = t->n; a.max_frames = max_frames; a.ring = (uint32_t)t->ring;
  a.rings = t->d_rings; a.slots = t->d_slots; a.tile_count = t->d_tile_count; a.index = t->d_index;
  a.count = dCount; a.frames = dFrames;
  if (asdr_launch_packet_collect(&a, stream) != 0) return fail("packet collect launch failed");
  return stage_after_launch(*t, stream);
}

int check_max_frames(int max_frames) {
  return max_frames < 0 || max_frames > ASDR_PACKET_MAX_FRAMES ? fail("max_frames must be in 0..16777216") : 0;
}
}  // namespace

extern "C" {

uint16_t asdr_packet_fcs(const uint8_t *bytes, size_t n) {
  if (!bytes && n > 0) { fail("null bytes"); return 0; }
  return (uint16_t)~crc_of(bytes, n);
}

int asdr_packet_format_address(const uint8_t *frame, int length, char *out, int out_size) {
  if (!frame || !out) return fail("null pointer");
  if (length < 14) return fail("an address field is at least 14 bytes");
  std::string call[10];
  bool repeated[10] = {};
  int n = 0;
  for (bool last = false; !last; n++) {
    if (n == 10 || 7 * n + 7 > length) return fail("address field: no end mark within 10 addresses");
    const uint8_t *a = frame + 7 * n;
    for (int k = 0; k < 6; k++) {
      const int ch = a[k] >> 1;
      if ((a[k] & 1) || ch < 0x20 || ch > 0x7E) return fail("address " + std::to_string(n) + ": not a shifted printable character");
      if (ch != ' ') call[n] += (char)ch;
    }
    const int ssid = (a[6] >> 1) & 15;
    if (ssid) call[n] += "-" + std::to_string(ssid);
    repeated[n] = n >= 2 && (a[6] & 0x80);
    last = a[6] & 1;
  }
  if (n < 2) return fail("address field: the end mark is in the destination");
  std::string s = call[1] + ">" + call[0];
  for (int k = 2; k < n; k++) s += "," + call[k] + (repeated[k] ? "*" : "");
  if ((int)s.size() + 1 > out_size) return fail("out_size too small");
  std::memcpy(out, s.c_str(), s.size() + 1);
  return (int)s.size();
}

asdr_packet_t *asdr_packet_create(int n_channels, int ring, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  if (ring < 1 || ring > ASDR_PACKET_MAX_RING) { fail("ring must be in 1..16"); return nullptr; }
  asdr_packet *t = new asdr_packet;
  t->n = n_channels;
  t->ring = ring;
  t->boost.host.assign(n_channels, 256u);
  if (device == ASDR_NO_DEVICE) {
    creation_state(t);
    return t;
  }
  const size_t n = n_channels, n_tiles = (n + ASDR_PACKET_TILE - 1) / ASDR_PACKET_TILE;
  if (stage_open(*t, device, "packet") != 0) { asdr_packet_destroy(t); return nullptr; }
  if (hipMalloc(&t->boost.dev, n * sizeof(uint32_t)) != hipSuccess || hipMalloc(&t->state.dev, n * sizeof(asdr_packet_state_t)) != hipSuccess ||
      hipMalloc(&t->d_rings, n * sizeof(PacketRing)) != hipSuccess || hipMalloc(&t->d_slots, n * ring * sizeof(asdr_packet_frame_t)) != hipSuccess ||
      hipMalloc(&t->d_tile_count, n_tiles * sizeof(uint32_t)) != hipSuccess || hipMalloc(&t->d_index, n * ring * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&t->d_count, 16) != hipSuccess || creation_state(t) != 0 || hipDeviceSynchronize() != hipSuccess) {
    fail("packet: device allocation failed");
    asdr_packet_destroy(t);
    return nullptr;
  }
  return t;
}

void asdr_packet_destroy(asdr_packet_t *t) {
  if (!t) return;
  stage_close(*t, {t->boost.dev, t->state.dev, t->d_rings, t->d_slots, t->d_tile_count, t->d_index, t->d_count, t->d_frames});
  delete t;
}

int asdr_packet_n_channels(const asdr_packet_t *t) { return t ? t->n : fail("null packet decoder"); }

int asdr_packet_set_space_boost(asdr_packet_t *t, int ch, uint32_t space_boost) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (space_boost < ASDR_PACKET_MIN_BOOST || space_boost > ASDR_PACKET_MAX_BOOST) return fail("space_boost must be in 64..4096");
  t->boost.apply(ch, [=](uint32_t &b) { b = space_boost; });
  return 0;
}

int asdr_packet_get_space_boost(const asdr_packet_t *t, int ch, uint32_t *space_boost) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (space_boost) *space_boost = t->boost[ch];
  return 0;
}

int asdr_packet_update_device(asdr_packet_t *t, const int16_t *dIn, long in_stride_blocks, int n_blocks, void *stream_) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (stage_check_block_rows({{dIn}, t->n, in_stride_blocks}, {}, n_blocks, nullptr) != 0) return -1;
  if (n_blocks == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*t, stream) != 0 || t->boost.push(stream) != 0) return -1;
  PacketArgs a;
  a.in = dIn; a.in_stride_blocks = in_stride_blocks;
  a.n_channels = t->n; a.n_blocks = n_blocks;
  a.ring = (uint32_t)t->ring; a.block0 = (uint32_t)t->blocks;
  a.boost = t->boost.dev; a.state = t->state.dev; a.rings = t->d_rings; a.slots = t->d_slots;
  if (asdr_launch_packet(&a, stream) != 0) return fail("packet kernel launch failed");
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->blocks += n_blocks;
  return 0;
}

int asdr_packet_collect_device(asdr_packet_t *t, uint32_t *dCount, asdr_packet_frame_t *dFrames, int max_frames, void *stream) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (check_max_frames(max_frames) != 0) return -1;
  if (!dCount || (!dFrames && max_frames > 0)) return fail("null device pointer");
  if (((uintptr_t)dCount & 3u) != 0 || ((uintptr_t)dFrames & 15u) != 0) return fail("dCount must be 4-byte and dFrames 16-byte aligned");
  return collect(t, dCount, dFrames, max_frames, (hipStream_t)stream);
}

int asdr_packet_deliver(asdr_packet_t *t, uint32_t *count, asdr_packet_frame_t *host_frames, int max_frames) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (check_max_frames(max_frames) != 0) return -1;
  if (!count || (!host_frames && max_frames > 0)) return fail("null destination");
  const size_t rows = std::min((size_t)max_frames, (size_t)t->n * t->ring);
  HIPCHK(hipSetDevice(t->device));
  if (stage_reserve(*t, &t->d_frames, &t->frames_cap, std::max(rows, (size_t)1) * sizeof(asdr_packet_frame_t)) != 0) return -1;
  if (collect(t, t->d_count, (asdr_packet_frame_t *)t->d_frames, max_frames, t->stream) != 0) return -1;
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, t->d_count, sizeof(n), hipMemcpyDeviceToHost, t->stream));
  HIPCHK(hipStreamSynchronize(t->stream));
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(host_frames, t->d_frames, (size_t)n * sizeof(asdr_packet_frame_t), hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
  }
  *count = n;
  return 0;
}

int asdr_packet_ring_state(asdr_packet_t *t, uint32_t *pending, uint32_t *lost) {
  if (check_handle(t) != 0) return -1;
  std::vector<PacketRing> g(t->n, PacketRing{0, 0, 0, 0});
  if (t->device != ASDR_NO_DEVICE) {
    if (stage_quiesce(*t) != 0) return -1;
    HIPCHK(hipMemcpy(g.data(), t->d_rings, g.size() * sizeof(PacketRing), hipMemcpyDeviceToHost));
  }
  for (int c = 0; c < t->n; c++) {
    if (pending) pending[c] = g[c].head - g[c].taken;
    if (lost) lost[c] = g[c].lost;
  }
  return 0;
}

int asdr_packet_read_state(asdr_packet_t *t, asdr_packet_state_t *dst) {
  if (check_handle(t) != 0) return -1;
  return t->state.read(*t, dst);
}

int asdr_packet_write_state(asdr_packet_t *t, const int *channels, int n, const asdr_packet_state_t *src) {
  if (check_handle(t) != 0) return -1;
  auto check_record = [](int k, const asdr_packet_state_t &s) {
    const std::string r = "record " + std::to_string(k);
    if (s.clk >= ASDR_PACKET_CLOCK) return fail(r + ": clk must be below 147");
    if (s.len > ASDR_PACKET_MAX_LEN) return fail(r + ": len must be at most 332");
    if (s.nb >= 8) return fail(r + ": nb must be below 8");
    if (s.b > 1) return fail(r + ": b must be 0 or 1");
    if (s.prev > 1) return fail(r + ": prev must be 0 or 1");
    if (s.in_frame > 1) return fail(r + ": in_frame must be 0 or 1");
    for (uint32_t v : s.reserved)
      if (v != 0) return fail(r + ": reserved fields must be 0");
    return 0;
  };
  return t->state.write(*t, channels, n, src, check_record);
}

int asdr_packet_clear(asdr_packet_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) {
    for (asdr_packet_state_t &s : t->state.host) s.bits = s.edges = s.flags = s.crc_errors = s.aborts = 0;
  } else {   // one launch zeroes the five counters and lost of every channel: all of it or, if the launch fails, none
    if (stage_quiesce(*t) != 0) return -1;
    if (asdr_launch_packet_clear(t->state.dev, t->d_rings, t->n, t->stream) != 0) return fail("packet clear launch failed");
    HIPCHK(hipStreamSynchronize(t->stream));
  }
  t->blocks = 0;
  return 0;
}

int asdr_packet_reset(asdr_packet_t *t) {
  if (check_handle(t) != 0) return -1;
  if (creation_state(t) != 0) return -1;
  t->blocks = 0;
  return 0;
}

long long asdr_packet_blocks(const asdr_packet_t *t) { return t ? t->blocks : -1; }

int asdr_packet_synchronize(asdr_packet_t *t) {
  if (check_handle(t) != 0) return -1;
  return stage_quiesce(*t);
}

}  // extern "C"
