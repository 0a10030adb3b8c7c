// asdr_dcs_host.cpp -- host side + C ABI (include/asdr_dcs.h) of the DCS squelch.  The settings live in host mirrors: the code table
// and the per-channel settings are pushed on the call's stream before a launch when a setter touched them, the scalar ones travel in
// the kernel's arguments; the state records live on the device only (an ASDR_NO_DEVICE handle keeps them on the host instead).
#include <algorithm>
#include <vector>

#include "asdr_dcs_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_dcs_state_t) == 192, "asdr_dcs_state_t is a 192-byte record");
static_assert(sizeof(DcsSetting) == 8, "DcsSetting is 8 bytes");

struct asdr_dcs : StageDev {
  StageMirror<DcsSetting> set;
  StageMirror<uint32_t> words;                 // ASDR_DCS_MAX_CODES code words, 0 from n_codes on
  int codes[ASDR_DCS_MAX_CODES] = {};
  int n_codes = 0, max_errors = 0, confirm = 2, hold_bits = 46;
  StageRecords<asdr_dcs_state_t> state;
  long long blocks = 0;
};

namespace {
const char *kNoDevice = "control-plane-only DCS squelch (ASDR_NO_DEVICE): the signal path needs a HIP device";
const uint32_t kWordMask = 0x7FFFFFu, kPoly = 0xC75u;

// the fields a new table restores; the whole of a creation record around them
void restart_decode(asdr_dcs_state_t &s) {
  s.sr = 0; s.cand = -1; s.age = 255; s.run = 0; s.detected = -1; s.quiet = 0;
}

// (detected = cand = -1, age = 255: creation and reset write records, they do not memset)
asdr_dcs_state_t creation_record() {
  asdr_dcs_state_t s{};
  restart_decode(s);
  return s;
}

uint32_t word_of(int code) {
  const uint32_t d = 0x800u | (uint32_t)code;
  uint32_t r = d << 11;
  for (int k = 22; k >= 11; k--)
    if (r >> k & 1u) r ^= kPoly << (k - 11);
  return r << 12 | d;
}

bool is_rotation(uint32_t t, uint32_t w) {
  for (int k = 0; k < 23; k++)
    if ((((w >> k) | (w << (23 - k))) & kWordMask) == t) return true;
  return false;
}

// the smallest number of differing bits over the pairs of a table; 23 for a table of one
int min_distance(const uint32_t *words, int n) {
  int d = 23;
  for (int i = 0; i < n; i++)
    for (int j = i + 1; j < n; j++) d = std::min(d, __builtin_popcount(words[i] ^ words[j]));
  return d;
}

int check_handle(const asdr_dcs_t *t) { return t ? 0 : fail("null DCS squelch"); }

int check_channel(const asdr_dcs_t *t, int ch, bool all_allowed) { return stage_check_channel(t, ch, all_allowed, "null DCS squelch"); }
}  // namespace

extern "C" {

uint32_t asdr_dcs_word(int code) {
  if (code < 0 || code > ASDR_DCS_MAX_CODE) { fail("code must be in 0..0777"); return 0; }
  return word_of(code);
}

int asdr_dcs_find(const asdr_dcs_t *t, int code, int inverted) {
  if (check_handle(t) != 0) return -1;
  if (code < 0 || code > ASDR_DCS_MAX_CODE) return fail("code must be in 0..0777");
  const uint32_t w = inverted ? word_of(code) ^ kWordMask : word_of(code);
  for (int i = 0; i < t->n_codes; i++)
    if (is_rotation(t->words[i], w)) return i;
  return -1;
}

asdr_dcs_t *asdr_dcs_create(int n_channels, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  asdr_dcs *t = new asdr_dcs;
  t->n = n_channels;
  t->set.host.assign(n_channels, DcsSetting{ASDR_DCS_PASS, 0});
  t->words.host.assign(ASDR_DCS_MAX_CODES, 0u);
  t->n_codes = ASDR_DCS_COUNT;
  for (int i = 0; i < ASDR_DCS_COUNT; i++) { t->codes[i] = ASDR_DCS_CODES[i]; t->words.host[i] = word_of(ASDR_DCS_CODES[i]); }
  if (device == ASDR_NO_DEVICE) {
    t->state.fill(*t, creation_record());
    return t;
  }
  const size_t n = n_channels;
  if (stage_open(*t, device, "dcs") != 0) { asdr_dcs_destroy(t); return nullptr; }
  if (hipMalloc(&t->set.dev, n * sizeof(DcsSetting)) != hipSuccess || hipMalloc(&t->state.dev, n * sizeof(asdr_dcs_state_t)) != hipSuccess ||
      hipMalloc(&t->words.dev, ASDR_DCS_MAX_CODES * sizeof(uint32_t)) != hipSuccess || t->state.fill(*t, creation_record()) != 0 ||
      hipDeviceSynchronize() != hipSuccess) {
    fail("dcs: device allocation failed");
    asdr_dcs_destroy(t);
    return nullptr;
  }
  return t;
}

void asdr_dcs_destroy(asdr_dcs_t *t) {
  if (!t) return;
  stage_close(*t, {t->set.dev, t->state.dev, t->words.dev});
  delete t;
}

int asdr_dcs_n_channels(const asdr_dcs_t *t) { return t ? t->n : fail("null DCS squelch"); }

int asdr_dcs_set_codes(asdr_dcs_t *t, const int *codes, int n_codes) {
  if (check_handle(t) != 0) return -1;
  if (!codes) return fail("null code table");
  if (n_codes < 1 || n_codes > ASDR_DCS_MAX_CODES) return fail("n_codes must be in 1..128");
  uint32_t words[ASDR_DCS_MAX_CODES] = {};
  for (int k = 0; k < n_codes; k++) {
    if (codes[k] < 0 || codes[k] > ASDR_DCS_MAX_CODE) return fail("code " + std::to_string(k) + ": must be in 0..0777");
    words[k] = word_of(codes[k]);
  }
  if (min_distance(words, n_codes) < 2 * t->max_errors + 1)
    return fail("the table's words must differ in at least 2 max_errors + 1 = " + std::to_string(2 * t->max_errors + 1) + " bits");
  if (t->state.rewrite(*t, restart_decode) != 0) return -1;
  std::fill(t->codes, t->codes + ASDR_DCS_MAX_CODES, 0);
  std::copy(codes, codes + n_codes, t->codes);
  std::copy(words, words + ASDR_DCS_MAX_CODES, t->words.host.begin());
  t->n_codes = n_codes;
  t->words.dirty = true;
  return 0;
}

int asdr_dcs_get_codes(const asdr_dcs_t *t, int *codes, uint32_t *words) {
  if (check_handle(t) != 0) return -1;
  if (codes) std::copy(t->codes, t->codes + t->n_codes, codes);
  if (words) std::copy(t->words.host.begin(), t->words.host.begin() + t->n_codes, words);
  return t->n_codes;
}

int asdr_dcs_set_max_errors(asdr_dcs_t *t, int max_errors) {
  if (check_handle(t) != 0) return -1;
  if (max_errors < 0 || max_errors > ASDR_DCS_MAX_ERRORS) return fail("max_errors must be in 0..3");
  if (min_distance(t->words.host.data(), t->n_codes) < 2 * max_errors + 1) return fail("max_errors: the table's words differ in too few bits for it");
  t->max_errors = max_errors;
  return 0;
}

int asdr_dcs_get_max_errors(const asdr_dcs_t *t) { return t ? t->max_errors : fail("null DCS squelch"); }

int asdr_dcs_set_confirm(asdr_dcs_t *t, int confirm) {
  if (check_handle(t) != 0) return -1;
  if (confirm < 1 || confirm > ASDR_DCS_MAX_CONFIRM) return fail("confirm must be in 1..8");
  t->confirm = confirm;
  return 0;
}

int asdr_dcs_get_confirm(const asdr_dcs_t *t) { return t ? t->confirm : fail("null DCS squelch"); }

int asdr_dcs_set_hold_bits(asdr_dcs_t *t, int hold_bits) {
  if (check_handle(t) != 0) return -1;
  if (hold_bits < ASDR_DCS_MIN_HOLD || hold_bits > ASDR_DCS_MAX_HOLD) return fail("hold_bits must be in 23..1023");
  t->hold_bits = hold_bits;
  return 0;
}

int asdr_dcs_get_hold_bits(const asdr_dcs_t *t) { return t ? t->hold_bits : fail("null DCS squelch"); }

int asdr_dcs_set_want(asdr_dcs_t *t, int ch, int want) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (want < ASDR_DCS_PASS || want >= t->n_codes) return fail("want must be ASDR_DCS_PASS, ASDR_DCS_ANY or an entry of the table");
  t->set.apply(ch, [=](DcsSetting &s) { s.want = want; });
  return 0;
}

int asdr_dcs_get_want(const asdr_dcs_t *t, int ch, int *want) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (want) *want = t->set[ch].want;
  return 0;
}

int asdr_dcs_set_hysteresis(asdr_dcs_t *t, int ch, uint32_t hysteresis) {
  if (check_channel(t, ch, true) != 0) return -1;
  t->set.apply(ch, [=](DcsSetting &s) { s.hysteresis = hysteresis; });
  return 0;
}

int asdr_dcs_get_hysteresis(const asdr_dcs_t *t, int ch, uint32_t *hysteresis) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (hysteresis) *hysteresis = t->set[ch].hysteresis;
  return 0;
}

int asdr_dcs_update_device(asdr_dcs_t *t, const int16_t *dIn, long in_stride_blocks, int16_t *dOut, long out_stride_blocks, int n_blocks,
                           void *stream_) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (stage_check_block_rows({{dIn}, t->n, in_stride_blocks}, {{dOut}, t->n, out_stride_blocks}, n_blocks, "output span overlaps the input span") != 0)
    return -1;
  if (n_blocks == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*t, stream) != 0 || t->set.push(stream) != 0 || t->words.push(stream) != 0) return -1;
  DcsArgs a;
  a.in = dIn; a.out = dOut;
  a.in_stride_blocks = in_stride_blocks; a.out_stride_blocks = out_stride_blocks;
  a.n_channels = t->n; a.n_blocks = n_blocks;
  a.n_codes = t->n_codes; a.max_errors = t->max_errors; a.confirm = t->confirm; a.hold_bits = t->hold_bits;
  a.table = t->words.dev; a.set = t->set.dev; a.state = t->state.dev;
  if (asdr_launch_dcs(&a, stream) != 0) return fail("dcs kernel launch failed");
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->blocks += n_blocks;
  return 0;
}

int asdr_dcs_read_state(asdr_dcs_t *t, asdr_dcs_state_t *dst) {
  if (check_handle(t) != 0) return -1;
  return t->state.read(*t, dst);
}

int asdr_dcs_write_state(asdr_dcs_t *t, const int *channels, int n, const asdr_dcs_state_t *src) {
  if (check_handle(t) != 0) return -1;
  const int n_codes = t->n_codes;
  auto check_record = [=](int k, const asdr_dcs_state_t &s) {
    const std::string r = "record " + std::to_string(k);
    if (s.clk >= ASDR_DCS_CLOCK) return fail(r + ": clk must be below 2625");
    if (s.sr > kWordMask) return fail(r + ": sr must be below 2^23");
    if (s.b > 1) return fail(r + ": b must be 0 or 1");
    if (s.open > 1) return fail(r + ": open must be 0 or 1");
    if (s.detected < -1 || s.detected >= n_codes || s.cand < -1 || s.cand >= n_codes)
      return fail(r + ": detected and cand must be -1 or an entry of the table");
    if (s.reserved[0] != 0 || s.reserved[1] != 0) return fail(r + ": reserved fields must be 0");
    return 0;
  };
  return t->state.write(*t, channels, n, src, check_record);
}

int asdr_dcs_clear(asdr_dcs_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->state.rewrite(*t, [](asdr_dcs_state_t &s) { s.bits = s.hits = s.detections = s.openings = s.open_blocks = s.edges = 0; }) != 0) return -1;
  t->blocks = 0;
  return 0;
}

int asdr_dcs_reset(asdr_dcs_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->state.fill(*t, creation_record()) != 0) return -1;
  t->blocks = 0;
  return 0;
}

long long asdr_dcs_blocks(const asdr_dcs_t *t) { return t ? t->blocks : -1; }

int asdr_dcs_synchronize(asdr_dcs_t *t) {
  if (check_handle(t) != 0) return -1;
  return stage_quiesce(*t);
}

}  // extern "C"
