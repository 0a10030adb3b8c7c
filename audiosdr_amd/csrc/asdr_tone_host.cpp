// asdr_tone_host.cpp -- host side + C ABI (include/asdr_tone.h) of the tone squelch.  The settings live in host mirrors that are
// pushed before a launch when a setter touched them (the scalar ones travel in the kernel's arguments); the state records live on
// the device only (an ASDR_NO_DEVICE handle keeps them on the host instead).
#include <algorithm>
#include <cmath>
#include <vector>

#include "asdr_stage_host.h"
#include "asdr_tone_device.h"

static_assert(sizeof(asdr_tone_state_t) == 704, "asdr_tone_state_t is a 704-byte record");
static_assert(sizeof(ToneSetting) == 16, "ToneSetting is 16 bytes");

struct asdr_tone : StageDev {
  StageMirror<ToneSetting> set;
  StageMirror<uint32_t> steps;                 // ASDR_TONE_MAX_TONES phase steps, 0 from n_tones on
  double hz[ASDR_TONE_MAX_TONES] = {};
  int n_tones = 0, window = 64, dominance = 64, sections = 0;
  int32_t coef[ASDR_TONE_MAX_SECTIONS][5] = {};
  StageRecords<asdr_tone_state_t> state;
  long long blocks = 0;
  uint32_t *d_table = nullptr;
};

namespace {
const char *kNoDevice = "control-plane-only tone squelch (ASDR_NO_DEVICE): the signal path needs a HIP device";
const double kFs = 44100.0, kPi = 3.14159265358979323846;

asdr_tone_state_t creation_record() {
  asdr_tone_state_t s{};
  s.detected = s.last_best = -1;
  return s;
}

int check_handle(const asdr_tone_t *t) { return t ? 0 : fail("null tone squelch"); }

int check_channel(const asdr_tone_t *t, int ch, bool all_allowed) { return stage_check_channel(t, ch, all_allowed, "null tone squelch"); }

// the phase steps of a table, or -1 with the reason
int steps_of(const double *hz, int n, uint32_t *steps) {
  if (!hz) return fail("null tone table");
  if (n < 1 || n > ASDR_TONE_MAX_TONES) return fail("n_tones must be in 1..64");
  for (int k = 0; k < n; k++) {
    if (!(hz[k] > 0.0 && hz[k] < ASDR_TONE_MAX_HZ)) return fail("tone " + std::to_string(k) + ": must be above 0 and below 1378 Hz");
    steps[k] = (uint32_t)std::floor(hz[k] * 16.0 * 4294967296.0 / kFs + 0.5);
    if (k > 0 && steps[k] <= steps[k - 1]) return fail("tone " + std::to_string(k) + ": the table must ascend strictly");
  }
  return 0;
}

// a new table or window: every channel's window starts again
int restart_windows(asdr_tone_t *t) {
  return t->state.rewrite(*t, [](asdr_tone_state_t &s) { std::fill(&s.acc[0][0], &s.acc[0][0] + 2 * ASDR_TONE_MAX_TONES, 0); s.window_block = 0; });
}
}  // namespace

extern "C" {

int asdr_tone_highpass_design(double fc_hz, int sections, int32_t *out) {
  if (sections < 0 || sections > ASDR_TONE_MAX_SECTIONS) return fail("sections must be in 0..3");
  if (sections == 0) return 0;
  if (!out) return fail("null coefficients");
  if (!(fc_hz > 0.0 && fc_hz < kFs / 2.0)) return fail("fc_hz must be above 0 and below 22050");
  const double K = std::tan(kPi * fc_hz / kFs);
  int32_t c[ASDR_TONE_MAX_SECTIONS][5];
  for (int k = 0; k < sections; k++) {
    const double q = 2.0 * std::sin(kPi * (2 * k + 1) / (4.0 * sections));
    const double n = 1.0 / (1.0 + q * K + K * K);
    const double v[5] = {n, -2.0 * n, n, 2.0 * (K * K - 1.0) * n, (1.0 - q * K + K * K) * n};
    for (int j = 0; j < 5; j++) c[k][j] = (int32_t)std::floor(v[j] * 268435456.0 + 0.5);   // |v| < 2
  }
  std::copy(&c[0][0], &c[0][0] + 5 * sections, out);
  return 0;
}

uint64_t asdr_tone_min_power(double amplitude, int window_blocks) {
  if (window_blocks < ASDR_TONE_MIN_WINDOW || window_blocks > ASDR_TONE_MAX_WINDOW) { fail("window must be in 16..128"); return 0; }
  if (!(amplitude >= 0.0 && amplitude <= 32768.0)) { fail("amplitude must be in 0..32768"); return 0; }
  const double a = 128.0 * amplitude * window_blocks;   // <= 2^29
  return (uint64_t)std::floor(a * a / 4.0);
}

asdr_tone_t *asdr_tone_create(int n_channels, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  asdr_tone *t = new asdr_tone;
  t->n = n_channels;
  t->set.host.assign(n_channels, ToneSetting{0, ASDR_TONE_PASS, 0});
  t->steps.host.assign(ASDR_TONE_MAX_TONES, 0u);
  t->n_tones = ASDR_CTCSS_COUNT;
  std::copy(ASDR_CTCSS_TONES, ASDR_CTCSS_TONES + ASDR_CTCSS_COUNT, t->hz);
  steps_of(t->hz, t->n_tones, t->steps.host.data());
  if (device == ASDR_NO_DEVICE) {
    t->state.fill(*t, creation_record());
    return t;
  }
  const size_t n = n_channels;
  if (stage_open(*t, device, "tone") != 0) { asdr_tone_destroy(t); return nullptr; }
  std::vector<uint32_t> table(ASDR_TONE_TABLE);
  int C[ASDR_TONE_TABLE];
  for (int j = 0; j < ASDR_TONE_TABLE; j++) C[j] = (int)std::floor(16384.0 * std::cos(2.0 * kPi * j / ASDR_TONE_TABLE) + 0.5);
  for (int j = 0; j < ASDR_TONE_TABLE; j++) table[j] = ((uint32_t)C[j] & 0xFFFFu) | ((uint32_t)C[(j - 256) & (ASDR_TONE_TABLE - 1)] << 16);
  if (hipMalloc(&t->set.dev, n * sizeof(ToneSetting)) != hipSuccess || hipMalloc(&t->state.dev, n * sizeof(asdr_tone_state_t)) != hipSuccess ||
      hipMalloc(&t->steps.dev, ASDR_TONE_MAX_TONES * sizeof(uint32_t)) != hipSuccess || hipMalloc(&t->d_table, ASDR_TONE_TABLE * sizeof(uint32_t)) != hipSuccess ||
      hipMemcpy(t->d_table, table.data(), ASDR_TONE_TABLE * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
      t->state.fill(*t, creation_record()) != 0 || hipDeviceSynchronize() != hipSuccess) {
    fail("tone: device allocation failed");
    asdr_tone_destroy(t);
    return nullptr;
  }
  return t;
}

void asdr_tone_destroy(asdr_tone_t *t) {
  if (!t) return;
  stage_close(*t, {t->set.dev, t->state.dev, t->steps.dev, t->d_table});
  delete t;
}

int asdr_tone_n_channels(const asdr_tone_t *t) { return t ? t->n : fail("null tone squelch"); }

int asdr_tone_set_tones(asdr_tone_t *t, const double *hz, int n_tones) {
  if (check_handle(t) != 0) return -1;
  uint32_t steps[ASDR_TONE_MAX_TONES] = {};
  if (steps_of(hz, n_tones, steps) != 0) return -1;
  if (restart_windows(t) != 0) return -1;
  std::fill(t->hz, t->hz + ASDR_TONE_MAX_TONES, 0.0);
  std::copy(hz, hz + n_tones, t->hz);
  std::copy(steps, steps + ASDR_TONE_MAX_TONES, t->steps.host.begin());
  t->n_tones = n_tones;
  t->steps.dirty = true;
  return 0;
}

int asdr_tone_get_tones(const asdr_tone_t *t, double *hz, uint32_t *steps) {
  if (check_handle(t) != 0) return -1;
  if (hz) std::copy(t->hz, t->hz + t->n_tones, hz);
  if (steps) std::copy(t->steps.host.begin(), t->steps.host.begin() + t->n_tones, steps);
  return t->n_tones;
}

int asdr_tone_set_window(asdr_tone_t *t, int window_blocks) {
  if (check_handle(t) != 0) return -1;
  if (window_blocks < ASDR_TONE_MIN_WINDOW || window_blocks > ASDR_TONE_MAX_WINDOW) return fail("window must be in 16..128");
  if (restart_windows(t) != 0) return -1;
  t->window = window_blocks;
  return 0;
}

int asdr_tone_get_window(const asdr_tone_t *t) { return t ? t->window : fail("null tone squelch"); }

int asdr_tone_set_dominance(asdr_tone_t *t, int dominance_q4) {
  if (check_handle(t) != 0) return -1;
  if (dominance_q4 < ASDR_TONE_MIN_DOMINANCE || dominance_q4 > ASDR_TONE_MAX_DOMINANCE) return fail("dominance must be in 16..1024");
  t->dominance = dominance_q4;
  return 0;
}

int asdr_tone_get_dominance(const asdr_tone_t *t) { return t ? t->dominance : fail("null tone squelch"); }

int asdr_tone_set_highpass(asdr_tone_t *t, const int32_t *coefficients, int sections) {
  if (check_handle(t) != 0) return -1;
  if (sections < 0 || sections > ASDR_TONE_MAX_SECTIONS) return fail("sections must be in 0..3");
  if (sections > 0 && !coefficients) return fail("null coefficients");
  std::fill(&t->coef[0][0], &t->coef[0][0] + 5 * ASDR_TONE_MAX_SECTIONS, 0);
  if (sections > 0) std::copy(coefficients, coefficients + 5 * sections, &t->coef[0][0]);
  t->sections = sections;
  return 0;
}

int asdr_tone_get_highpass(const asdr_tone_t *t, int32_t *coefficients) {
  if (check_handle(t) != 0) return -1;
  if (coefficients) std::copy(&t->coef[0][0], &t->coef[0][0] + 5 * ASDR_TONE_MAX_SECTIONS, coefficients);
  return t->sections;
}

int asdr_tone_set_want(asdr_tone_t *t, int ch, int want) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (want < ASDR_TONE_PASS || want >= t->n_tones) return fail("want must be ASDR_TONE_PASS, ASDR_TONE_ANY or a tone of the table");
  t->set.apply(ch, [=](ToneSetting &s) { s.want = want; });
  return 0;
}

int asdr_tone_get_want(const asdr_tone_t *t, int ch, int *want) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (want) *want = t->set[ch].want;
  return 0;
}

int asdr_tone_set_min_power(asdr_tone_t *t, int ch, uint64_t min_power) {
  if (check_channel(t, ch, true) != 0) return -1;
  t->set.apply(ch, [=](ToneSetting &s) { s.min_power = min_power; });
  return 0;
}

int asdr_tone_get_min_power(const asdr_tone_t *t, int ch, uint64_t *min_power) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (min_power) *min_power = t->set[ch].min_power;
  return 0;
}

int asdr_tone_set_hang(asdr_tone_t *t, int ch, int hang_windows) {
  if (check_channel(t, ch, true) != 0) return -1;
  if (hang_windows < 0 || hang_windows > ASDR_TONE_MAX_HANG) return fail("hang_windows must be in 0..255");
  t->set.apply(ch, [=](ToneSetting &s) { s.hang_windows = (uint32_t)hang_windows; });
  return 0;
}

int asdr_tone_get_hang(const asdr_tone_t *t, int ch, int *hang_windows) {
  if (check_channel(t, ch, false) != 0) return -1;
  if (hang_windows) *hang_windows = (int)t->set[ch].hang_windows;
  return 0;
}

int asdr_tone_update_device(asdr_tone_t *t, const int16_t *dIn, long in_stride_blocks, int16_t *dOut, long out_stride_blocks, int n_blocks,
                            void *stream_) {
  if (check_handle(t) != 0) return -1;
  if (t->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (stage_check_block_rows({{dIn}, t->n, in_stride_blocks}, {{dOut}, t->n, out_stride_blocks}, n_blocks, "output span overlaps the input span") != 0)
    return -1;
  if (n_blocks == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*t, stream) != 0 || t->set.push(stream) != 0 || t->steps.push(stream) != 0) return -1;
  ToneArgs a;
  a.in = dIn; a.out = dOut;
  a.in_stride_blocks = in_stride_blocks; a.out_stride_blocks = out_stride_blocks;
  a.n_channels = t->n; a.n_blocks = n_blocks;
  a.n_tones = t->n_tones; a.window = t->window; a.dominance = t->dominance; a.sections = t->sections;
  std::copy(&t->coef[0][0], &t->coef[0][0] + 5 * ASDR_TONE_MAX_SECTIONS, &a.coef[0][0]);
  a.steps = t->steps.dev; a.table = t->d_table; a.set = t->set.dev; a.state = t->state.dev;
  if (asdr_launch_tone(&a, stream) != 0) return fail("tone kernel launch failed");
  if (stage_after_launch(*t, stream) != 0) return -1;
  t->blocks += n_blocks;
  return 0;
}

int asdr_tone_read_state(asdr_tone_t *t, asdr_tone_state_t *dst) {
  if (check_handle(t) != 0) return -1;
  return t->state.read(*t, dst);
}

int asdr_tone_write_state(asdr_tone_t *t, const int *channels, int n, const asdr_tone_state_t *src) {
  if (check_handle(t) != 0) return -1;
  const int window = t->window, n_tones = t->n_tones;
  auto check_record = [=](int k, const asdr_tone_state_t &s) {
    const std::string r = "record " + std::to_string(k);
    if (s.open > 1) return fail(r + ": open must be 0 or 1");
    if (s.window_block >= window) return fail(r + ": window_block must be below the window");
    if (s.detected < -1 || s.detected >= n_tones || s.last_best < -1 || s.last_best >= n_tones)
      return fail(r + ": detected and last_best must be -1 or a tone of the table");
    if (s.reserved[0] != 0 || s.reserved[1] != 0) return fail(r + ": reserved fields must be 0");
    for (int j = n_tones; j < ASDR_TONE_MAX_TONES; j++)
      if (s.acc[j][0] != 0 || s.acc[j][1] != 0) return fail(r + ": acc must be 0 from n_tones on");
    return 0;
  };
  return t->state.write(*t, channels, n, src, check_record);
}

int asdr_tone_clear(asdr_tone_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->state.rewrite(*t, [](asdr_tone_state_t &s) { s.windows = s.matches = s.openings = s.open_blocks = 0; }) != 0) return -1;
  t->blocks = 0;
  return 0;
}

int asdr_tone_reset(asdr_tone_t *t) {
  if (check_handle(t) != 0) return -1;
  if (t->state.fill(*t, creation_record()) != 0) return -1;
  t->blocks = 0;
  return 0;
}

long long asdr_tone_blocks(const asdr_tone_t *t) { return t ? t->blocks : -1; }

int asdr_tone_synchronize(asdr_tone_t *t) {
  if (check_handle(t) != 0) return -1;
  return stage_quiesce(*t);
}

}  // extern "C"
