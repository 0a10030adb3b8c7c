// asdr_fm_host.cpp -- host side + C ABI (include/asdr_fm.h) of the FM demodulator.  The settings live in a host mirror that is
// pushed before a launch when a setter touched it; the state records live on the device only (an ASDR_NO_DEVICE handle keeps them
// on the host instead).
#include <algorithm>
#include <cmath>
#include <vector>

#include "asdr_fm_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_fm_state_t) == 48, "asdr_fm_state_t is a 48-byte record");
static_assert(sizeof(FmSetting) == 32, "FmSetting is 32 bytes");

struct asdr_fm : StageDev {
  StageMirror<FmSetting> set;
  StageRecords<asdr_fm_state_t> state;
  long long blocks = 0;
};

namespace {
const char *kNoDevice = "control-plane-only FM demodulator (ASDR_NO_DEVICE): the signal path needs a HIP device";
const double kFs = 44100.0;

int check_channel(const asdr_fm_t *f, int ch, bool all_allowed) { return stage_check_channel(f, ch, all_allowed, "null FM demodulator"); }

// write_state's check of record k beyond its channel
int check_record(int k, const asdr_fm_state_t &s) {
  if (s.open > 1) return fail("record " + std::to_string(k) + ": open must be 0 or 1");
  if (s.reserved != 0 || s.reserved2 != 0) return fail("record " + std::to_string(k) + ": reserved fields must be 0");
  return 0;
}
}  // namespace

extern "C" {

uint32_t asdr_fm_gain_from_deviation(double hz) {
  const double g = hz > 0.0 ? std::floor(32767.0 * kFs / (2.0 * hz) + 0.5) : 0.0;   // NaN too
  if (!(g >= 1.0 && g <= (double)ASDR_FM_MAX_GAIN)) { fail("deviation gives a gain outside 1..2^24"); return 0; }
  return (uint32_t)g;
}

uint32_t asdr_fm_deemphasis_from_tau_us(double t) {
  const double a = t > 0.0 ? std::floor(32768.0 * (1.0 - std::exp(-1e6 / (kFs * t))) + 0.5) : 0.0;   // NaN too
  if (!(a >= 1.0 && a <= (double)ASDR_FM_MAX_DEEMPHASIS)) { fail("time constant gives a coefficient outside 1..32768"); return 0; }
  return (uint32_t)a;
}

asdr_fm_t *asdr_fm_create(int n_channels, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  asdr_fm *f = new asdr_fm;
  f->n = n_channels;
  f->set.host.assign(n_channels, FmSetting{ASDR_FM_MAX_NOISE, ASDR_FM_MAX_NOISE, asdr_fm_gain_from_deviation(5000.0), ASDR_FM_MAX_DEEMPHASIS, 0, 0});
  if (device == ASDR_NO_DEVICE) {
    f->state.zero(*f);
    return f;
  }
  const size_t n = n_channels;
  if (stage_open(*f, device, "fm") != 0) { asdr_fm_destroy(f); return nullptr; }
  if (hipMalloc(&f->set.dev, n * sizeof(FmSetting)) != hipSuccess || hipMalloc(&f->state.dev, n * sizeof(asdr_fm_state_t)) != hipSuccess ||
      hipMemset(f->state.dev, 0, n * sizeof(asdr_fm_state_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fail("fm: device allocation failed");
    asdr_fm_destroy(f);
    return nullptr;
  }
  return f;
}

void asdr_fm_destroy(asdr_fm_t *f) {
  if (!f) return;
  stage_close(*f, {f->set.dev, f->state.dev});
  delete f;
}

int asdr_fm_n_channels(const asdr_fm_t *f) { return f ? f->n : fail("null FM demodulator"); }

int asdr_fm_set_gain(asdr_fm_t *f, int ch, uint32_t gain) {
  if (check_channel(f, ch, true) != 0) return -1;
  if (gain < 1 || gain > ASDR_FM_MAX_GAIN) return fail("gain must be in 1..2^24");
  f->set.apply(ch, [=](FmSetting &s) { s.gain = gain; });
  return 0;
}

int asdr_fm_get_gain(const asdr_fm_t *f, int ch, uint32_t *gain) {
  if (check_channel(f, ch, false) != 0) return -1;
  if (gain) *gain = f->set[ch].gain;
  return 0;
}

int asdr_fm_set_deemphasis(asdr_fm_t *f, int ch, uint32_t a) {
  if (check_channel(f, ch, true) != 0) return -1;
  if (a < 1 || a > ASDR_FM_MAX_DEEMPHASIS) return fail("de-emphasis coefficient must be in 1..32768");
  f->set.apply(ch, [=](FmSetting &s) { s.deemphasis = a; });
  return 0;
}

int asdr_fm_get_deemphasis(const asdr_fm_t *f, int ch, uint32_t *a) {
  if (check_channel(f, ch, false) != 0) return -1;
  if (a) *a = f->set[ch].deemphasis;
  return 0;
}

int asdr_fm_set_dc_shift(asdr_fm_t *f, int ch, int hp_shift) {
  if (check_channel(f, ch, true) != 0) return -1;
  if (hp_shift < 0 || hp_shift > ASDR_FM_MAX_DC_SHIFT) return fail("hp_shift must be in 0..15");
  f->set.apply(ch, [=](FmSetting &s) { s.hp_shift = (uint32_t)hp_shift; });
  return 0;
}

int asdr_fm_get_dc_shift(const asdr_fm_t *f, int ch, int *hp_shift) {
  if (check_channel(f, ch, false) != 0) return -1;
  if (hp_shift) *hp_shift = (int)f->set[ch].hp_shift;
  return 0;
}

int asdr_fm_set_squelch(asdr_fm_t *f, int ch, uint64_t open_noise, uint64_t close_noise, int hang_blocks) {
  if (check_channel(f, ch, true) != 0) return -1;
  if (open_noise > close_noise) return fail("open_noise must not exceed close_noise");
  if (close_noise > ASDR_FM_MAX_NOISE) return fail("the noise thresholds must not exceed 2^41");
  if (hang_blocks < 0 || hang_blocks > ASDR_FM_MAX_HANG) return fail("hang_blocks must be in 0..65535");
  f->set.apply(ch, [=](FmSetting &s) { s.open_noise = open_noise; s.close_noise = close_noise; s.hang_blocks = (uint32_t)hang_blocks; });
  return 0;
}

int asdr_fm_get_squelch(const asdr_fm_t *f, int ch, uint64_t *open_noise, uint64_t *close_noise, int *hang_blocks) {
  if (check_channel(f, ch, false) != 0) return -1;
  if (open_noise) *open_noise = f->set[ch].open_noise;
  if (close_noise) *close_noise = f->set[ch].close_noise;
  if (hang_blocks) *hang_blocks = (int)f->set[ch].hang_blocks;
  return 0;
}

int asdr_fm_update_device(asdr_fm_t *f, const int16_t *dI, const int16_t *dQ, long in_stride_blocks, int16_t *dOut, long out_stride_blocks,
                          int n_blocks, void *stream_) {
  if (!f) return fail("null FM demodulator");
  if (f->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (stage_check_block_rows({{dI, dQ}, f->n, in_stride_blocks}, {{dOut}, f->n, out_stride_blocks}, n_blocks, "output span overlaps an input span") != 0)
    return -1;
  if (n_blocks == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  if (stage_before_launch(*f, stream) != 0 || f->set.push(stream) != 0) return -1;
  FmArgs a;
  a.i = dI; a.q = dQ; a.out = dOut;
  a.in_stride_blocks = in_stride_blocks; a.out_stride_blocks = out_stride_blocks;
  a.n_channels = f->n; a.n_blocks = n_blocks;
  a.set = f->set.dev; a.state = f->state.dev;
  if (asdr_launch_fm(&a, stream) != 0) return fail("FM kernel launch failed");
  if (stage_after_launch(*f, stream) != 0) return -1;
  f->blocks += n_blocks;
  return 0;
}

int asdr_fm_read_state(asdr_fm_t *f, asdr_fm_state_t *dst) {
  if (!f) return fail("null FM demodulator");
  return f->state.read(*f, dst);
}

int asdr_fm_write_state(asdr_fm_t *f, const int *channels, int n, const asdr_fm_state_t *src) {
  if (!f) return fail("null FM demodulator");
  return f->state.write(*f, channels, n, src, check_record);
}

int asdr_fm_clear(asdr_fm_t *f) {
  if (!f) return fail("null FM demodulator");
  if (f->state.rewrite(*f, [](asdr_fm_state_t &s) { s.openings = s.open_blocks = 0; }) != 0) return -1;
  f->blocks = 0;
  return 0;
}

int asdr_fm_reset(asdr_fm_t *f) {
  if (!f) return fail("null FM demodulator");
  if (f->state.zero(*f) != 0) return -1;
  f->blocks = 0;
  return 0;
}

long long asdr_fm_blocks(const asdr_fm_t *f) { return f ? f->blocks : -1; }

int asdr_fm_synchronize(asdr_fm_t *f) {
  if (!f) return fail("null FM demodulator");
  return stage_quiesce(*f);
}

}  // extern "C"
