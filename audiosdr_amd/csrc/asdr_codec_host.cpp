// asdr_codec_host.cpp -- host side + C ABI (include/asdr_codec.h) of the audio codec.  The state records live on the device only
// (an ASDR_NO_DEVICE codec keeps them on the host instead); deliver's packet buffer grows on demand and is kept.  The decoder is
// plain host code: a listener's side of the packet rows, and what the tests decode the device's bytes with.
#include <algorithm>
#include <vector>

#include "asdr_codec_device.h"
#include "asdr_stage_host.h"

static_assert(sizeof(asdr_codec_state_t) == 4, "asdr_codec_state_t is a 4-byte record");

struct asdr_codec : StageDev {
  int kind = 0;
  StageRecords<asdr_codec_state_t> state;
  void *d_rows = nullptr;
  size_t rows_cap = 0;
};

namespace {
const char *kNoDevice = "control-plane-only codec (ASDR_NO_DEVICE): the signal path needs a HIP device";
const uint16_t kStep[ASDR_CODEC_STEPS] = {ASDR_CODEC_STEP_TABLE};

bool kind_ok(int kind) { return kind == ASDR_CODEC_ULAW || kind == ASDR_CODEC_ALAW || kind == ASDR_CODEC_ADPCM; }
long row_bytes(int kind, long n) { return kind == ASDR_CODEC_ADPCM ? ASDR_CODEC_ADPCM_HEADER_BYTES + (n + 1) / 2 : n; }
long round4(long b) { return (b + 3) & ~3L; }

// what encode_device and deliver check alike, before they ask for a device: an ASDR_NO_DEVICE codec refuses a bad argument as
// any other does.  Gives the rows of the launch
int check_input(const asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, const int32_t *dIndex,
                const int32_t *dCount, int capacity_rows, int *grid_rows) {
  if (!dRows) return fail("null device pointer");
  if (n_samples < 1 || n_samples > ASDR_CODEC_MAX_SAMPLES) return fail("n_samples must be in 1..8388480");
  if (row_stride_samples < n_samples) return fail("row stride shorter than n_samples");
  if (row_stride_samples > (1L << 40)) return fail("row stride too large");
  if (((uintptr_t)dRows & 1u) != 0) return fail("the input rows must be 2-byte aligned");
  if (dIndex && !dCount) return fail("an index needs a count");
  if (dIndex && capacity_rows < 0) return fail("capacity_rows is negative");
  *grid_rows = dIndex ? std::min(capacity_rows, c->n) : c->n;
  return 0;
}

// the bytes of the input that a launch may read
size_t input_bytes(const asdr_codec_t *c, long row_stride_samples, long n_samples, const int32_t *dIndex, int rows_compact, int grid_rows) {
  const int in_rows = (dIndex && rows_compact) ? grid_rows : c->n;
  return in_rows > 0 ? ((size_t)(in_rows - 1) * row_stride_samples + n_samples) * sizeof(int16_t) : 0;
}

int launch(asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, int rows_compact, uint8_t *dOut,
           long out_stride_bytes, const int32_t *dIndex, const int32_t *dCount, int capacity_rows, int grid_rows, hipStream_t stream) {
  CodecArgs a;
  a.rows = dRows; a.row_stride = row_stride_samples;
  a.out = dOut; a.out_stride = out_stride_bytes;
  a.index = dIndex; a.count = dCount;
  a.state = c->state.dev;
  a.n_channels = c->n; a.n_samples = (int32_t)n_samples; a.grid_rows = grid_rows; a.capacity_rows = dIndex ? capacity_rows : c->n;
  a.rows_compact = rows_compact ? 1 : 0; a.kind = c->kind;
  a.aligned = (((uintptr_t)dRows & 15u) == 0 && row_stride_samples % 8 == 0) ? 1 : 0;
  a.pieces = (int32_t)((n_samples + 7) / 8);
  if (c->kind != ASDR_CODEC_ADPCM && (unsigned long long)std::max(grid_rows, 0) * (unsigned long long)a.pieces >= (1ULL << 32))
    return fail("codec: the call is too large for one launch; split it");
  if (stage_before_launch(*c, stream) != 0) return -1;
  if ((c->kind == ASDR_CODEC_ADPCM ? asdr_launch_codec_adpcm(&a, stream) : asdr_launch_codec_g711(&a, stream)) != 0)
    return fail("codec kernel launch failed");
  return stage_after_launch(*c, stream);
}

int check_record(const asdr_codec_t *c, int k, const asdr_codec_state_t &s) {
  if (s.step_index > ASDR_CODEC_MAX_STEP_INDEX) return fail("record " + std::to_string(k) + ": step_index must be in 0..88");
  if (s.reserved != 0) return fail("record " + std::to_string(k) + ": reserved byte must be 0");
  if (c->kind != ASDR_CODEC_ADPCM && (s.predictor != 0 || s.step_index != 0))
    return fail("record " + std::to_string(k) + ": a G.711 codec's records are all zero");
  return 0;
}
}  // namespace

extern "C" {

asdr_codec_t *asdr_codec_create(int n_channels, int kind, int device) {
  if (stage_check_create(n_channels) != 0) return nullptr;
  if (!kind_ok(kind)) { fail("codec: kind must be ASDR_CODEC_ULAW (1), ASDR_CODEC_ALAW (2) or ASDR_CODEC_ADPCM (3)"); return nullptr; }
  asdr_codec *c = new asdr_codec;
  c->n = n_channels; c->kind = kind;
  if (device == ASDR_NO_DEVICE) {
    c->state.zero(*c);
    return c;
  }
  const size_t bytes = (size_t)n_channels * sizeof(asdr_codec_state_t);
  if (stage_open(*c, device, "codec") != 0) { asdr_codec_destroy(c); return nullptr; }
  if (hipMalloc(&c->state.dev, bytes) != hipSuccess || hipMemset(c->state.dev, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    fail("codec: device allocation failed");
    asdr_codec_destroy(c);
    return nullptr;
  }
  return c;
}

void asdr_codec_destroy(asdr_codec_t *c) {
  if (!c) return;
  stage_close(*c, {c->state.dev, c->d_rows});
  delete c;
}

int asdr_codec_n_channels(const asdr_codec_t *c) { return c ? c->n : fail("null codec"); }
int asdr_codec_kind(const asdr_codec_t *c) { return c ? c->kind : fail("null codec"); }

long asdr_codec_row_bytes(int kind, long n_samples) {
  if (!kind_ok(kind)) return fail("codec: kind must be ASDR_CODEC_ULAW (1), ASDR_CODEC_ALAW (2) or ASDR_CODEC_ADPCM (3)");
  if (n_samples < 1 || n_samples > ASDR_CODEC_MAX_SAMPLES) return fail("n_samples must be in 1..8388480");
  return row_bytes(kind, n_samples);
}

long asdr_codec_encode_device(asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, int rows_compact, uint8_t *dOut,
                              long out_stride_bytes, const int32_t *dIndex, const int32_t *dCount, int capacity_rows, void *stream_) {
  if (!c) return fail("null codec");
  int grid_rows = 0;
  if (check_input(c, dRows, row_stride_samples, n_samples, dIndex, dCount, capacity_rows, &grid_rows) != 0) return -1;
  if (!dOut) return fail("null device pointer");
  const long bytes = row_bytes(c->kind, n_samples), padded = round4(bytes);
  if (((uintptr_t)dOut & 3u) != 0) return fail("the output rows must be 4-byte aligned");
  if (out_stride_bytes % 4 != 0) return fail("out_stride_bytes must be a multiple of 4");
  if (out_stride_bytes < padded) return fail("out_stride_bytes shorter than the row's bytes rounded up to 4");
  if (out_stride_bytes > (1L << 40)) return fail("output row stride too large");
  if (c->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  if (grid_rows > 0) {
    const size_t out_bytes = (size_t)(grid_rows - 1) * out_stride_bytes + padded;
    if (overlap((uintptr_t)dRows, input_bytes(c, row_stride_samples, n_samples, dIndex, rows_compact, grid_rows), (uintptr_t)dOut, out_bytes))
      return fail("output span overlaps the input span");
  }
  if (launch(c, dRows, row_stride_samples, n_samples, rows_compact, dOut, out_stride_bytes, dIndex, dCount, capacity_rows, grid_rows,
             (hipStream_t)stream_) != 0)
    return -1;
  return bytes;
}

long asdr_codec_deliver(asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, int rows_compact, int32_t *host_index,
                        uint8_t *host_rows, const int32_t *dIndex, const int32_t *dCount, int capacity_rows, void *stream_) {
  if (!c) return fail("null codec");
  int grid_rows = 0;
  if (check_input(c, dRows, row_stride_samples, n_samples, dIndex, dCount, capacity_rows, &grid_rows) != 0) return -1;
  if (grid_rows > 0 && !host_rows) return fail("null host rows");
  if (c->device == ASDR_NO_DEVICE) return fail(kNoDevice);
  const long padded = round4(row_bytes(c->kind, n_samples));
  hipStream_t stream = (hipStream_t)stream_;
  HIPCHK(hipSetDevice(c->device));
  const size_t need = (size_t)grid_rows * padded;
  if (stage_reserve(*c, &c->d_rows, &c->rows_cap, need) != 0) return -1;
  if (grid_rows > 0) {
    if (overlap((uintptr_t)dRows, input_bytes(c, row_stride_samples, n_samples, dIndex, rows_compact, grid_rows), (uintptr_t)c->d_rows, need))
      return fail("internal: packet buffer overlaps the input span");
    if (launch(c, dRows, row_stride_samples, n_samples, rows_compact, (uint8_t *)c->d_rows, padded, dIndex, dCount, capacity_rows, grid_rows,
               stream) != 0)
      return -1;
  }
  int32_t count = c->n;
  if (dIndex) {
    HIPCHK(hipMemcpyAsync(&count, dCount, sizeof(count), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (count < 0) count = 0;
  }
  const int rows = std::min<int32_t>(count, grid_rows);
  if (rows > 0) {
    if (host_index) {
      if (dIndex) HIPCHK(hipMemcpyAsync(host_index, dIndex, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
      else for (int k = 0; k < rows; k++) host_index[k] = k;
    }
    HIPCHK(hipMemcpyAsync(host_rows, c->d_rows, (size_t)rows * padded, hipMemcpyDeviceToHost, stream));
  }
  HIPCHK(hipStreamSynchronize(stream));
  return count;
}

int asdr_codec_decode(int kind, const uint8_t *row, long n_samples, int16_t *out) {
  if (!kind_ok(kind)) return fail("codec: kind must be ASDR_CODEC_ULAW (1), ASDR_CODEC_ALAW (2) or ASDR_CODEC_ADPCM (3)");
  if (n_samples < 1 || n_samples > ASDR_CODEC_MAX_SAMPLES) return fail("n_samples must be in 1..8388480");
  if (!row || !out) return fail("null pointer");
  if (kind == ASDR_CODEC_ULAW) {
    for (long k = 0; k < n_samples; k++) {
      const int u = ~row[k] & 0xFF, e = (u >> 4) & 7, q = u & 15;
      const int t = (((q << 3) + 132) << e) - 132;
      out[k] = (int16_t)((u & 0x80) ? -t : t);
    }
    return 0;
  }
  if (kind == ASDR_CODEC_ALAW) {
    for (long k = 0; k < n_samples; k++) {
      const int a = row[k] ^ 0x55, e = (a >> 4) & 7, q = a & 15;
      const int t = e == 0 ? (q << 4) + 8 : ((q << 4) + 0x108) << (e - 1);
      out[k] = (int16_t)((a & 0x80) ? t : -t);
    }
    return 0;
  }
  int p = (int16_t)(row[0] | (row[1] << 8)), i = row[2];
  if (i > ASDR_CODEC_MAX_STEP_INDEX) return fail("codec: the row's step_index must be in 0..88");
  if (row[3] != 0) return fail("codec: the row's fourth header byte must be 0");
  for (long k = 0; k < n_samples; k++) {
    const int nib = (row[ASDR_CODEC_ADPCM_HEADER_BYTES + k / 2] >> (4 * (k & 1))) & 15, c = nib & 7, s = kStep[i];
    const int v = (s >> 3) + ((c & 4) ? s : 0) + ((c & 2) ? s >> 1 : 0) + ((c & 1) ? s >> 2 : 0);
    p = std::min(std::max((nib & 8) ? p - v : p + v, -32768), 32767);
    i = std::min(std::max(i + (c < 4 ? -1 : 2 * (c - 3)), 0), ASDR_CODEC_MAX_STEP_INDEX);
    out[k] = (int16_t)p;
  }
  return 0;
}

int asdr_codec_read_state(asdr_codec_t *c, asdr_codec_state_t *dst) {
  if (!c) return fail("null codec");
  return c->state.read(*c, dst);
}

int asdr_codec_write_state(asdr_codec_t *c, const int *channels, int n, const asdr_codec_state_t *src) {
  if (!c) return fail("null codec");
  return c->state.write(*c, channels, n, src, [c](int k, const asdr_codec_state_t &s) { return check_record(c, k, s); });
}

int asdr_codec_reset(asdr_codec_t *c) {
  if (!c) return fail("null codec");
  return c->state.zero(*c);
}

int asdr_codec_synchronize(asdr_codec_t *c) {
  if (!c) return fail("null codec");
  return stage_quiesce(*c);
}

}  // extern "C"
