/* asdr_codec.h -- C ABI of the audio codec: delivered int16 audio rows as G.711 (mu-law, A-law) or 4-bit IMA ADPCM packet rows.
 *
 * The last after-pass between "rows on the device" and "bytes a listener can take".  It reads int16 rows -- the chain's rows
 * (asdr_update_device_strided), a capture sink's rows, or a resampler's dOut (asdr_resample.h) -- and writes one packet row per
 * channel on the device, for every channel or for the channels a gate (asdr_gate.h) delivered, so that a service behind a large
 * bank moves 21 or 22 bytes per channel-block (12 kHz ADPCM) over PCIe instead of 256 (raw 44.1 kHz int16).  A codec is an object
 * of its own (libasdr_hip.so, asdr_codec.hip); it changes no chain, tuner, gate or resampler kernel, and a deployment that
 * creates none runs exactly as without this header.  Same conventions as asdr_gate.h and asdr_resample.h: ASDR_NO_DEVICE for a
 * control-plane-only codec whose signal calls fail, 0 / -1 return codes with asdr_last_error(), and a refused call changes nothing.
 *
 * Statement (integers only; tests/codec_ref.py is the independent numpy restatement, and the kernels are held to it bit for bit).
 * x is an int16 sample, >> the arithmetic shift.
 *
 *   mu-law (ASDR_CODEC_ULAW).
 *       encode:  m = x >> 2, neg = m < 0;  a = min(|m|, 8158) + 33;  e = floor(log2 a) - 5  (0 .. 7);
 *                code = (e << 4) | ((a >> (e + 1)) & 15);  byte = code ^ (neg ? 0x7F : 0xFF)
 *       decode:  u = ~b & 0xFF, e = (u >> 4) & 7, q = u & 15;  t = (((q << 3) + 132) << e) - 132;  y = (u & 0x80) ? -t : t
 *       0 -> 0xFF, -1 -> 0x7E, 32767 -> 0x80, -32768 -> 0x00.  0x7F (negative zero) is decoded as 0 and never produced: it would
 *       need |m| = 0 with m < 0.  |decode(encode(x)) - x| <= 644, the maximum at the clipped top of the range.
 *
 *   A-law (ASDR_CODEC_ALAW).
 *       encode:  m = x >> 3, neg = m < 0;  a = neg ? -m - 1 : m;  e = max(floor(log2 max(a, 1)) - 4, 0);
 *                q = e < 2 ? (a >> 1) & 15 : (a >> e) & 15;  byte = ((e << 4) | q) ^ (neg ? 0x55 : 0xD5)
 *       decode:  a = b ^ 0x55, e = (a >> 4) & 7, q = a & 15;  t = e == 0 ? (q << 4) + 8 : ((q << 4) + 0x108) << (e - 1);
 *                y = (a & 0x80) ? t : -t
 *       0 -> 0xD5.  |decode(encode(x)) - x| <= 512.
 *       Both pairs are ITU-T G.711 as Python's audioop computes it (lin2ulaw / lin2alaw on all 65,536 inputs, ulaw2lin / alaw2lin
 *       on all 256 bytes).
 *
 *   IMA ADPCM (ASDR_CODEC_ADPCM).  Per-channel state: a predictor p (int16) and a step index i in 0 .. 88; a fresh channel has
 *       both 0.  The step table T[89]:
 *           7 8 9 10 11 12 13 14 16 17 19 21 23 25 28 31 34 37 41 45 50 55 60 66 73 80 88 97 107 118 130 143 157 173 190 209 230
 *           253 279 307 337 371 408 449 494 544 598 658 724 796 876 963 1060 1166 1282 1411 1552 1707 1878 2066 2272 2499 2749 3024
 *           3327 3660 4026 4428 4871 5358 5894 6484 7132 7845 8630 9493 10442 11487 12635 13899 15289 16818 18500 20350 22385 24623
 *           27086 29794 32767
 *       encode one sample:
 *           s = T[i];  d = x - p;  sign = d < 0 ? 8 : 0;  d = |d|;  v = s >> 3;  c = 0
 *           if d >= s:         c |= 4, d -= s,      v += s
 *           if d >= (s >> 1):  c |= 2, d -= s >> 1, v += s >> 1
 *           if d >= (s >> 2):  c |= 1,              v += s >> 2
 *           p = sat16(sign ? p - v : p + v);  i = clamp(i + (c < 4 ? -1 : 2 (c - 3)), 0, 88);  nibble = c | sign
 *       decode one nibble (c = nibble & 7, sign = nibble & 8):
 *           v = (s >> 3) + (c & 4 ? s : 0) + (c & 2 ? s >> 1 : 0) + (c & 1 ? s >> 2 : 0);  p and i as in the encoder;  y = p
 *       so the decoder reproduces the encoder's predictor sequence sample for sample.  (audioop.lin2adpcm / adpcm2lin give the
 *       same nibbles and the same state; audioop packs the first sample of a byte into the HIGH nibble, this header the low one.)
 *
 *   Packet rows.  A mu-law or A-law row of n samples is n bytes.  An ADPCM row is a 4-byte header and ceil(n / 2) bytes:
 *           offset 0  int16 predictor (little-endian)   the channel's state BEFORE the row's first sample
 *           offset 2  uint8 step_index
 *           offset 3  uint8 0
 *           offset 4  sample 2k in the low nibble of byte k, sample 2k + 1 in the high nibble (IMA's order); for odd n the
 *                     unused last high nibble is 0
 *       so every row is decodable on its own and a listener can join at any packet.  asdr_codec_row_bytes(kind, n) is the row's
 *       size; the bytes from there up to the next multiple of 4 are written as 0 and nothing past that is written.
 *
 *   State and timing.  The record is asdr_codec_state_t, 4 bytes; it is all zero, and stays so, for the two G.711 kinds.
 *       A channel's state advances ONLY in calls that encode it: its stream is the concatenation of the rows delivered for it, and
 *       an undelivered channel's record does not change.  This is the opposite of the resampler's carry, which advances for every
 *       channel in every call: a receiver that was closed for a while resumes its ADPCM stream where its last packet ended (its
 *       next header says from where), it does not track audio nobody received.  Splitting a sample sequence into calls of any
 *       sizes leaves the nibble sequence and the final state unchanged.
 *
 * The pass.  asdr_codec_encode_device is asynchronous on `stream` with the stream-ordering contract of asdr_gate_update_device: a
 * call on another stream than the previous one first waits (on the device) for the previous call's work.  It returns the row's
 * byte count, asdr_codec_row_bytes(kind, n_samples), or -1.
 *     dRows     int16 [..][row_stride_samples], 2-byte aligned; samples 0 .. n_samples - 1 of a row are read, n_samples in
 *               1 .. 8388480 (65535 blocks), row_stride_samples >= n_samples.  The chain's and a capture sink's rows are
 *               n_samples = 128 n_blocks with row_stride_samples = 128 stride_blocks; a resampler's dOut is n_samples = its returned
 *               count with row_stride_samples = out_stride_samples, which may be odd.  A 16-byte aligned dRows with a stride that is
 *               a multiple of 8 samples is read in aligned 16-byte pieces (the piece that holds a row's last sample is loaded whole and
 *               what lies behind that sample is discarded); any other geometry is read sample by sample, slower and as exact.
 *     dOut      uint8 [..][out_stride_bytes], 4-byte aligned; out_stride_bytes is a multiple of 4 and at least the row's byte count
 *               rounded up to 4.  It may not overlap the input.
 *     dIndex == NULL:                   input row c and output row c are channel c, for all n_channels (capacity_rows is ignored).
 *     dIndex given, rows_compact = 0:   output row i is channel dIndex[i], read from input row dIndex[i] -- the chain's rows behind
 *                                       a gate (asdr_gate_index_device / asdr_gate_count_device).
 *     dIndex given, rows_compact = 1:   input row i is already channel dIndex[i] -- a resampler's dOut behind the same index.  As
 *                                       there, the buffer has room for min(capacity_rows, n_channels) rows (the host does not know
 *                                       the count: that is the span the overlap check takes), of which the first count are read.
 *     In both index forms i runs below min(*dCount, capacity_rows); rows past that are not written, and there is no host round
 *     trip.  Index entries must be distinct.  An entry outside 0 .. n_channels - 1 is skipped on the device: its row is not
 *     written and no state is touched.
 *
 * asdr_codec_deliver is the host entry of asdr_gate_deliver's kind (a resampler has none: this closes gate -> resampler -> codec ->
 * host).  It enqueues the same pass on `stream` into an internal buffer that grows on demand, reads the count once (4 bytes), copies
 * exactly min(count, capacity_rows) index entries (host_index may be NULL) and packet rows to the host, and returns count, having
 * synchronized `stream`.  The host row stride is the row's byte count rounded up to 4.  With dIndex == NULL capacity_rows is ignored
 * as above, count is n_channels, all rows are copied and host_index, when given, receives 0 .. n_channels - 1.
 *
 * asdr_codec_decode is plain host C: it needs no device and no codec.  It decodes one packet row of n_samples samples into out and
 * returns 0, or -1 for an unknown kind or an ADPCM header with step_index > 88 or a non-zero fourth byte.
 *
 * State.  read_state / write_state / reset wait for the codec's work first.  write_state is all or nothing: every record is checked
 * before one is written (channels in range, step_index <= 88, reserved == 0, and all zero for a G.711 codec).  It is how a receiver
 * that moves to another batch takes its ADPCM stream along.  reset gives zero records.  An ASDR_NO_DEVICE codec keeps its records
 * on the host: everything works on it except encode_device and deliver.
 */
#ifndef ASDR_CODEC_H_
#define ASDR_CODEC_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_CODEC_ULAW 1
#define ASDR_CODEC_ALAW 2
#define ASDR_CODEC_ADPCM 3
#define ASDR_CODEC_MAX_SAMPLES 8388480     /* per row and call: 65535 blocks of 128 */
#define ASDR_CODEC_MAX_STEP_INDEX 88
#define ASDR_CODEC_ADPCM_HEADER_BYTES 4

typedef struct asdr_codec asdr_codec_t;

typedef struct {
  int16_t predictor;
  uint8_t step_index;
  uint8_t reserved;
} asdr_codec_state_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576 */
asdr_codec_t *asdr_codec_create(int n_channels, int kind, int device);
void asdr_codec_destroy(asdr_codec_t *c);
int asdr_codec_n_channels(const asdr_codec_t *c);
int asdr_codec_kind(const asdr_codec_t *c);
long asdr_codec_row_bytes(int kind, long n_samples); /* pure; -1 for a wrong kind or n_samples outside 1 .. 8388480 */

/* the pass */
long asdr_codec_encode_device(asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, int rows_compact, uint8_t *dOut,
                              long out_stride_bytes, const int32_t *dIndex /* NULL: all channels */, const int32_t *dCount, int capacity_rows,
                              void *stream);
long asdr_codec_deliver(asdr_codec_t *c, const int16_t *dRows, long row_stride_samples, long n_samples, int rows_compact,
                        int32_t *host_index /* may be NULL */, uint8_t *host_rows, const int32_t *dIndex, const int32_t *dCount,
                        int capacity_rows, void *stream);

/* a packet row back to samples, on the host */
int asdr_codec_decode(int kind, const uint8_t *row, long n_samples, int16_t *out /* [n_samples] */);

/* state */
int asdr_codec_read_state(asdr_codec_t *c, asdr_codec_state_t *dst /* [n_channels] */);
int asdr_codec_write_state(asdr_codec_t *c, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_codec_state_t *src /* [n] */);
int asdr_codec_reset(asdr_codec_t *c);
int asdr_codec_synchronize(asdr_codec_t *c);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_CODEC_H_ */
