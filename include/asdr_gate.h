/* asdr_gate.h -- C ABI of the audio gate: per-receiver audio meters, a squelch, and delivery of the open channels.
 *
 * An after-pass over the int16 audio rows that asdr_update_device_strided wrote (or that the capture sink holds).  It reads the
 * rows once on the device and hands back a short ascending list of the channels whose gate was open during the call and, when the
 * caller gives room for one, a compact packet of those channels' rows: a service behind a large bank moves only the receivers that
 * hear something over PCIe.  A gate is an object of its own (libasdr_hip.so, asdr_gate.hip); a deployment that creates none runs
 * exactly as without this header.  Same conventions as asdr.h: `ch` = channel index or ASDR_ALL (-1) for the setter,
 * ASDR_NO_DEVICE for a control-plane-only gate whose signal calls fail, 0 / -1 return codes with asdr_last_error().
 *
 * Statement (integers only; tests/gate_ref.py is the independent numpy restatement, and the kernels are held to it bit for bit).
 *
 *   Input: int16 rows [n_channels][stride_blocks][128] in HBM, of which blocks 0 .. n_blocks - 1 are new.
 *
 *   Per channel and block b:   E_b = sum of x[n]^2 over the 128 samples, exact in unsigned 64 bits (a row of -32768 gives 2^37),
 *                              P_b = max |x[n]|, in 0 .. 32768.
 *
 *   Per-channel settings:      open_energy, close_energy (uint64, close_energy <= open_energy), hang_blocks (0 .. 65535).
 *                              Creation values 0, 0, 0: that gate is open for every block, so it delivers everything.
 *
 *   Per-channel state:         asdr_gate_state_t, 32 bytes, every field little-endian:
 *                                offset  0  uint64 energy       sum of E_b since clear, mod 2^64
 *                                offset  8  uint64 last_energy  E of the newest block
 *                                offset 16  int32  peak         max of P_b since clear
 *                                offset 20  uint32 openings     closed -> open transitions since clear
 *                                offset 24  uint32 open_blocks  blocks with the gate open since clear
 *                                offset 28  uint16 hang_left
 *                                offset 30  uint8  open
 *                                offset 31  uint8  reserved     0
 *
 *   Per block, in block order:
 *       if   E >= open_energy:            if !open: openings++;   open = 1; hang_left = hang_blocks
 *       elif open and E >= close_energy:  hang_left = hang_blocks
 *       elif open and hang_left > 0:      hang_left--
 *       elif open:                        open = 0
 *       open_blocks += open;  energy += E;  last_energy = E;  peak = max(peak, P)
 *
 *   The gate stays open for the loud block plus hang_blocks blocks below close_energy.  Energies 0,10,0,0,0,0 with thresholds
 *   10 / 5 and hang 2 give open = 0,1,1,1,0,0; energies 9,10,9,4,4 with hang 0 give 0,1,1,0,0.
 *
 *   A channel is DELIVERED by a call when its gate was open after at least one of the call's blocks.  The call's result:
 *       count                   one int32 on the device: the number of delivered channels
 *       index[0 .. count - 1]   the delivered channels, ascending
 *       the packet              int16 [min(count, capacity_rows)][n_blocks][128]: row i is all n_blocks blocks of channel
 *                               index[i], bit for bit.  Whole calls are delivered, not single blocks; the attack block is inside
 *                               because its own energy decides, so no look-back is needed.
 *   Splitting a sequence of blocks into calls of any sizes leaves the state and every per-block decision unchanged.
 *
 *   asdr_gate_energy_from_dbfs(db) = floor(128 * 32767^2 * 10^(db / 10) + 0.5), clamped to [0, 2^37]: the block energy of a
 *   square wave of amplitude 32767 is 0 dBFS (137 430 564 992); a full-scale sine with a whole number of cycles per block sits
 *   at -3.01 dBFS.  NaN gives 0.
 *
 * Calls.  asdr_gate_update_device is asynchronous on `stream` with the stream-ordering contract of asdr_tuner_update_device: a
 * call on another stream than the previous one first waits (on the device) for the previous call's work.  There is no host round
 * trip inside: count stays on the device, and asdr_gate_count_device / asdr_gate_index_device give the addresses (int32, and
 * int32 [n_channels]; fixed for the gate's lifetime) for a consumer on the same stream.  dAudio and dRows must be 16-byte aligned
 * and must not overlap; n_blocks is 1 .. 65535 (0 does nothing and leaves count and index as they were) and
 * stride_blocks >= n_blocks.  dRows = NULL (or capacity_rows = 0) asks for no packet; rows past count are not written.
 *
 * asdr_gate_deliver is the synchronous host entry: it runs the pass on the gate's own stream (the rows at dAudio must be complete:
 * synchronize their producer first, or produce them on the NULL stream), reads count, and copies only index and the delivered
 * rows to the host.  It returns the rows copied, min(count, capacity_rows), and sets *n_open to the full count; host_index
 * (room for n_channels entries) receives all count entries either way.  host_rows may be NULL with capacity_rows = 0.  With
 * count == 0 nothing but the count crosses PCIe.
 *
 * State.  read_state / write_state / clear / reset wait for the gate's work first.  write_state checks every record on the host
 * before it writes one (open <= 1, reserved == 0, channels in range); a hang_left above the current hang_blocks is allowed.  It is
 * how a receiver that moves between batches (asdr.h, "State records") takes its gate along.  clear zeroes the meters (energy,
 * last_energy, peak, openings, open_blocks, and the count asdr_gate_blocks returns) and keeps open and hang_left; reset restores
 * the creation state and keeps the settings.  An ASDR_NO_DEVICE gate keeps its state records on the host: every state call
 * works on it, and update_device and deliver fail.
 */
#ifndef ASDR_GATE_H_
#define ASDR_GATE_H_

#include <stddef.h>
#include <stdint.h>

#include "asdr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASDR_GATE_MAX_HANG 65535
#define ASDR_GATE_MAX_ENERGY (1ULL << 37) /* of one block: 128 * 32768^2 */

typedef struct asdr_gate asdr_gate_t;

typedef struct {
  uint64_t energy;
  uint64_t last_energy;
  int32_t peak;
  uint32_t openings;
  uint32_t open_blocks;
  uint16_t hang_left;
  uint8_t open;
  uint8_t reserved;
} asdr_gate_state_t;

/* lifetime; NULL on failure (asdr_last_error).  n_channels in 1 .. 1048576 */
asdr_gate_t *asdr_gate_create(int n_channels, int device);
void asdr_gate_destroy(asdr_gate_t *g);
int asdr_gate_n_channels(const asdr_gate_t *g);

/* settings: take effect with the next call.  A refused call changes nothing */
int asdr_gate_set_squelch(asdr_gate_t *g, int ch, uint64_t open_energy, uint64_t close_energy, int hang_blocks);
int asdr_gate_get_squelch(const asdr_gate_t *g, int ch, uint64_t *open_energy, uint64_t *close_energy, int *hang_blocks);
uint64_t asdr_gate_energy_from_dbfs(double db);

/* the pass */
int asdr_gate_update_device(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int16_t *dRows /* NULL: no packet */,
                            int capacity_rows, void *stream);
const int32_t *asdr_gate_count_device(asdr_gate_t *g);
const int32_t *asdr_gate_index_device(asdr_gate_t *g);
int asdr_gate_deliver(asdr_gate_t *g, const int16_t *dAudio, long stride_blocks, int n_blocks, int32_t *host_index, int16_t *host_rows,
                      int capacity_rows, int *n_open);

/* state */
int asdr_gate_read_state(asdr_gate_t *g, asdr_gate_state_t *dst /* [n_channels] */);
int asdr_gate_write_state(asdr_gate_t *g, const int *channels /* NULL: 0 .. n - 1 */, int n, const asdr_gate_state_t *src /* [n] */);
int asdr_gate_clear(asdr_gate_t *g);
int asdr_gate_reset(asdr_gate_t *g);
long long asdr_gate_blocks(const asdr_gate_t *g); /* blocks seen since creation / clear / reset; -1 for a NULL gate */
int asdr_gate_synchronize(asdr_gate_t *g);

#ifdef __cplusplus
}
#endif
#endif /* ASDR_GATE_H_ */
