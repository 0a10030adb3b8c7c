// asdr_host.cpp -- host control plane + C ABI of libasdr_hip.so (see include/asdr.h).
//
// Mirrors the reference's `AudioSDR` class surface (SRC/AudioSDRlib/AudioSDR.h:88-156,
// AudioSDR.cpp:174-757) for a batch of N channels: every setter is a field write on a host-side
// per-channel record (plus the same derived-parameter arithmetic the reference performs, in the same
// float/double types), and marks the device parameter block dirty; update() uploads what changed and
// launches the HIP kernels of asdr_kernels.hip.  There is deliberately no CPU implementation of the
// signal path here: without a HIP device asdr_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/asdr.h"
#include "asdr_device.h"
#include "asdr_tables.h"

// batches of at least this many waves issue a multi-block call as one launch per block (asdr_update_device_strided)
#ifndef ASDR_SAM_CHUNK
#define ASDR_SAM_CHUNK 8         /* SAM role streams in chunks: blocks per launch ... */
#define ASDR_SAM_CHUNK_SETS 32   /* ... and tile sets (blocks in flight between the pre role and the post role: four chunks) */
#define ASDR_SAM_CHUNK_MAX_WAVES 512   /* ... for banks of up to this many waves (4,096 channels: 128 MB of tiles) */
#endif
#ifndef ASDR_ALS_ROLE_MAX_WAVES
#define ASDR_ALS_ROLE_MAX_WAVES 512   /* ALS role streams: banks of up to this many waves (4,096 channels: 64 MB of stage) */
#endif
#ifndef ASDR_PER_BLOCK_LAUNCH_WAVES
#define ASDR_PER_BLOCK_LAUNCH_WAVES 1024
#endif
// A multi-block call on a SMALL batch of SSB-class channels runs as a block pipeline of three role-specialised waves per channel
// group (asdr_stream_kernel): all 3 x waves workgroups must be resident at once, hence the cap; shorter calls are not worth the
// pipeline's fill and drain.
#ifndef ASDR_STREAM_MAX_WAVES
#define ASDR_STREAM_MAX_WAVES 1024   /* upper bound on what the occupancy query may allow (asdr_create) */
#endif
#ifndef ASDR_STREAM_MIN_BLOCKS
#define ASDR_STREAM_MIN_BLOCKS 8
#endif
#ifndef ASDR_STREAM_SIDE_MARGIN
#define ASDR_STREAM_SIDE_MARGIN 16   /* resident-workgroup slots kept free on top of the side sub-ranges' waves when a pipeline call carries any */
#endif
#ifndef ASDR_STREAM_SIDE_WAVES
#define ASDR_STREAM_SIDE_WAVES 64   /* waves of other kernel kinds / remainders a pipeline call may carry beside it (on the in-kernel block loop) */
#endif
extern "C" int asdr_launch_stream(const UpdateArgs *a, hipStream_t stream, int fir_helpers);
extern "C" int asdr_stream_capacity(int device, int *compute_units, int fir_helpers);
extern "C" int asdr_launch_stream_snapshot(const UpdateArgs *a, void *snap, int restore, hipStream_t stream);
extern "C" int asdr_launch_stream_ack(uint32_t *err, hipStream_t stream);
extern "C" int asdr_kernels_upload_tables(void);
namespace { void autopin_batch_created(); void autopin_batch_gone(); }   // (the auto-pinned caller ranges live as long as the process has a device batch: host path, below)
extern "C" int asdr_launch_update(const UpdateArgs *a, int variant, int uniform, hipStream_t stream);
extern "C" int asdr_launch_update_ordered(const UpdateArgs *a, int variant, int uniform, hipStream_t stream, int *reversed);
extern "C" int asdr_launch_sam_role(const UpdateArgs *a, int variant, int uniform, int role, hipStream_t stream);
extern "C" int asdr_launch_als_role(const UpdateArgs *a, int role, hipStream_t stream);
extern "C" int asdr_launch_als_stage_seed(const UpdateArgs *a, int ch0, int n, hipStream_t stream);
extern "C" int asdr_launch_reset(const UpdateArgs *a, const uint32_t *d_reset_bits, int first_row, int n_rows, hipStream_t stream);

namespace {

constexpr double kPI = 3.1415926535897932384626433832795;  // Arduino.h PI
constexpr float kFs = 44100.0f;                            // AUDIO_SAMPLE_RATE_EXACT (Teensy 4.x)
constexpr float kIFcenter = 6890.0f, kBWssb = 3000.0f, kBWcw = 1000.0f, kBWwspr = 1000.0f, kBWam = 8500.0f;  // .h:164-168

thread_local std::string g_err;
int fail(const std::string &m) { g_err = m; return -1; }
#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

// One reference instance's control-plane members (AudioSDR.h:172-246), batch-side naming.
struct Chan {
  float in_gain = 1.0f, in_gain_i = 1.0f, in_gain_q = 1.0f, gain_balance = 1.0f;
  float output_gain = 0.5f, out_gain = 1.0f, current_out_gain = 1.0f;
  float freq_shift = 0.0f;
  uint16_t mode = 0;
  bool muted = true;
  int16_t current_filter = 0;
  bool af_en = false;
  int if_table = ASDR_TBL_IF_SSB, audio_table = ASDR_TBL_AUDIO_BASE + ASDR_audio2700;
  int16_t als_m = 55, als_delay = 3;
  float als_lambda = 0.5f;
  bool als_en = false, als_notch = true, als_adaptive = true;
  float agc_alpha_att = 0, agc_beta_att = 0, agc_alpha_rel = 0, agc_beta_rel = 0;
  float agc_attack_ms = 0, agc_release_ms = 0, agc_knee = 0, agc_slope = 0, agc_threshold = 0;
  float agc_static_gain = 10.0f;
  float agc_slot129 = 100.0f;  // _agc_hangTime, which is also _agc_gainLookup[129] (.h:219-220)
  uint32_t agc_hang_count = 0;
  bool agc_en = true;
  int agc_table = -1;
  float nb_threshold = 1.2f;
  bool nb_en = true;
};

struct AgcTable {
  float thr, slope, knee;
  float v[ASDR_AGC_TAB_ROW];
};

// log2_approx_f32, AudioSDR.h:483-491
float log2_approx(float input) {
  int exponent;
  float mantissa = frexpf(fabsf(input), &exponent);
  return (((1.23149591368684f * mantissa - 4.11852516267426f) * mantissa + 6.02197014179219f) * mantissa -
          3.13396450166353f) + exponent;
}

// agc_createLookupTable, AudioSDR.cpp:459-480 (130 entries: the loop bound is tableSize + 1)
void build_agc_table(AgcTable &t) {
  const float thr = t.thr, slope = t.slope, knee = t.knee;
  const float lin_lo = expf((float)(2.3025 * ((double)thr - (double)knee / 2.0) / 20.0));
  const float lin_hi = expf((float)(2.3025 * ((double)thr + (double)knee / 2.0) / 20.0));
  for (int i = 0; i < 130; i++) {
    const float input = (float)((double)(float)i / 128.0);
    const float in_db = (float)(6.026 * (double)log2_approx(input));
    if (input < lin_lo) {
      t.v[i] = 1.0f;
    } else if (input > lin_hi) {
      const float out_db = thr + (in_db - thr) * slope;
      t.v[i] = expf((float)(2.3025 * (double)(out_db - in_db) / 20.0));
    } else {
      const double u = (double)(in_db - thr) + (double)knee / 2.0;
      const float out_db = (float)((double)in_db + (((double)slope - 1.0) * u * u) / (2.0 * (double)knee));
      t.v[i] = expf((float)(2.3025 * (double)(out_db - in_db) / 20.0));
    }
  }
  t.v[130] = t.v[131] = 0.0f;
}

float time_constant(float ms) {  // AudioSDR.cpp:448/553: exp(log(0.1) / (FS*ms/1000.0))
  return (float)exp(log(0.1) / ((double)(kFs * ms) / 1000.0));
}

}  // namespace

namespace {
class CopyPool {   // a handful of threads that copy between caller memory and the pinned staging area, all of them on ONE chunk at a time
 public:
  // A chunk is copied as `slices` slices, claimed one by one: every worker helps with the chunk the DMA waits for next (a whole chunk per
  // worker left the first H2D waiting for one thread's 4 MB: 0.5 ms of a 1 ms call).  Waiting is a short sleep, not a spin: the box
  // gives a process fewer threads than it shows, and spinning waiters take the cores the copying threads need.
  struct Job {
    int n_chunks = 0, slices = 1;
    std::function<void(int, int, int)> copy_in, copy_out;   // (chunk, slice, slices)
    std::vector<std::atomic<int>> in_done, out_ready;        // in_done[k] counts finished slices; out_ready[k]: the chunk's D2H is complete
    std::atomic<int> next_in{0}, next_out{0}, out_finished{0}, workers_left{0};
    Job(int k, int sl) : n_chunks(k), slices(sl), in_done(k), out_ready(k) { for (int i = 0; i < k; i++) { in_done[i].store(0); out_ready[i].store(0); } }
  };
  static void nap() { std::this_thread::sleep_for(std::chrono::microseconds(20)); }
  explicit CopyPool(int n) { for (int i = 0; i < n; i++) th_.emplace_back([this] { loop(); }); }
  ~CopyPool() { { std::lock_guard<std::mutex> g(m_); quit_ = true; } cv_.notify_all(); for (auto &t : th_) t.join(); }
  int threads() const { return (int)th_.size(); }
  void start(Job *j) { j->workers_left.store((int)th_.size()); { std::lock_guard<std::mutex> g(m_); job_ = j; gen_++; } cv_.notify_all(); }
  static void work(Job *j) {
    const int n_tasks = j->n_chunks * j->slices;
    for (int t; (t = j->next_in.fetch_add(1)) < n_tasks;) { const int k = t / j->slices; j->copy_in(k, t % j->slices, j->slices); j->in_done[k].fetch_add(1, std::memory_order_release); }
    for (int t; (t = j->next_out.fetch_add(1)) < n_tasks;) {
      const int k = t / j->slices;
      while (!j->out_ready[k].load(std::memory_order_acquire)) nap();
      j->copy_out(k, t % j->slices, j->slices); j->out_finished.fetch_add(1, std::memory_order_release);
    }
  }
 private:
  void loop() {
    unsigned long seen = 0;
    for (;;) {
      Job *j;
      { std::unique_lock<std::mutex> g(m_); cv_.wait(g, [&] { return quit_ || gen_ != seen; }); if (quit_) return; seen = gen_; j = job_; }
      work(j);
      j->workers_left.fetch_sub(1, std::memory_order_release);
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_; std::condition_variable cv_;
  Job *job_ = nullptr; unsigned long gen_ = 0; bool quit_ = false;
};

// chunk plan of a host call: K channel ranges [bound[j], bound[j + 1]); kernel part p needs input chunks 0..need_in[p]; output chunk
// j is complete after kernel part last_part[j]
struct HostPlan { int K = 1; std::vector<int> bound, need_in, last_part; long sched_gen = -1; int n_blocks = 0; };

}  // namespace

#define ASDR_LANES 8   /* most lanes a batch can run (asdr_batch::n_lanes of them are used) */
#define ASDR_AUX_STREAMS (ASDR_KERNEL_KINDS + 1 + 8)   /* every sub-range but the first runs on a helper stream; a large sub-range may be split over several (launch_split) */
struct asdr_batch {
  int n = 0, device = 0;
  hipStream_t stream = nullptr;  // used by the host-pointer entry point and by getters
  std::vector<Chan> ch;          // n + 1 (last = dummy channel used to pad the last wave)
  std::vector<AgcTable> agc_pool;
  std::unordered_map<uint64_t, std::vector<int>> agc_index;   // hash of (threshold, slope, knee) bits -> rows of agc_pool
  std::vector<uint32_t> agc_refs;                              // channels using each table
  std::vector<ChanParams> hp;
  std::vector<uint32_t> reset;
  std::vector<SlotInfo> sched;
  // Incremental control plane: a setter marks only the channels it touched.  flush() refills and uploads those rows; the
  // wave schedule is rebuilt only when a touched channel's schedule key (kernel kind, mode, enables, tables) changed.
  std::vector<int32_t> dirty;          // channels whose parameter row changed since the last flush (each listed once)
  std::vector<uint8_t> dirty_flag;
  bool all_dirty = true;               // first flush, or so many dirty rows that one bulk upload is cheaper
  bool sched_dirty = true, reset_pending = true, agc_pool_dirty = true;
  bool agc_refs_changed = true;        // a setter moved a channel to another gain table since the last compaction check
  int reset_lo = 0x7fffffff, reset_hi = -1;   // rows with pending reset bits lie in [reset_lo, reset_hi]
  // The sorted schedule is launched as up to three sub-ranges, one per kernel instantiation (plain / SAM / ALS), each padded
  // to whole waves with the dummy channel: one SAM or ALS channel no longer demotes the whole batch.
  // Inside a sub-range the whole waves of each key group come first ("uniform" waves: 8 real channels, one key -> the
  // instantiation with scalar mode/flag tests), then the groups' remainders packed together ("mixed").
  int kind_first[ASDR_KERNEL_KINDS] = {}, kind_slots[ASDR_KERNEL_KINDS] = {}, kind_uniform_slots[ASDR_KERNEL_KINDS] = {};
  int left_first = 0, left_slots = 0, left_kind = ASDR_KERNEL_PLAIN;   // the key groups' remainders of all kinds: one sub-range, one launch
  bool kind_direct[ASDR_KERNEL_KINDS] = {};   // the uniform part is ONE key group of consecutive channel ids (checked when the schedule is built)
  // params_uniform: the rows of hp of a kind's direct group (kind_direct) are equal in every field the kernels read -- such a group's
  // direct launches carry the row as launch constants (UpdateArgs.uni).  Kept incrementally: puni_differs[c] = channel c's row differs
  // from the row of its group's first channel, puni_diff[k] = how many of kind k's group do.  A per-channel setter costs ONE row
  // comparison at the next flush; a whole pass over a group's rows runs only after a bulk refill (broadcast setters), a schedule
  // rebuild or a change of the group's first row -- never at a flush or launch with no setter in front of it.
  bool kind_puni[ASDR_KERNEL_KINDS] = {}, puni_recheck[ASDR_KERNEL_KINDS] = {};
  long puni_diff[ASDR_KERNEL_KINDS] = {};
  std::vector<uint8_t> puni_differs;
  long stat_puni_rows_compared = 0;    // rows compared so far (asdr_params_uniform_groups)
  bool uniform_params = true;          // (ASDR_NO_UNIFORM_PARAMS: off, for measurements and tests)
  // counters for the control-plane tests (ASDR_NO_DEVICE): what the last flush did
  long stat_rows_refilled = 0, stat_sched_rebuilds = 0, stat_bulk_uploads = 0;
  int stat_lo_groups_without_entry = 0;   // settings groups that mix early but got none of the ASDR_LO_ENTRIES cache entries (the smallest ones)
  // device
  ChanParams *d_params = nullptr;
  ChanSmall *d_small = nullptr;
  int16_t *d_nb_hist = nullptr;
  uint8_t *d_nb_mask = nullptr;
  float *d_hil_q = nullptr, *d_hil_i = nullptr, *d_als_x = nullptr,
        *d_als_w = nullptr, *d_agc_tab = nullptr, *d_taps = nullptr;
  float *d_audio_prev = nullptr;   // _audioOut of the previous block, per channel (unknown mode values re-process it: AudioSDR.cpp:149-161)
  bool exact_unknown_mode = true;  // asdr_set_exact_unknown_mode
  size_t agc_tab_cap = 0;
  SlotInfo *d_sched = nullptr;
  uint32_t *d_reset = nullptr;
  int16_t *d_io[3] = {nullptr, nullptr, nullptr};
  // host-pointer path (asdr_update): pinned staging rows for pageable caller buffers, copy streams, per-chunk events, the chunk plan
  int16_t *h_io[3] = {nullptr, nullptr, nullptr};
  size_t h_io_cap = 0;
  hipStream_t h2d_stream = nullptr, d2h_stream = nullptr;
  std::vector<hipEvent_t> ev_host;
  HostPlan host_plan;
  std::unique_ptr<CopyPool> copy_pool;
  int host_chunks_forced = 0;            // asdr_set_host_chunks: 0 = chosen from the call's size
  // LANES: a batch whose schedule is ONE settings group of consecutive channels (C2, C5 ...) may run its two halves on two streams of
  // its own that never wait for each other -- half A of block k + 1 starts when half A of block k is done, while half B of block k
  // still drains its last waves (kernels of one stream run strictly one after the other, each with a tail in which the GPU runs
  // empty: 0.121 -> 0.111 ms per C2 step, tools/split_probe.py).  Inside a multi-block call (which joins at its end) always; from
  // call to call only for calls on ASDR_STREAM_BATCH, whose contract leaves the ordering against other streams to the caller.
  hipStream_t lane[ASDR_LANES + 1] = {};   // [ASDR_LANES] = the stream of the sub-ranges that are not cut (the remainders' few long-lived waves)
  hipEvent_t ev_lane[ASDR_LANES + 1] = {};
  int n_lanes = 2, n_lanes_sam = 3;      // lanes in use: 2 (C2: 0.1209 -> 0.1106 ms; 3 and 4 lanes: +0.5 %); schedules whose SAM channels run as
                                         // pre | PLL | post launches take 3 = one per pool stream (C3, host clock from idle to drained over 1,500
                                         // calls: 0.499 -> 0.4645 ms: a PLL kernel, which leaves issue slots free, beside pre / post kernels,
                                         // which do not; 2 lanes 0.493, 4 lanes -- two of them sharing a stream, which then carries half the
                                         // work -- 0.495, 6 lanes 0.4705)
  int sched_lanes = 2;                   // ... as the schedule was built for (the lanes' writer bits in SlotInfo.lo)
  bool lanes_pending = false;            // the lanes hold launches that nothing has been ordered behind yet
  bool sched_sam_heavy = false;          // the schedule's lane count is the SAM one (the three-launch SAM form is at least half of it)
  bool last_was_lanes = false;           // the previous call ran on the lanes (asdr_update_device on ASDR_STREAM_BATCH)
  int lanes_min_waves = 1024;            // smallest sub-range that is run as lanes
  bool lanes_enabled = true;
  bool lanes_forced = false;     // asdr_set_lanes(b, on > 0): the caller's word outranks the overlap probe
  long stat_lane_calls = 0;
  int launch_split = 1, launch_split_min_waves = 2048;   // asdr_set_launch_split: a sub-range of at least that many waves is launched as `launch_split` kernels on as many streams
  int stat_host_chunks = 0, stat_host_pinned = 0;   // what the last asdr_update did (asdr_host_path_info)
  // A SHARDED batch (asdr_create_sharded) owns no channels itself: shard g holds channels [shard_first[g], shard_first[g + 1]) on
  // its own device with its own state, schedule and streams; every entry point of the C ABI routes global channel indices to the
  // owner (ASDR_ALL fans out), asdr_update scatters / gathers host rows with one host thread per shard, and there is no collective.
  std::vector<asdr_batch *> shards;
  std::vector<int> shard_first;
  void *workers = nullptr;   // (ShardWorkers *) asdr_update on host rows: one persistent thread per shard >= 1 (the caller's thread takes shard 0), started at the first such call
  int16_t *d_capture = nullptr;  // capture sink [n][capture_cap][128]
  long capture_cap = 0, capture_pos = 0;
  size_t io_cap = 0;
  bool taps_on = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_valid = false;
  bool time_calls = false;       // asdr_set_launch_timing: an event pair around every call's launches (two more packets per call)
  hipEvent_t rev0 = nullptr, rev1 = nullptr;   // asdr_region_timing_begin / _end
  hipStream_t region_stream = nullptr;
  bool region_on_lanes = false;  // asdr_region_timing_begin(b, ASDR_STREAM_BATCH)
  long region_calls = -1;        // update calls since asdr_region_timing_begin (-1: no region open)
  std::vector<hipEvent_t> tev;   // optional per-launch event pairs (asdr_kernel_timing_begin)
  size_t tev_used = 0;
  hipStream_t last_stream = nullptr;
  hipEvent_t ev_last = nullptr;  // recorded after every launch: a call on another stream waits for it first
  hipStream_t aux[ASDR_AUX_STREAMS] = {};   // helper streams for concurrent sub-range launches
  hipEvent_t ev_fork = nullptr, ev_join[ASDR_AUX_STREAMS] = {};
  bool ev_last_valid = false;
  LoEntry *d_lo = nullptr;       // local-oscillator cache, 2 entries (asdr_device.h)
  // streaming pipeline (asdr_stream_kernel): exchange rings and progress counters, allocated at its first use
  float *d_xch_a = nullptr, *d_xch_b = nullptr;
  uint32_t *d_stream_prog = nullptr;
  LoEntry *d_lo_ring = nullptr;
  // Launch-form switches.  Their defaults come from the environment WHEN THE BATCH IS CREATED (ASDR_SAM_FUSED, ASDR_SAM_SPLIT_MIN,
  // ASDR_NO_STREAM_PIPELINE: comparison switches of the measurement tools); asdr_set_sam_launch_form / asdr_set_stream_pipeline change
  // them per batch afterwards.
  bool sam_fused = false;           // SAM channels through the fused 4-wave kernel instead of the pre | PLL | post launches
  int sam_split_min = 512;          // ... which are chosen from this many SAM channels on
  bool stream_pipeline = true;      // small multi-block calls may run as the block pipeline (asdr_stream_kernel)
  int stream_query_waves = 0;       // ... as the occupancy query of asdr_create answered (the debug hook cannot go beyond it)
  int stream_max_waves = 0;         // channel groups the pipeline may hold: 3 w + 1 workgroups must be co-resident, one per compute unit
  int stream_cap_workgroups = 0;    // the occupancy query's answer itself (resident workgroups of the pipeline kernel on this device)
  int stream_cap_h3 = 0, stream_cus = 0;   // ... of its three-helper form (256 threads per workgroup), and the device's compute units: that form is taken while every workgroup has one to itself
  int stream_h3 = -1;               // -1: by the rule above; 0 / 1: forced (ASDR_STREAM_H3, asdr_set_stream_fir_helpers: measurements, tests)
  long stat_stream_h3_calls = 0;
  uint32_t stream_spin_limit = ASDR_STREAM_SPIN_LIMIT;
  void *d_stream_snap = nullptr;    // snapshot of the state a pipeline call advances (asdr_kernels.hip "the pipeline as a transaction")
  long stat_stream_recoveries = 0;  // pipeline calls that gave up and were re-run on the in-kernel block loop (read back at synchronisation points)
  bool sam_split = false;           // decided when the schedule is built (enough SAM channels, not sam_fused)
  int als_split_min = 0x7fffffff;   // channels with a short ALS filter (not SAM) run as chain | filter launches from this many on (default: never --
                                    // measured against the final fused kernel: 2 % slower for C4's 131,072-channel share, 12 % slower at 1,048,576
                                    // channels, 9 % slower all-ALS; profiles/README.md "Round 3" is the one source of these numbers)
  bool als_split = false;           // decided when the schedule is built
  float *d_xch_sam = nullptr;       // SAM sub-range as pre | PLL | post launches: the IF rows of the current block (1 KB per slot)
  size_t xch_sam_slots = 0;         // ... TWO sets of tiles (and of lock words behind them): consecutive blocks of a multi-block call alternate
  hipEvent_t ev_role[6] = {};       // SAM role streams: [0..1] pre done, [2..3] PLL done, [4..5] post done, by block parity
  bool sam_role_streams = true;     // (ASDR_NO_SAM_ROLE_STREAMS: off, for measurements)
  bool sam_chunks = true;           // ... in chunks where the rule allows (ASDR_NO_SAM_CHUNKS: the per-block form, for measurements)
  long stat_sam_role_calls = 0;
  // ALS role streams: a SMALL bank of channels with a short ALS filter (one uniform sub-range, below the one-launch-per-block size) runs a
  // multi-block call as chain | filter launches on two event-chained streams, a chunk of blocks per launch -- the filter of a chunk (a
  // 33-epoch dependent chain per block: ~13 us whatever the bank size) beside the chain of the next one -- through a stage of post-AGC rows.
  // SAM role streams in CHUNKS (round 5): a uniform SAM sub-range's multi-block call as pre | PLL | post launches of ASDR_SAM_CHUNK blocks each
  // (the roles' block loops kept) -- one event pair per chunk and role instead of per block (every event between two kernels of a queue costs
  // ~10 us of command-processor time: the per-block form ran 50 us per block for a PLL chain of 32).  Tile sets of ASDR_SAM_CHUNK_SETS blocks.
  float *d_xch_sam_chunk = nullptr; size_t xch_sam_chunk_slots = 0;
  long stat_sam_chunk_calls = 0;
  hipEvent_t ev_samc[3 * (ASDR_SAM_CHUNK_SETS / ASDR_SAM_CHUNK)] = {};   // pre / PLL / post chunk k done, by k % R
  float *d_als_stage = nullptr;     // [n][ASDR_ALS_STAGE_SLOTS][128], allocated at the first such call
  hipEvent_t ev_als[3 * (ASDR_ALS_STAGE_SLOTS / ASDR_ALS_CHUNK)] = {};   // chain (back half) chunk k done [k % R], filter chunk k done [R + k % R], front half chunk k done [2 R + k % R]
  int als_role_stages = 3;          // 3: front half | back half | filter on three streams (ASDR_ALS_ROLE_STAGES=2: the whole chain | filter on two)
  bool als_role_streams = true;     // (ASDR_NO_ALS_ROLE_STREAMS: off, for measurements)
  long stat_als_role_calls = 0;
  bool plain_uniform_ssb = false;   // every uniform wave of the plain instantiation runs an SSB-class mode or AM: the modes the block pipeline has roles for (checked when the schedule is built)
  bool stream_launched = false;     // a streaming launch is (or was) in flight: its error flag has not been read yet
  long stat_stream_launches = 0;
  long stat_stream_headroom_refusals = 0;   // pipeline calls sent to the other launch forms because pipeline + side sub-ranges would not be co-resident (asdr_stream_pipeline_headroom_refusals)
  long stat_stream_alloc_failures = 0;   // the pipeline's buffers could not be allocated: the batch opted itself out (asdr_stream_pipeline_alloc_failures)
  uint32_t lo_parity = 0;
  // Alternating channel order (asdr_set_alternate_order): the one-block direct launches of the plain kind walk their sub-range forwards in one
  // launched block and backwards in the next, so that the state rows a launch wrote last are the first the next launch reads -- built for the
  // last-level cache to serve those reads; measured, it buys nothing (profiles/README.md).  The parity advances per launched block like
  // lo_parity, whether the order is on or off; a lane reverses within its own half.
  uint32_t wg_parity = 0;
  bool alternate_order = false;     // off by default: measured, no gain (profiles/README.md); ASDR_ALTERNATE_ORDER=1 / asdr_set_alternate_order
  long stat_reversed_launches = 0;  // launches that ran in the reversed order (asdr_reversed_launches)
  // receiver state records (asdr_export_state* / asdr_import_state*, the end of this file): pinned and device staging, allocated at first use;
  // st_ev is recorded behind the last asynchronous use of the pinned half
  uint8_t *st_h = nullptr, *st_d = nullptr;
  size_t st_h_cap = 0, st_d_cap = 0;
  hipEvent_t st_ev = nullptr;
  bool st_ev_pending = false;
  uint32_t nb_phase = 0;         // blocks processed so far, mod 3 (position of every channel's blanker ring)
  uint32_t als_phase = 0;        // blocks processed so far, mod 2 (position of every channel's ALS input ring)
  ChainConsts k{};
};

namespace {

int sharded_update(asdr_batch *b, const int16_t *I, const int16_t *Q, int16_t *out, int n_blocks);
void shard_workers_stop(asdr_batch *b);
inline bool is_sharded(const asdr_batch *b);

uint64_t agc_hash(float thr, float slope, float knee) {
  uint32_t a, b2, c;
  memcpy(&a, &thr, 4); memcpy(&b2, &slope, 4); memcpy(&c, &knee, 4);
  uint64_t h = 1469598103934665603ull;
  for (uint32_t w : {a, b2, c}) { h ^= w; h *= 1099511628211ull; }
  return h;
}

int find_agc_table(asdr_batch *b, float thr, float slope, float knee) {
  std::vector<int> &bucket = b->agc_index[agc_hash(thr, slope, knee)];
  for (int i : bucket) {
    const AgcTable &t = b->agc_pool[i];
    if (memcmp(&t.thr, &thr, 4) == 0 && memcmp(&t.slope, &slope, 4) == 0 && memcmp(&t.knee, &knee, 4) == 0) return i;
  }
  AgcTable t;
  t.thr = thr; t.slope = slope; t.knee = knee;
  build_agc_table(t);
  b->agc_pool.push_back(t);
  b->agc_refs.push_back(0);
  bucket.push_back((int)b->agc_pool.size() - 1);
  b->agc_pool_dirty = true;
  return (int)b->agc_pool.size() - 1;
}

void rebuild_agc(asdr_batch *b, Chan &c) {  // agc_createLookupTable(): also clobbers _agc_hangTime's storage
  const int old = c.agc_table;
  c.agc_table = find_agc_table(b, c.agc_threshold, c.agc_slope, c.agc_knee);
  b->agc_refs[c.agc_table]++;
  b->agc_refs_changed = true;
  if (old >= 0 && old < (int)b->agc_refs.size() && b->agc_refs[old] > 0) b->agc_refs[old]--;
  c.agc_slot129 = b->agc_pool[c.agc_table].v[129];
}

// Drop tables no channel uses any more (a UI knob sweep leaves one dead table per step) once they outnumber the live ones.
void compact_agc_pool(asdr_batch *b) {
  if (!b->agc_refs_changed) return;   // (every update call comes through here: no scan of the pool unless a reference moved)
  b->agc_refs_changed = false;
  size_t live = 0;
  for (uint32_t r : b->agc_refs) live += (r != 0);
  if (b->agc_pool.size() < 64 || b->agc_pool.size() <= 2 * live) return;
  std::vector<int> remap(b->agc_pool.size(), -1);
  std::vector<AgcTable> pool;
  std::vector<uint32_t> refs;
  for (size_t i = 0; i < b->agc_pool.size(); i++)
    if (b->agc_refs[i]) { remap[i] = (int)pool.size(); pool.push_back(b->agc_pool[i]); refs.push_back(b->agc_refs[i]); }
  b->agc_pool.swap(pool); b->agc_refs.swap(refs);
  b->agc_index.clear();
  for (size_t i = 0; i < b->agc_pool.size(); i++) b->agc_index[agc_hash(b->agc_pool[i].thr, b->agc_pool[i].slope, b->agc_pool[i].knee)].push_back((int)i);
  for (Chan &c : b->ch) c.agc_table = remap[c.agc_table];
  b->agc_pool_dirty = true; b->all_dirty = true; b->sched_dirty = true;   // every row carries a table index
}

void mark_reset(asdr_batch *b, int i, uint32_t bits) {
  b->reset[i] |= bits;
  b->reset_pending = true;
  if (i < b->reset_lo) b->reset_lo = i;
  if (i > b->reset_hi) b->reset_hi = i;
}

// setDemodMode, AudioSDR.cpp:187-222
float set_mode(asdr_batch *b, int idx, int new_mode) {
  Chan &c = b->ch[idx];
  c.mode = (uint16_t)new_mode;
  int tbl = -1;
  if (c.mode == ASDR_USBmode) { c.freq_shift = (float)((double)kIFcenter - (double)kBWssb / 2.0); tbl = ASDR_TBL_IF_SSB; }
  else if (c.mode == ASDR_LSBmode) { c.freq_shift = (float)((double)kIFcenter + (double)kBWssb / 2.0); tbl = ASDR_TBL_IF_SSB; }
  else if (c.mode == ASDR_WSPRmode) { c.freq_shift = (float)((double)kIFcenter - (double)kBWssb / 2.0); tbl = ASDR_TBL_IF_WSPR; }
  else if (c.mode == ASDR_CW_USBmode) { c.freq_shift = (float)((double)kIFcenter - (double)kBWcw / 2.0); tbl = ASDR_TBL_IF_CW; }
  else if (c.mode == ASDR_CW_LSBmode) { c.freq_shift = (float)((double)kIFcenter + (double)kBWcw / 2.0); tbl = ASDR_TBL_IF_CW; }
  else if (c.mode == ASDR_AMmode || c.mode == ASDR_SAMmode) { c.freq_shift = kIFcenter; tbl = ASDR_TBL_IF_AM; }
  if (tbl >= 0) { c.if_table = tbl; mark_reset(b, idx, ASDR_R_IF); }
  return c.freq_shift;
}

// agc_init, AudioSDR.cpp:439-457
void agc_init(asdr_batch *b, Chan &c) {
  c.agc_threshold = -60.0f; c.agc_slope = 0.1f; c.agc_knee = 2.0f;
  c.agc_attack_ms = 5.0f; c.agc_release_ms = 500.0f;
  c.agc_slot129 = 100.0f;
  c.agc_hang_count = (uint32_t)((double)kFs * ((double)c.agc_slot129 / 1000.0));
  c.agc_alpha_att = time_constant(c.agc_attack_ms);
  c.agc_beta_att = (float)(1.0 - (double)c.agc_alpha_att);
  c.agc_alpha_rel = time_constant(c.agc_release_ms);
  c.agc_beta_rel = (float)(1.0 - (double)c.agc_alpha_rel);
  c.agc_en = true;
  rebuild_agc(b, c);
}

// init(), AudioSDR.cpp:174-185
void chan_init(asdr_batch *b, int idx) {
  Chan &c = b->ch[idx];
  c.audio_table = ASDR_TBL_AUDIO_BASE + ASDR_audio2700;
  c.if_table = ASDR_TBL_IF_SSB;
  mark_reset(b, idx, ASDR_R_AF | ASDR_R_IF | ASDR_R_IMG | ASDR_R_NB);
  agc_init(b, c);
  set_mode(b, idx, ASDR_LSBmode);
  c.muted = false;
}

void fill_params(const Chan &c, ChanParams &p) {
  memset(&p, 0, sizeof p);
  p.mode = c.mode;
  p.flags = (c.nb_en ? ASDR_F_NB_EN : 0u) | (c.af_en ? ASDR_F_AF_EN : 0u) | (c.agc_en ? ASDR_F_AGC_EN : 0u) |
            (c.als_en ? ASDR_F_ALS_EN : 0u) | (c.als_notch ? ASDR_F_ALS_NOTCH : 0u) |
            (c.als_adaptive ? ASDR_F_ALS_ADAPTIVE : 0u) | (c.muted ? ASDR_F_MUTED : 0u);
  p.if_table = c.if_table; p.audio_table = c.audio_table; p.agc_table = c.agc_table;
  p.in_gain_i = c.in_gain_i; p.in_gain_q = c.in_gain_q; p.output_gain = c.output_gain;
  p.freq_shift = c.freq_shift; p.nb_threshold = c.nb_threshold;
  p.agc_alpha_att = c.agc_alpha_att; p.agc_beta_att = c.agc_beta_att;
  p.agc_alpha_rel = c.agc_alpha_rel; p.agc_beta_rel = c.agc_beta_rel;
  p.agc_static_gain = c.agc_static_gain; p.agc_hang_count = c.agc_hang_count;
  p.als_m = c.als_m; p.als_delay = c.als_delay; p.als_lambda = c.als_lambda;
}

// Wave scheduling: channels are grouped by kernel instantiation (plain / SAM / ALS) and, inside it, by (mode, enables, tables),
// so that a wave's 8 channels take the same branches.  Rows of I/Q/out and of every state array are per channel, so the
// grouping costs nothing in coalescing.
int g_force_split = -1;   // EXPERIMENT (ASDR_FORCE_SPLIT=1): every channel without the ALS filter through the pre | (PLL) | post launches
int kernel_kind(const ChanParams &p) {
  if (g_force_split < 0) g_force_split = getenv("ASDR_FORCE_SPLIT") ? 1 : 0;
  if (g_force_split && !(p.flags & ASDR_F_ALS_EN)) return ASDR_KERNEL_SAM;
  if (p.flags & ASDR_F_ALS_EN) {
    // a short filter on a channel that needs no PLL fits the plain instantiation's LDS rows (12 instead of 9 waves per CU)
    const bool small = p.als_m >= 0 && p.als_m <= 64 && p.als_delay >= 0 && p.als_delay + p.als_m <= 65;
    return !small ? ASDR_KERNEL_ALS : (p.mode == ASDR_SAMmode ? ASDR_KERNEL_SAM_ALS : ASDR_KERNEL_ALS_SMALL);
  }
  return (p.mode == ASDR_SAMmode) ? ASDR_KERNEL_SAM : ASDR_KERNEL_PLAIN;
}
#ifndef ASDR_SAM_SPLIT_MIN_CHANNELS
#define ASDR_SAM_SPLIT_MIN_CHANNELS 512
#endif
uint64_t sched_key(const ChanParams &p) {
  return ((uint64_t)kernel_kind(p) << 60) | ((uint64_t)(p.mode & 0xFFFF) << 40) | ((uint64_t)(p.flags & 0xFF) << 32) |
         ((uint64_t)(p.if_table & 0xFF) << 24) | ((uint64_t)(p.audio_table & 0xFF) << 16) | (uint64_t)(p.agc_table & 0xFFFF);
}

void mark_dirty(asdr_batch *b, int i) {
  if (b->all_dirty) return;
  if (!b->dirty_flag[i]) { b->dirty_flag[i] = 1; b->dirty.push_back(i); }
  if (b->dirty.size() > (size_t)b->n / 8 + 64) { b->all_dirty = true; }   // a bulk refill is cheaper from here on
}

// params_uniform (asdr_batch::kind_puni).  The comparison covers every field a kernel reads: `reset` is consumed by the reset kernel in
// front of the launch, the padding is never read.
inline bool params_rows_equal(const ChanParams &x, const ChanParams &y) {
  return memcmp(&x, &y, offsetof(ChanParams, reset)) == 0 &&
         memcmp(&x.if_table, &y.if_table, offsetof(ChanParams, pad_) - offsetof(ChanParams, if_table)) == 0;
}
// one pass over the rows of kind k's direct group
void puni_pass(asdr_batch *b, int k) {
  b->puni_recheck[k] = false; b->puni_diff[k] = 0; b->kind_puni[k] = false;
  if (!b->kind_direct[k]) return;
  const int ch0 = b->sched[b->kind_first[k]].ch, nu = b->kind_uniform_slots[k];
  const ChanParams &r = b->hp[ch0];
  long diff = 0;
  for (int c = ch0; c < ch0 + nu; c++) { const uint8_t d = params_rows_equal(b->hp[c], r) ? 0 : 1; b->puni_differs[c] = d; diff += d; }
  b->stat_puni_rows_compared += nu;
  b->puni_diff[k] = diff; b->kind_puni[k] = (diff == 0);
}
// channel c's row was refilled: one comparison against its group's first row (that row itself: the group is passed over again)
void puni_row_changed(asdr_batch *b, int c) {
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
    if (!b->kind_direct[k] || b->puni_recheck[k]) continue;
    const int ch0 = b->sched[b->kind_first[k]].ch;
    if (c < ch0 || c >= ch0 + b->kind_uniform_slots[k]) continue;
    if (c == ch0) { b->puni_recheck[k] = true; return; }
    const uint8_t d = params_rows_equal(b->hp[c], b->hp[ch0]) ? 0 : 1;
    b->stat_puni_rows_compared++;
    b->puni_diff[k] += (long)d - (long)b->puni_differs[c]; b->puni_differs[c] = d;
    b->kind_puni[k] = (b->puni_diff[k] == 0);
    return;
  }
}

// Host half of flush(): refill the parameter rows that changed, decide whether the schedule has to be rebuilt, rebuild it.
// Returns the sorted list of refilled rows in `rows_out` (empty + all_dirty = every row).  No HIP call in here, so the
// control-plane tests can time it on a device-less batch.
void flush_host(asdr_batch *b, std::vector<int32_t> &rows_out, bool &bulk, bool &sched_rebuilt) {
  const int rows = b->n + 1;
  compact_agc_pool(b);
  bulk = b->all_dirty;
  rows_out.clear();
  b->stat_rows_refilled = 0;
  if (bulk) {
    for (int i = 0; i < rows; i++) {
      const uint64_t old_key = sched_key(b->hp[i]);
      fill_params(b->ch[i], b->hp[i]);
      if (i < b->n && sched_key(b->hp[i]) != old_key) b->sched_dirty = true;
    }
    b->stat_rows_refilled = rows;
    b->stat_bulk_uploads++;
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) b->puni_recheck[k] = true;
  } else if (!b->dirty.empty()) {
    std::sort(b->dirty.begin(), b->dirty.end());
    for (int32_t i : b->dirty) {
      const uint64_t old_key = sched_key(b->hp[i]);
      fill_params(b->ch[i], b->hp[i]);
      if (sched_key(b->hp[i]) != old_key) b->sched_dirty = true;
      b->dirty_flag[i] = 0;
    }
    if (!b->sched_dirty) for (int32_t i : b->dirty) if (i < b->n) puni_row_changed(b, i);   // (a rebuilt schedule: every group is passed over below)
    rows_out = b->dirty;
    b->stat_rows_refilled = (long)rows_out.size();
  }
  b->dirty.clear();
  if (bulk) std::fill(b->dirty_flag.begin(), b->dirty_flag.end(), 0);
  b->all_dirty = false;
  sched_rebuilt = false;
  if (b->sched_dirty) {
    std::vector<std::pair<uint64_t, int32_t>> order(b->n);
    for (int i = 0; i < b->n; i++) order[i] = {sched_key(b->hp[i]), i};
    std::sort(order.begin(), order.end());   // (key, channel): equal keys stay in channel order
    // per kernel kind: slots of the whole waves of every key group, and of the groups' remainders
    int uni[ASDR_KERNEL_KINDS] = {}, rem[ASDR_KERNEL_KINDS] = {};
    // SAM (no ALS) as three launches per block only when there are enough SAM channels to fill the PLL kernel's waves: a handful
    // of them is quicker through the fused kernel (one launch, no exchange round trips)
    int n_sam = 0;
    for (int i = 0; i < b->n; i++) { const int k = (int)(order[i].first >> 60); n_sam += (k == ASDR_KERNEL_SAM || k == ASDR_KERNEL_SAM_ALS); }
    b->sam_split = !b->sam_fused && n_sam >= b->sam_split_min;
    {   // short ALS filters on channels that are not SAM: the chain up to the AGC as the plain instantiation, then the filter as a
        // launch of its own (asdr_als_kernel: small LDS rows, 18 waves per CU) -- when there are enough of them to fill it
      int n_als_small = 0;
      for (int i = 0; i < b->n; i++) n_als_small += ((int)(order[i].first >> 60) == ASDR_KERNEL_ALS_SMALL);
      b->als_split = n_als_small >= b->als_split_min;
    }
    const bool sam_general_only = !b->sam_split;
    // The remainders (< 8 channels) of all key groups share ONE sub-range behind the kinds' whole waves, run by one launch of a
    // general instantiation: as a launch per kind they were up to five more streams of a handful of long-lived waves each, and
    // streams that share a hardware queue run one after the other (profiles/README.md: C4's last 80 us were four such waves).
    int left = 0; bool left_general = false;
    for (int i = 0; i < b->n;) {
      int j = i + 1;
      while (j < b->n && order[j].first == order[i].first) j++;
      const int k = (int)(order[i].first >> 60), g = j - i;
      if (k == ASDR_KERNEL_SAM && sam_general_only) rem[k] += g;   // the fused SAM instantiation has only the general form (4-wave workgroups)
      else { uni[k] += g / 8 * 8; left += g % 8; if (g % 8) left_general = left_general || (k != ASDR_KERNEL_PLAIN); }
      i = j;
    }
    int pos = 0;
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
      b->kind_first[k] = pos; b->kind_uniform_slots[k] = uni[k]; b->kind_slots[k] = uni[k] + ((rem[k] + 7) / 8) * 8;
      pos += b->kind_slots[k];
    }
    b->left_first = pos; b->left_slots = (left + 7) / 8 * 8; b->left_kind = left_general ? ASDR_KERNEL_ALS : ASDR_KERNEL_PLAIN;
    pos += b->left_slots;
    b->sched.assign(pos, SlotInfo{b->n, b->hp[b->n].mode, b->hp[b->n].flags, 0u});   // padding = the dummy channel
    int at_u[ASDR_KERNEL_KINDS], at_m[ASDR_KERNEL_KINDS], at_left = b->left_first;
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) { at_u[k] = b->kind_first[k]; at_m[k] = b->kind_first[k] + uni[k]; }
    // Local-oscillator cache: the settings groups with whole waves get an entry each, THE LARGEST GROUPS FIRST when there are more
    // groups than entries (the mixer's pairs are a function of (phase, increment); receivers of one group that were configured
    // together share them for ever).  A group without an entry computes its own pairs: time only, never results.
    std::unordered_map<uint64_t, uint32_t> lo_of_key;
    {
      std::vector<std::pair<int, uint64_t>> cand;   // (-whole slots, key)
      for (int i = 0; i < b->n;) {
        int j = i + 1;
        while (j < b->n && order[j].first == order[i].first) j++;
        const int k = (int)(order[i].first >> 60), g = j - i;
        const int whole = (k == ASDR_KERNEL_SAM && sam_general_only) ? 0 : g / 8 * 8;
        const uint32_t gm = b->hp[order[i].second].mode;
        const bool mixes_early = (gm == ASDR_USBmode || gm == ASDR_LSBmode || gm == ASDR_CW_USBmode || gm == ASDR_CW_LSBmode || gm == ASDR_WSPRmode || gm == ASDR_AMmode);
        if (whole > 0 && mixes_early) cand.push_back({-whole, order[i].first});
        i = j;
      }
      std::stable_sort(cand.begin(), cand.end(), [](const std::pair<int, uint64_t> &x, const std::pair<int, uint64_t> &y) { return x.first < y.first; });
      for (size_t e = 0; e < cand.size() && e < ASDR_LO_ENTRIES; e++) lo_of_key[cand[e].second] = (uint32_t)e + 1u;   // 1 + entry
      b->stat_lo_groups_without_entry = cand.size() > ASDR_LO_ENTRIES ? (int)(cand.size() - ASDR_LO_ENTRIES) : 0;
    }
    for (int i = 0; i < b->n;) {
      int j = i + 1;
      while (j < b->n && order[j].first == order[i].first) j++;
      const int k = (int)(order[i].first >> 60), g = j - i;
      const bool fused = (k == ASDR_KERNEL_SAM && sam_general_only);
      const int whole = fused ? 0 : g / 8 * 8;
      const auto lo_it = lo_of_key.find(order[i].first);
      const uint32_t lo_id = (whole > 0 && lo_it != lo_of_key.end()) ? lo_it->second : 0u;   // 1 + entry, 0 = none
      for (int t = 0; t < g; t++) {
        const int c = order[i + t].second;
        int &at = (t < whole) ? at_u[k] : (fused ? at_m[k] : at_left);
        const uint32_t lo = (t < whole) ? (lo_id | ((t < 8 && lo_id) ? ASDR_LO_WRITER : 0u)) : 0u;
        b->sched[at++] = SlotInfo{c, b->hp[c].mode, b->hp[c].flags, lo};
      }
      i = j;
    }
    // The lanes' writers: in every uniform sub-range, for lane l >= 1, the first wave of each settings group at or behind the start of
    // lane l's piece (the launcher's split: waves [w l / n, w (l + 1) / n) of the sub-range) and inside it.
    {   // 3 lanes (one per pool stream) when the pre | PLL | post launches are at least half of the work (C3: 0.5165 -> 0.481 ms), 2 otherwise (C4, a seventh SAM: 0.331 / 0.386)
      const int sam_slots_ = b->kind_slots[ASDR_KERNEL_SAM] + b->kind_slots[ASDR_KERNEL_SAM_ALS];
      b->sched_sam_heavy = b->sam_split && 2 * sam_slots_ >= pos;
      b->sched_lanes = b->sched_sam_heavy ? b->n_lanes_sam : b->n_lanes;
    }
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
      const long w = b->kind_uniform_slots[k] / 8;
      for (int l = 1; l < b->sched_lanes; l++) {
        const int lo = b->kind_first[k] + (int)(w * l / b->sched_lanes) * 8, hi = b->kind_first[k] + (int)(w * (l + 1) / b->sched_lanes) * 8;
        uint32_t seen = 0;   // entries (ids 1..8) that already have their writer in this lane
        for (int sl = lo; sl < hi; sl += 8) {
          const uint32_t id = b->sched[sl].lo & 0xFFu;
          if (id == 0u || (seen >> id) & 1u) continue;
          seen |= 1u << id;   // (a group's waves are consecutive: the first one met is the group's first wave in this lane)
          for (int t = 0; t < 8; t++) b->sched[sl + t].lo |= ASDR_LO_WRITER_LANE(l);
        }
      }
    }
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
      const SlotInfo *sl = b->sched.data() + b->kind_first[k];
      bool direct = b->kind_uniform_slots[k] > 0;
      for (int j = 1; j < b->kind_uniform_slots[k] && direct; j++)
        direct = (sl[j].ch == sl[0].ch + j) && sl[j].mode == sl[0].mode && sl[j].flags == sl[0].flags;
      b->kind_direct[k] = direct;
    }
    {
      const SlotInfo *sl = b->sched.data() + b->kind_first[ASDR_KERNEL_PLAIN];
      bool ssb = b->kind_uniform_slots[ASDR_KERNEL_PLAIN] > 0;
      for (int j = 0; j < b->kind_uniform_slots[ASDR_KERNEL_PLAIN] && ssb; j += 8) {
        const uint32_t m = sl[j].mode;
        ssb = (m == ASDR_USBmode || m == ASDR_LSBmode || m == ASDR_CW_USBmode || m == ASDR_CW_LSBmode || m == ASDR_WSPRmode ||
               m == ASDR_AMmode);   // (round 3: the pipeline's role 2 also runs the envelope detector)
      }
      b->plain_uniform_ssb = ssb;
    }
    b->sched_dirty = false;
    sched_rebuilt = true;
    b->stat_sched_rebuilds++;
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) b->puni_recheck[k] = true;
  }
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) if (b->puni_recheck[k]) puni_pass(b, k);
}

int flush(asdr_batch *b, hipStream_t stream) {
  const int rows = b->n + 1;
  std::vector<int32_t> changed;
  bool bulk = false, sched_rebuilt = false;
  flush_host(b, changed, bulk, sched_rebuilt);
  bool uploaded = false;
  if (b->agc_pool_dirty) {
    const size_t need = b->agc_pool.size() * ASDR_AGC_TAB_ROW;
    if (need > b->agc_tab_cap) {
      HIPCHK(hipStreamSynchronize(stream));      // ordered behind every earlier launch (update waits for ev_last first)
      if (b->d_agc_tab) HIPCHK(hipFree(b->d_agc_tab));
      b->agc_tab_cap = need * 2;
      HIPCHK(hipMalloc(&b->d_agc_tab, b->agc_tab_cap * sizeof(float)));
    }
    std::vector<float> flat(need);
    for (size_t i = 0; i < b->agc_pool.size(); i++) memcpy(&flat[i * ASDR_AGC_TAB_ROW], b->agc_pool[i].v, sizeof(float) * ASDR_AGC_TAB_ROW);
    HIPCHK(hipMemcpyAsync(b->d_agc_tab, flat.data(), need * sizeof(float), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));  // `flat` is a temporary
    b->agc_pool_dirty = false;
  }
  if (bulk) {
    HIPCHK(hipMemcpyAsync(b->d_params, b->hp.data(), rows * sizeof(ChanParams), hipMemcpyHostToDevice, stream));
    uploaded = true;
  } else {
    for (size_t i = 0; i < changed.size();) {   // one copy per run of consecutive rows
      size_t j = i + 1;
      while (j < changed.size() && changed[j] == changed[j - 1] + 1) j++;
      HIPCHK(hipMemcpyAsync(b->d_params + changed[i], &b->hp[changed[i]], (j - i) * sizeof(ChanParams), hipMemcpyHostToDevice, stream));
      uploaded = true;
      i = j;
    }
  }
  if (sched_rebuilt) {
    HIPCHK(hipMemcpyAsync(b->d_sched, b->sched.data(), b->sched.size() * sizeof(SlotInfo), hipMemcpyHostToDevice, stream));
    uploaded = true;
  }
  if (uploaded) HIPCHK(hipStreamSynchronize(stream));  // the host rows may be rewritten by the next setter + flush
  return 0;
}

void fill_args(asdr_batch *b, UpdateArgs &a) {
  memset(&a, 0, sizeof a);
  a.params = b->d_params; a.small = b->d_small;
  a.nb_hist = b->d_nb_hist; a.nb_mask = b->d_nb_mask; a.hil_q = b->d_hil_q; a.hil_i = b->d_hil_i;
  a.als_x = b->d_als_x; a.als_w = b->d_als_w; a.agc_tab = b->d_agc_tab;
  a.audio_prev = b->exact_unknown_mode ? b->d_audio_prev : nullptr;
  a.sched = b->d_sched; a.n_sched = 0; a.n_channels = b->n;   // the launcher sets the sub-range
  a.taps = b->taps_on ? b->d_taps : nullptr;
  a.nb_phase = b->nb_phase; a.als_phase = b->als_phase;
  a.lo_cache = b->d_lo; a.lo_parity = b->lo_parity; a.lo_write = 0; a.lo_writer_bit = ASDR_LO_WRITER;
  a.k = b->k;
}

// a direct launch of (a piece of) the group whose first channel is ch0: the group's one parameter row as launch constants, when it has one
void set_uni(asdr_batch *b, UpdateArgs &a, int ch0) {
  const int k = kernel_kind(b->hp[ch0]);
  a.uni_valid = 0u;
  if (b->uniform_params && b->kind_direct[k] && b->kind_puni[k] && b->sched[b->kind_first[k]].ch == ch0) { a.uni = b->hp[ch0]; a.uni_valid = 1u; }
}

int apply_resets(asdr_batch *b, hipStream_t stream) {
  if (!b->reset_pending) return 0;
  const int lo = b->reset_lo < 0 ? 0 : b->reset_lo, hi = b->reset_hi > b->n ? b->n : b->reset_hi;
  if (hi >= lo) {   // only the rows that carry bits travel and get a workgroup
    const int cnt = hi - lo + 1;
    HIPCHK(hipMemcpyAsync(b->d_reset + lo, b->reset.data() + lo, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    UpdateArgs a;
    fill_args(b, a);
    if (asdr_launch_reset(&a, b->d_reset, lo, cnt, stream) != 0) return fail("reset kernel launch failed");
    HIPCHK(hipStreamSynchronize(stream));
    std::fill(b->reset.begin() + lo, b->reset.begin() + hi + 1, 0u);
  }
  b->reset_pending = false; b->reset_lo = 0x7fffffff; b->reset_hi = -1;
  return 0;
}

// ---- sharded batches: routing of global channel indices ---------------------------------------------------------------------
inline bool is_sharded(const asdr_batch *b) { return b && !b->shards.empty(); }
// the shard that owns global channel `ch` (which becomes the shard-local index), or nullptr
asdr_batch *shard_of(asdr_batch *b, int &ch) {
  if (ch < 0 || ch >= b->n) return nullptr;
  const std::vector<int> &f = b->shard_first;
  int g = (int)(std::upper_bound(f.begin(), f.end(), ch) - f.begin()) - 1;
  ch -= f[g];
  return b->shards[g];
}
// Setters.  The lambdas of the entry points capture their `b` parameter by reference and `each` takes that same variable by
// reference: for a sharded batch it is pointed at the owning shard (every shard in turn for ASDR_ALL) while `f` runs, so that the
// per-batch helpers the lambdas call (chan_init, set_mode, mark_reset, rebuild_agc) work on the owner.
template <typename F>
void each(asdr_batch *&b, int ch, F f) {
  if (!b) return;
  if (is_sharded(b)) {
    asdr_batch *const parent = b;
    if (ch == ASDR_ALL) { for (asdr_batch *sh : parent->shards) { b = sh; each(b, ASDR_ALL, f); } }
    else { int local = ch; asdr_batch *sh = shard_of(parent, local); if (sh) { b = sh; each(b, local, f); } }
    b = parent;
    return;
  }
  if (ch == ASDR_ALL) { for (int i = 0; i < b->n; i++) f(i, b->ch[i]); b->all_dirty = true; }
  else if (ch >= 0 && ch < b->n) { f(ch, b->ch[ch]); mark_dirty(b, ch); }
  else return;
}
// Getters: `b` is left pointing at the owner (the callers only read through it afterwards).
const Chan *get(asdr_batch *&b, int ch) {
  if (is_sharded(b)) { asdr_batch *sh = shard_of(b, ch); if (!sh) return nullptr; b = sh; }
  return (b && ch >= 0 && ch < b->n) ? &b->ch[ch] : nullptr;
}

// Helper streams (aux: concurrent sub-range launches of a call; lanes: never-joined pieces of a batch) come from ONE pool per device
// and process, created at first use.  HIP maps the streams in use onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default): from
// the fifth on, streams share a queue, and what shares a queue runs one after the other with barrier packets in between -- a batch
// that owns 24 streams changes the mapping for every other stream of the process (C4's three concurrent sub-range launches: 0.345 ms
// per step, 0.404 with nine unused lane streams created beside them; a single back-to-back kernel stream: 0.122 -> 0.152).  Sharing
// a pool stream between batches only adds ordering nobody needs; it never breaks the ordering somebody does (a stream is in-order).
constexpr int kPoolMax = 16;
int g_pool_priority = -1;   // -1: ASDR_POOL_PRIORITY or the default (highest); 0 normal, 1 highest, 2 lowest (asdr_set_pool_priority)
bool g_pool_created = false;
struct StreamPool { hipStream_t s[kPoolMax] = {}; int size = 0; std::mutex m; };
StreamPool g_pool[16];   // [kPoolDevices]
constexpr int kPoolDevices = 16;   // device ordinals 0 .. 15 (a node holds 8)
hipStream_t pool_stream(int device, int i) {
  if (device < 0 || device >= kPoolDevices) return nullptr;
  StreamPool &p = g_pool[device];
  std::lock_guard<std::mutex> g(p.m);
  if (p.size == 0) { const char *e = getenv("ASDR_STREAM_POOL"); p.size = e ? std::max(1, std::min(atoi(e), kPoolMax)) : 3; }
  const int k = (i < 0) ? p.size - 1 : i % p.size;
  if (!p.s[k]) {
    // The pool's streams are created at the HIGHEST stream priority (round 5).  The runtime keeps its hardware queues per priority level, so the
    // pool no longer shares queues with whatever streams the application creates at the default priority: with two application streams
    // created in front of the pool the lanes' overlap probe read "serialised" (lanes off: 0.110 instead of 0.099 ms per C2 step), and the
    // role streams of a caller with a stream of its own ran 57 instead of 37 us per SAM block -- both gone at either other priority
    // (profiles/README.md).  ASDR_POOL_PRIORITY=normal | low: the default level (round 4's behaviour) / the lowest.
    // (asdr_set_pool_priority, before the first batch of the process, overrides the environment: a library kernel on a highest-priority stream
    // is scheduled in front of the application's default-priority work on the same device -- an application that runs latency-critical kernels
    // of its own beside the receiver bank may prefer "normal" and live with shared hardware queues.)
    static const char *pe_env = getenv("ASDR_POOL_PRIORITY");
    const char *pe = (g_pool_priority == 0) ? "normal" : (g_pool_priority == 2) ? "low" : (g_pool_priority == 1) ? nullptr : pe_env;
    hipError_t rc;
    if (pe == nullptr || pe[0] != 'n') {
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      rc = hipStreamCreateWithPriority(&p.s[k], hipStreamNonBlocking, (pe != nullptr && pe[0] == 'l') ? least : greatest);
      if (rc != hipSuccess) { (void)hipGetLastError(); rc = hipStreamCreateWithFlags(&p.s[k], hipStreamNonBlocking); }
    } else rc = hipStreamCreateWithFlags(&p.s[k], hipStreamNonBlocking);
    if (rc != hipSuccess) { (void)hipGetLastError(); p.s[k] = nullptr; return nullptr; }
    g_pool_created = true;
  }
  return p.s[k];
}
// Do two streams of the pool really run at the same time?  The lanes rest on it: HIP maps the streams of a process onto a
// few hardware queues, and two streams that share a queue run one after the other -- then two never-joined halves gain nothing and a
// batch does better on its caller's stream order.  Probed at the first call that would use the lanes (not at asdr_create: round 5): a
// 30-us spin kernel on each of the pool's first two streams; together they end after one duration (concurrent) or two (serialised).
// 1 = concurrent, 0 = serialised (batches then stay on the ordinary path unless asdr_set_lanes asked for the lanes), -1 = not probed / the probe itself failed
// (lanes stay at their default: an error here must not change behaviour).
// Round 6: the verdict no longer rests on absolute microseconds -- ONE spin on one stream is timed first (duration + launch and event
// latency of this box, this moment), the pair counts as concurrent when its later end is below 1.5 x that; three rounds, majority; and a
// "serialised" verdict is not kept for the process: it holds for the batch that asked (asdr_lanes_enabled says so), the next batch's first
// lane-sized call probes again, up to three times per device (streams created meanwhile may have re-mapped the queues either way).
int g_lanes_probe[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
int g_lanes_probe_last[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};   // the last verdict, cached or not (asdr_lanes_overlap_probe)
int g_lanes_probe_tries[16] = {};
extern "C" int asdr_launch_spin(unsigned long long ticks, hipStream_t stream);
int lanes_overlap_probe(int device) {
  if (device < 0 || device >= kPoolDevices) return -1;
  static std::mutex pm;
  std::lock_guard<std::mutex> g(pm);
  if (g_lanes_probe[device] >= 0) return g_lanes_probe[device];
  if (getenv("ASDR_NO_LANES_PROBE")) return -1;
  hipStream_t s0 = pool_stream(device, 0), s1 = pool_stream(device, 1);
  if (!s0 || !s1 || s0 == s1) return -1;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool ok = true;
  for (hipEvent_t &e : ev) if (hipEventCreate(&e) != hipSuccess) ok = false;
  const unsigned long long ticks = 3000;   // 30 us at 100 MHz
  int votes = 0, rounds = 0;
  // warm both streams (first launches pay code-object loading)
  ok = ok && asdr_launch_spin(10, s0) == 0 && asdr_launch_spin(10, s1) == 0 && hipStreamSynchronize(s0) == hipSuccess && hipStreamSynchronize(s1) == hipSuccess;
  for (int r = 0; r < 3 && ok; r++) {
    float alone = 0.0f, both = 0.0f, one = 0.0f;
    // one spin on its own: the yardstick
    ok = ok && hipEventRecord(ev[0], s0) == hipSuccess && asdr_launch_spin(ticks, s0) == 0 && hipEventRecord(ev[1], s0) == hipSuccess;
    ok = ok && hipStreamSynchronize(s0) == hipSuccess && hipEventElapsedTime(&alone, ev[0], ev[1]) == hipSuccess;
    // the pair, both behind the same marker
    ok = ok && hipEventRecord(ev[0], s0) == hipSuccess && hipStreamWaitEvent(s1, ev[0], 0) == hipSuccess;
    ok = ok && asdr_launch_spin(ticks, s0) == 0 && asdr_launch_spin(ticks, s1) == 0;
    ok = ok && hipEventRecord(ev[1], s0) == hipSuccess && hipEventRecord(ev[2], s1) == hipSuccess;
    ok = ok && hipStreamSynchronize(s0) == hipSuccess && hipStreamSynchronize(s1) == hipSuccess;
    ok = ok && hipEventElapsedTime(&one, ev[0], ev[1]) == hipSuccess && hipEventElapsedTime(&both, ev[0], ev[2]) == hipSuccess;
    if (!ok) break;
    rounds++;
    if (std::max(one, both) < 1.5f * alone) votes++;
  }
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  if (!ok || rounds == 0) { (void)hipGetLastError(); return -1; }
  const int verdict = (2 * votes > rounds) ? 1 : 0;
  g_lanes_probe_last[device] = verdict;
  if (verdict == 1 || ++g_lanes_probe_tries[device] >= 3) g_lanes_probe[device] = verdict;   // "concurrent" is kept; "serialised" only after three batches found it
  return verdict;
}
hipStream_t aux_stream(asdr_batch *b, int i) {
  if (!b->aux[i]) b->aux[i] = pool_stream(b->device, i + 1);   // (+ 1: a lane call's pieces and an ordinary call's helpers start on different pool streams)
  return b->aux[i];
}
hipStream_t lane_stream(asdr_batch *b, int l) {
  if (!b->lane[l]) b->lane[l] = pool_stream(b->device, l);
  return b->lane[l];
}
bool needs_flush(const asdr_batch *b) {
  return b->all_dirty || !b->dirty.empty() || b->sched_dirty || b->agc_pool_dirty || b->reset_pending || b->agc_refs_changed;
}
// everything the lanes hold so far happens before whatever is enqueued on `stream` from now on
int lanes_join_into(asdr_batch *b, hipStream_t stream) {
  for (int i = 0; i <= b->sched_lanes; i++) {   // the lanes in use, and the stream of the uncut sub-ranges (a schedule change synchronises them all first)
    const int l = (i == b->sched_lanes) ? ASDR_LANES : i;
    if (!b->lane[l]) continue;   // never used
    HIPCHK(hipEventRecord(b->ev_lane[l], b->lane[l])); HIPCHK(hipStreamWaitEvent(stream, b->ev_lane[l], 0));
  }
  return 0;
}
// ... and the batch's last call (on another stream than `stream`) happens before whatever is enqueued on `stream` from now on.  The event is recorded now, on
// that call's stream -- behind everything it enqueued there -- rather than after every call: one packet less per launch for the common single-stream caller.
int wait_for_last(asdr_batch *b, hipStream_t stream) { HIPCHK(hipEventRecord(b->ev_last, b->last_stream)); HIPCHK(hipStreamWaitEvent(stream, b->ev_last, 0)); return 0; }
int sync_all(asdr_batch *b);
// an ordinary call on `stream` after calls on the lanes: behind them -- on the host when a flush is due, which rewrites rows the lanes' kernels read
int leave_lanes(asdr_batch *b, hipStream_t stream) {
  if (!b->lanes_pending) return 0;
  if (needs_flush(b)) { if (sync_all(b) != 0) return -1; }
  else { if (lanes_join_into(b, stream) != 0) return -1; b->lanes_pending = false; }
  b->last_stream = stream; b->last_was_lanes = false;
  return 0;
}
// host-side: every launch of the batch so far is complete
int sync_all(asdr_batch *b) {
  HIPCHK(hipStreamSynchronize(b->last_stream));   // nullptr = the null stream
  HIPCHK(hipStreamSynchronize(b->stream));
  if (b->lanes_pending) { for (int l = 0; l < ASDR_LANES + 1; l++) if (b->lane[l]) HIPCHK(hipStreamSynchronize(b->lane[l])); b->lanes_pending = false; }

  return 0;
}

// The streaming pipeline's recovery counter (a wave gave up waiting for its neighbour role, the call was re-run on the in-kernel
// block loop from the snapshot: asdr_kernels.hip "the pipeline as a transaction"): read back at the host's synchronisation points
// (asdr_synchronize, asdr_update, the status / capture readers).  Results are exact either way; this is only a statistic.
int check_stream_error(asdr_batch *b) {
  if (!b->stream_launched || !b->d_stream_prog) return 0;
  if (sync_all(b) != 0) return -1;
  uint32_t *word = b->d_stream_prog + 3 * ((b->n + 7) / 8) + 1, v[2] = {0, 0};
  HIPCHK(hipMemcpy(v, word, sizeof v, hipMemcpyDeviceToHost));
  b->stream_launched = false;
  b->stat_stream_recoveries = (long)v[1];
  if (v[0]) return fail("streaming pipeline: error word still set after the recovery launches (internal error)");
  return 0;
}

int read_small(asdr_batch *b, int ch, ChanSmall &s) {
  if (!b || ch < 0 || ch >= b->n) return fail("bad channel");
  if (is_sharded(b)) b = shard_of(b, ch);
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch has no device state");
  HIPCHK(hipSetDevice(b->device));
  if (sync_all(b) != 0) return -1;
  if (check_stream_error(b) != 0) return -1;
  if (apply_resets(b, b->stream) != 0) return -1;
  HIPCHK(hipMemcpy(&s, b->d_small + ch, sizeof s, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

// a sharded batch: the same call on every shard, first failure wins
#define FOR_SHARDS(b, call) do { if (is_sharded(b)) { for (asdr_batch *sh_ : (b)->shards) { const int rc_ = (call); if (rc_ != 0) return rc_; } return 0; } } while (0)

extern "C" {

const char *asdr_last_error(void) { return g_err.c_str(); }
}  // extern "C"
// shared with asdr_front_host.cpp (internal C++ linkage, not part of the C ABI)
int asdr_internal_fail(const std::string &m) { return fail(m); }
extern "C" {
const char *asdr_version(void) { return "asdr-hip 0.1 (gfx950, wave64, -ffp-contract=off)"; }

asdr_batch_t *asdr_create(int n_channels, int device) {
  if (n_channels <= 0 || n_channels > (1 << 20)) { fail("n_channels must be in 1..1048576"); return nullptr; }
  asdr_batch *b = new asdr_batch();
  b->n = n_channels; b->device = device;
  b->sam_fused = getenv("ASDR_SAM_FUSED") != nullptr;
  b->sam_split_min = getenv("ASDR_SAM_SPLIT_MIN") ? atoi(getenv("ASDR_SAM_SPLIT_MIN")) : ASDR_SAM_SPLIT_MIN_CHANNELS;
  b->stream_pipeline = getenv("ASDR_NO_STREAM_PIPELINE") == nullptr;
  b->uniform_params = getenv("ASDR_NO_UNIFORM_PARAMS") == nullptr;
  b->alternate_order = getenv("ASDR_ALTERNATE_ORDER") != nullptr && getenv("ASDR_NO_ALTERNATE_ORDER") == nullptr;
  b->als_split_min = getenv("ASDR_ALS_SPLIT_MIN") ? atoi(getenv("ASDR_ALS_SPLIT_MIN")) : 0x7fffffff;
  if (getenv("ASDR_LAUNCH_SPLIT")) b->launch_split = std::max(1, std::min(atoi(getenv("ASDR_LAUNCH_SPLIT")), 8));
  if (getenv("ASDR_LAUNCH_SPLIT_MIN_WAVES")) b->launch_split_min_waves = std::max(8, atoi(getenv("ASDR_LAUNCH_SPLIT_MIN_WAVES")));
  const size_t rows = (size_t)n_channels + 1;
  if (device != ASDR_NO_DEVICE) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { delete b; fail("no HIP device: libasdr_hip has no CPU path"); return nullptr; }
    if (device < 0 || device >= ndev) { delete b; fail("bad device ordinal"); return nullptr; }
    if (device >= 16) { delete b; fail("device ordinal >= 16: the per-device stream pool of this library has 16 entries"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { delete b; fail("hipSetDevice failed"); return nullptr; }
    autopin_batch_created();   // (paired with asdr_destroy, which every later failure path goes through)
    bool ok = true;
    auto alloc = [&](void **p, size_t bytes) { if (ok && hipMalloc(p, bytes) != hipSuccess) ok = false; };
    alloc((void **)&b->d_params, rows * sizeof(ChanParams));
    alloc((void **)&b->d_small, rows * sizeof(ChanSmall));
    alloc((void **)&b->d_nb_hist, rows * 768 * sizeof(int16_t));
    alloc((void **)&b->d_nb_mask, rows * ASDR_NB_MASK_ROW * sizeof(uint8_t));
    alloc((void **)&b->d_hil_q, rows * 256 * sizeof(float));
    alloc((void **)&b->d_hil_i, rows * 256 * sizeof(float));
    alloc((void **)&b->d_als_x, rows * 256 * sizeof(float));
    alloc((void **)&b->d_als_w, rows * 128 * sizeof(float));
    alloc((void **)&b->d_audio_prev, rows * 128 * sizeof(float));
    if (ok && hipMemset(b->d_audio_prev, 0, rows * 128 * sizeof(float)) != hipSuccess) ok = false;
    alloc((void **)&b->d_sched, (rows + 32) * sizeof(SlotInfo));   // three sub-ranges, each padded to a whole wave
    alloc((void **)&b->d_reset, rows * sizeof(uint32_t));
    alloc((void **)&b->d_lo, (1 + ASDR_LANES) * 2 * ASDR_LO_ENTRIES * sizeof(LoEntry));   // + one set per lane: a lane's readers only ever see its own writer
    if (ok && hipMemset(b->d_lo, 0xFF, (1 + ASDR_LANES) * 2 * ASDR_LO_ENTRIES * sizeof(LoEntry)) != hipSuccess) ok = false;   // keys no phase can match
    // hipMemset on device memory runs on the NULL stream and does not wait for itself on the host; the batch's kernels run on non-blocking
    // streams, which the null stream does not order: without this the fills above can land AFTER a first kernel's stores (round 4's
    // launch-form fuzz caught exactly that on the stage taps: one word of a tap row zeroed behind the kernel that had written it)
    if (ok && hipStreamSynchronize(nullptr) != hipSuccess) ok = false;
    for (int i = 0; i < ASDR_LANES + 1 && ok; i++)
      if (hipEventCreateWithFlags(&b->ev_lane[i], hipEventDisableTiming) != hipSuccess) ok = false;
    b->lanes_enabled = getenv("ASDR_NO_LANES") == nullptr;   // (the overlap probe runs at the first call that would use the lanes: plan_enter)
    b->sam_role_streams = getenv("ASDR_NO_SAM_ROLE_STREAMS") == nullptr;
    b->sam_chunks = getenv("ASDR_NO_SAM_CHUNKS") == nullptr;
    b->als_role_streams = getenv("ASDR_NO_ALS_ROLE_STREAMS") == nullptr;
    if (getenv("ASDR_ALS_ROLE_STAGES")) b->als_role_stages = atoi(getenv("ASDR_ALS_ROLE_STAGES")) == 2 ? 2 : 3;
    if (ok && (b->stream = pool_stream(device, 0)) == nullptr) ok = false;   // the pool's first stream (= lane 0: a batch runs on the lanes or on its own stream, never both at once)
    if (ok && hipEventCreate(&b->ev0) != hipSuccess) ok = false;
    if (ok && hipEventCreate(&b->ev1) != hipSuccess) ok = false;
    if (ok && hipEventCreate(&b->rev0) != hipSuccess) ok = false;
    if (ok && hipEventCreate(&b->rev1) != hipSuccess) ok = false;
    if (ok && hipEventCreateWithFlags(&b->ev_last, hipEventDisableTiming) != hipSuccess) ok = false;
    if (ok && hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming) != hipSuccess) ok = false;
    // The helper streams (aux, lanes) are created at their first use: HIP maps streams onto a few hardware queues, and streams that
    // share a queue run one after the other -- every stream a batch creates but never uses shifts that mapping for the ones it does
    // use (C4's three concurrent sub-range launches: 0.345 ms per step, 0.404 with nine unused lane streams created beside them).
    for (int i = 0; i < ASDR_AUX_STREAMS && ok; i++)
      if (hipEventCreateWithFlags(&b->ev_join[i], hipEventDisableTiming) != hipSuccess) ok = false;
    if (ok && asdr_kernels_upload_tables() != 0) ok = false;
    if (ok) {
      // The pipeline's roles wait for each other: its 3 w workgroups must fit the device at once -- an occupancy query, not an
      // assumption about the part (MI355X: 6 workgroups of this kernel per compute unit x 256 = 1,536 -> 512 channel groups).
      // Measured with several workgroups per compute unit (tools/stream_sizes.py): 6.9 us per block up to 84 groups, 7.3 at 128,
      // 8.4 at 256, 11.0 at 512 -- against 18.9-20.2 us for the in-kernel block loop at every one of those sizes.
      int cus = 0;
      const int cap = asdr_stream_capacity(device, &cus, 1);
      const int cap3 = asdr_stream_capacity(device, nullptr, 3);
      b->stream_cap_h3 = cap3 > 0 ? cap3 : 0; b->stream_cus = cus;
      { const char *e = getenv("ASDR_STREAM_H3"); if (e) b->stream_h3 = atoi(e) != 0 ? 1 : 0; }
      b->stream_cap_workgroups = cap > 0 ? cap : 0;
      b->stream_max_waves = cap >= 3 ? cap / 3 : 0;
      if (b->stream_max_waves > ASDR_STREAM_MAX_WAVES) b->stream_max_waves = ASDR_STREAM_MAX_WAVES;
      b->stream_query_waves = b->stream_max_waves;
    }
    if (!ok) { fail("device allocation / table upload failed"); asdr_destroy(b); return nullptr; }
  }

  // constants shared by all channels: in-class initialisers of AudioSDR.h:238-239, 249-284
  ChainConsts &k = b->k;
  k.if_center = kIFcenter;
  k.two_pi_f = (float)(2.0 * kPI);
  k.half_pi_f = (float)(0.5 * kPI);
  k.inv_two_pi_d = 1.0 / (double)k.two_pi_f;
  k.sin_index_scale_d = (65535.0 / (double)k.two_pi_f) * (1.0 + 0x1p-49);
  k.half_pi_d = kPI / 2.0;
  k.phase_inc_unit = k.two_pi_f / kFs;
  k.nb_alpha = 0.995f;
  k.nb_beta = (float)(1.0 - (double)k.nb_alpha);
  {
    const float wn = 0.07f, zeta = 0.707f, Ka = 1000.f;
    const float tau1 = Ka / (wn * wn);
    const float tau2 = 2 * zeta / wn;
    k.pll_b0 = (float)((double)(2 * Ka / tau1) * (1.0 + 2.0 * (double)tau2));
    k.pll_b1 = (float)((double)(2 * Ka / tau1) * (1.0 - 2.0 * (double)tau2));
    k.pll_a1 = -1.0f;
  }
  k.pll_alpha_freq = 0.995f;
  k.pll_beta_freq = (float)(1.0 - (double)k.pll_alpha_freq);
  k.pll_f_conv = kFs / k.two_pi_f;
  k.pll_lock_lo = (float)((double)kIFcenter - 1000.0);
  k.pll_lock_hi = (float)((double)kIFcenter + 1000.0);

  b->ch.assign(rows, Chan());
  b->hp.resize(rows);
  memset(b->hp.data(), 0, rows * sizeof(ChanParams));
  b->dirty_flag.assign(rows, 0);
  b->puni_differs.assign(rows, 0);
  b->reset.assign(rows, ASDR_R_ALL);
  b->reset_lo = 0; b->reset_hi = (int)rows - 1;
  for (size_t i = 0; i < rows; i++) chan_init(b, (int)i);  // constructor -> init()
  b->all_dirty = true; b->sched_dirty = true; b->reset_pending = true;
  return b;
}

asdr_batch_t *asdr_create_sharded(int n_channels, int n_shards, const int *devices) {
  if (n_channels <= 0 || n_channels > (1 << 23)) { fail("n_channels must be in 1..8388608"); return nullptr; }
  if (n_shards <= 0 || n_shards > 64 || n_shards > n_channels || !devices) { fail("n_shards must be in 1..min(64, n_channels), with one device ordinal per shard"); return nullptr; }
  asdr_batch *b = new asdr_batch();
  b->n = n_channels; b->device = ASDR_NO_DEVICE;
  b->shard_first.resize((size_t)n_shards + 1);
  for (int g = 0; g <= n_shards; g++) b->shard_first[g] = (int)(((long)n_channels * g) / n_shards);   // audiosdr_amd/sharding.py shard_range
  for (int g = 0; g < n_shards; g++) {
    asdr_batch *sh = asdr_create(b->shard_first[g + 1] - b->shard_first[g], devices[g]);
    if (!sh) { const std::string e = g_err; asdr_destroy(b); fail("shard " + std::to_string(g) + ": " + e); return nullptr; }
    b->shards.push_back(sh);
  }
  b->k = b->shards[0]->k;
  return b;
}
int asdr_n_shards(const asdr_batch_t *b) { return b ? (is_sharded(b) ? (int)b->shards.size() : 1) : 0; }
asdr_batch_t *asdr_shard(asdr_batch_t *b, int shard) {
  if (!b) return nullptr;
  if (!is_sharded(b)) return shard == 0 ? b : nullptr;
  return (shard >= 0 && shard < (int)b->shards.size()) ? b->shards[shard] : nullptr;
}
int asdr_shard_first_channel(const asdr_batch_t *b, int shard) {
  if (!b) return -1;
  if (!is_sharded(b)) return shard == 0 ? 0 : (shard == 1 ? b->n : -1);
  return (shard >= 0 && shard <= (int)b->shards.size()) ? b->shard_first[shard] : -1;   // shard == n_shards: the total
}
int asdr_shard_device(const asdr_batch_t *b, int shard) {
  if (!b) return ASDR_NO_DEVICE;
  if (!is_sharded(b)) return b->device;
  return (shard >= 0 && shard < (int)b->shards.size()) ? b->shards[shard]->device : ASDR_NO_DEVICE;
}

void asdr_destroy(asdr_batch_t *b) {
  if (!b) return;
  if (is_sharded(b) || !b->shard_first.empty()) { shard_workers_stop(b); for (asdr_batch *sh : b->shards) asdr_destroy(sh); delete b; return; }
  if (b->device == ASDR_NO_DEVICE) { delete b; return; }
  hipSetDevice(b->device);
  hipDeviceSynchronize();
  autopin_batch_gone();   // (the last device batch of the process takes the auto-pinned caller ranges with it)
  void *ptrs[] = {b->d_params, b->d_small, b->d_nb_hist, b->d_nb_mask, b->d_hil_q, b->d_hil_i, b->d_als_x, b->d_als_w,
                  b->d_agc_tab, b->d_taps, b->d_sched, b->d_reset, b->d_lo, b->d_io[0], b->d_io[1], b->d_io[2], b->d_capture,
                  b->d_xch_a, b->d_xch_b, b->d_stream_prog, b->d_lo_ring, b->d_xch_sam, b->d_audio_prev, b->d_stream_snap, b->d_als_stage, b->d_xch_sam_chunk};
  for (void *p : ptrs) if (p) hipFree(p);
  b->copy_pool.reset();
  for (int i = 0; i < 3; i++) if (b->h_io[i]) hipHostFree(b->h_io[i]);
  if (b->st_d) hipFree(b->st_d);
  if (b->st_h) hipHostFree(b->st_h);
  if (b->st_ev) hipEventDestroy(b->st_ev);
  for (hipEvent_t e : b->ev_host) hipEventDestroy(e);
  for (hipEvent_t e : b->tev) hipEventDestroy(e);
  if (b->ev0) hipEventDestroy(b->ev0);
  if (b->ev1) hipEventDestroy(b->ev1);
  if (b->rev0) hipEventDestroy(b->rev0);
  if (b->rev1) hipEventDestroy(b->rev1);
  if (b->ev_last) hipEventDestroy(b->ev_last);
  if (b->ev_fork) hipEventDestroy(b->ev_fork);
  for (int i = 0; i < ASDR_AUX_STREAMS; i++) if (b->ev_join[i]) hipEventDestroy(b->ev_join[i]);   // (the streams belong to the process-wide pool)
  for (int i = 0; i < ASDR_LANES + 1; i++) if (b->ev_lane[i]) hipEventDestroy(b->ev_lane[i]);
  for (int i = 0; i < 6; i++) if (b->ev_role[i]) hipEventDestroy(b->ev_role[i]);
  for (hipEvent_t e : b->ev_als) if (e) hipEventDestroy(e);
  for (hipEvent_t e : b->ev_samc) if (e) hipEventDestroy(e);
  // (b->stream and the helper streams belong to the process-wide pool)
  delete b;
}

int asdr_n_channels(const asdr_batch_t *b) { return b ? b->n : 0; }

}  // extern "C"
// ---- the device-call dispatcher --------------------------------------------------------------------------------
// One call, or one PART of a call: with parts > 1 only the waves [w part / parts, w (part + 1) / parts) of every sub-range of the schedule are launched, and the
// batch's block counters advance with the last part.  The parts of a call touch disjoint channels (every schedule slot is launched exactly once:
// tests/test_launch_plan.py) and are enqueued on one stream: the overlapped host-pointer path (asdr_update) starts part p as soon as the input rows of ITS channels
// have arrived and copies a channel range out as soon as the parts that hold its channels are done.
// A call is planned once (CallPlan: every decision taken in front of the first launch) and issued by ONE launch form: the block pipeline, the lanes, SAM role
// streams in chunks, ALS role streams, or the item loop.  The order of HIP calls inside a form is the behaviour: tools/host_trace.py holds it against a revision.
namespace {
struct Sub { int kind, uniform, first, slots; };   // a sub-range of the sorted schedule: the slots of one kernel instantiation
struct Item { int sub, first, slots; };            // (a piece of) this part's waves of a sub-range: one launch of the item loop
struct CallPlan {
  const int16_t *dI, *dQ; int16_t *dOut; int n_blocks, part, parts; long in_stride, out_stride;
  hipStream_t stream; bool batch_stream, use_lanes;
  hipEvent_t e0, e1;                               // timing markers around the call's launches, or null
  Sub subs[ASDR_KERNEL_KINDS + 2]; int n_sub;      // heaviest instantiation first
  bool sam_split, als_split;                       // SAM channels as pre | PLL | post launches, short ALS filters as chain | filter
  bool per_block; int n_launch;                    // one launch per block: n_launch = n_blocks, else 1
  bool take_pipeline; int pipe_sub, other_waves;   // the block pipeline takes subs[pipe_sub]; other_waves run beside it
  Item items[ASDR_AUX_STREAMS + 1]; int n_items, main_item;   // (not filled for the pipeline and the lanes)
  bool sam_roles, sam_chunks, als_roles; int n_chunks;        // role streams; sam_chunks: by the rule -- the tile sets are reserved at the launch
};
// (a piece of) sub-range `su` into the launch arguments: the slots [first, first + slots) of the schedule, and a direct group -- one key group of consecutive
// channels: no schedule reads in the waves -- as launch constants.  lo_write: the first wave of every settings group fills the group's entry of the other half of
// the local-oscillator cache; a direct launch's wave 0 is its group's writer, so of the pieces of a direct group only the one that holds the group's first wave may
// write -- unless every piece has a writer bit and an entry set of its own (`own_writers`: the lanes).
void select_slots(asdr_batch *b, UpdateArgs &a, const Sub &su, int first, int slots, bool own_writers) {
  a.sched = b->d_sched + first; a.n_sched = slots; a.direct_ch0 = -1; a.uni_valid = 0u; a.lo_write = 1u;
  if (su.uniform && b->kind_direct[su.kind]) {
    const SlotInfo &s0 = b->sched[su.first];
    a.direct_ch0 = s0.ch + (first - su.first); a.direct_mode = s0.mode; a.direct_flags = s0.flags; a.direct_lo = s0.lo; set_uni(b, a, s0.ch);
    if (first != su.first && !own_writers) a.lo_write = 0u;
  }
}
// the launch works on the blocks [b0, b0 + count) of the call; `flips` launches of the call have flipped the oscillator cache's halves before it
void point_at_blocks(const asdr_batch *b, const CallPlan &p, UpdateArgs &a, int b0, int count, int flips) {
  a.in_i = p.dI + (size_t)b0 * ASDR_N; a.in_q = p.dQ + (size_t)b0 * ASDR_N; a.out = p.dOut + (size_t)b0 * ASDR_N; a.n_blocks = count;
  a.nb_phase = (b->nb_phase + (uint32_t)(b0 % 3)) % 3u; a.als_phase = (b->als_phase + (uint32_t)b0) & 1u; a.lo_parity = b->lo_parity ^ (uint32_t)(flips & 1);
}
// tiles / lock words of the slots [first, ..) of a SAM kind's sub-range, set `parity` (0 everywhere but in the role streams per block)
void set_sam_rows(const asdr_batch *b, UpdateArgs &a, int kind, int first, int parity) {
  const size_t at = (size_t)(first - b->kind_first[kind]) + (kind == ASDR_KERNEL_SAM_ALS ? (size_t)b->kind_slots[ASDR_KERNEL_SAM] : 0);
  a.xch_sam = b->d_xch_sam + ((size_t)parity * b->xch_sam_slots + at) * 2 * ASDR_N;
  a.sam_lock = reinterpret_cast<uint32_t *>(b->d_xch_sam + 2 * b->xch_sam_slots * 2 * ASDR_N) + (size_t)parity * b->xch_sam_slots + at;
}
// the chunked forms' tile sets: ASDR_SAM_CHUNK_SETS sets of tiles, the lock words behind them (the launch's first set: a.sam_set)
void set_chunk_tiles(const asdr_batch *b, UpdateArgs &a) {
  const size_t slots = b->xch_sam_chunk_slots;
  a.xch_sam = b->d_xch_sam_chunk; a.sam_lock = reinterpret_cast<uint32_t *>(b->d_xch_sam_chunk + (size_t)ASDR_SAM_CHUNK_SETS * slots * 2 * ASDR_N);
  a.sam_sets = (uint32_t)ASDR_SAM_CHUNK_SETS; a.sam_set_stride = (uint32_t)(slots * 2 * ASDR_N); a.sam_lock_stride = (uint32_t)slots;
}
// The exchange tiles grow on demand: `sets` sets of tiles for `slots` schedule slots and the sets' lock words behind them (d_xch_sam: two sets, consecutive blocks
// alternate; d_xch_sam_chunk: ASDR_SAM_CHUNK_SETS).  Pointer and size change only once the allocation succeeded; false: no memory.
bool reserve_tiles(float *&tiles, size_t &have, int slots, int sets, hipStream_t stream) {
  if ((size_t)slots <= have) return true;
  float *grown = nullptr;
  const size_t per_set = (size_t)slots * 2 * ASDR_N * sizeof(float) + (size_t)slots * sizeof(uint32_t);
  if (hipStreamSynchronize(stream) != hipSuccess || hipMalloc(&grown, sets * per_set) != hipSuccess) { (void)hipGetLastError(); return false; }
  if (tiles) hipFree(tiles);
  tiles = grown; have = (size_t)slots;
  return true;
}
bool reserve_chunk_tiles(asdr_batch *b, int slots, hipStream_t stream) { return reserve_tiles(b->d_xch_sam_chunk, b->xch_sam_chunk_slots, slots, ASDR_SAM_CHUNK_SETS, stream); }
// the pipeline's buffers at its first use: every one, or none (false: the batch stays on the other launch forms for good)
bool reserve_pipeline(asdr_batch *b, hipStream_t stream) {
  if (b->d_xch_a) return true;
  float *xa = nullptr, *xb = nullptr; uint32_t *prog = nullptr; LoEntry *ring = nullptr; void *snap = nullptr;
  const size_t n_prog = (size_t)(3 * ((b->n + 7) / 8) + 3);   // [.. + 1] = the error word, [.. + 2] = the recovery counter
  const bool ok = hipMalloc(&xa, (size_t)(b->n + 1) * ASDR_STREAM_DEPTH * 2 * ASDR_N * sizeof(float)) == hipSuccess &&
                  hipMalloc(&xb, (size_t)(b->n + 1) * ASDR_STREAM_DEPTH * (ASDR_N + 1) * sizeof(float)) == hipSuccess &&   // + the AM carrier words (xch_c) behind the rows
                  hipMalloc(&prog, n_prog * sizeof(uint32_t)) == hipSuccess &&
                  hipMalloc(&ring, ASDR_LO_RING * sizeof(LoEntry)) == hipSuccess &&
                  hipMalloc(&snap, (size_t)(((b->n + 7) / 8) * 8) * ASDR_SNAP_BYTES) == hipSuccess &&
                  hipMemsetAsync(prog, 0, n_prog * sizeof(uint32_t), stream) == hipSuccess;
  if (!ok) {   // (asdr_stream_pipeline_alloc_failures() counts this)
    for (void *q : {(void *)xa, (void *)xb, (void *)prog, (void *)ring, snap}) if (q) hipFree(q);
    (void)hipGetLastError();
    b->stream_pipeline = false; b->stat_stream_alloc_failures++;
    return false;
  }
  b->d_xch_a = xa; b->d_xch_b = xb; b->d_stream_prog = prog; b->d_lo_ring = ring; b->d_stream_snap = snap;
  return true;
}
// do the call's output rows overlap its I or Q rows?
bool rows_overlap(const asdr_batch *b, const CallPlan &p) {
  const uintptr_t in_bytes = ((uintptr_t)(b->n - 1) * (uintptr_t)p.in_stride + (uintptr_t)p.n_blocks) * ASDR_N * sizeof(int16_t);
  const uintptr_t out_bytes = ((uintptr_t)(b->n - 1) * (uintptr_t)p.out_stride + (uintptr_t)p.n_blocks) * ASDR_N * sizeof(int16_t);
  const uintptr_t o0 = (uintptr_t)p.dOut, o1 = o0 + out_bytes, i = (uintptr_t)p.dI, q = (uintptr_t)p.dQ;
  return (o0 < i + in_bytes && i < o1) || (o0 < q + in_bytes && q < o1);
}
// the lanes in use, and the stream of the uncut sub-ranges behind them, wait for `ev`
int lanes_fork(asdr_batch *b, hipEvent_t ev) {
  for (int i = 0; i <= b->sched_lanes; i++) {
    hipStream_t ls = lane_stream(b, i == b->sched_lanes ? ASDR_LANES : i);
    if (!ls) return fail("stream creation failed");
    HIPCHK(hipStreamWaitEvent(ls, ev, 0));
  }
  return 0;
}
// the order of launched block lb of this call, for a sub-range that may take it: a direct group of the plain kind, one block per launch (the launcher has the last
// word: asdr_launch_update_ordered reports whether the kernel it chose honours the field)
uint32_t order_bit(const asdr_batch *b, const CallPlan &p, const Sub &su, int direct_ch0, int lb) {
  const bool may = b->alternate_order && su.kind == ASDR_KERNEL_PLAIN && su.uniform && direct_ch0 >= 0 && (p.per_block || p.n_blocks == 1);
  return may ? (b->wg_parity ^ (uint32_t)lb) & 1u : 0u;
}
// The end of every call: what the next call and the timing getters read, and the batch's block counters.  lo_flips: the launches that flipped the oscillator
// cache's halves; order_flips: the launched blocks the alternating order counts; on_lanes: the call stays on the lanes, with nothing ordered behind it yet
// (last_stream is then still the last ordinary call's).
int end_call(asdr_batch *b, const CallPlan &p, int lo_flips, int order_flips, bool on_lanes) {
  if (p.e1) HIPCHK(hipEventRecord(p.e1, p.stream));
  b->ev_last_valid = true; b->ev_valid = (p.e0 != nullptr && p.e0 == b->ev0);
  if (b->region_calls >= 0) b->region_calls++;
  if (!on_lanes) b->last_stream = p.stream;
  b->lanes_pending = on_lanes; b->last_was_lanes = on_lanes;
  b->nb_phase = (b->nb_phase + (uint32_t)(p.n_blocks % 3)) % 3u; b->als_phase = (b->als_phase + (uint32_t)p.n_blocks) & 1u;
  b->lo_parity ^= (uint32_t)(lo_flips & 1); b->wg_parity ^= (uint32_t)(order_flips & 1);
  return 0;
}
// The call's arguments, its stream, whether it runs on the lanes, and its place behind the batch's earlier calls; setters and resets are applied here, so that what
// follows plans from the schedule as it will be launched.  1: go on, 0: nothing to do, -1: error.
int plan_enter(asdr_batch *b, CallPlan &p, const int16_t *dI, const int16_t *dQ, int16_t *dOut, int n_blocks, long in_stride_blocks,
               long out_stride_blocks, void *stream_, int part, int parts) {
  if (!b) return fail("null batch");
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch (ASDR_NO_DEVICE): the signal path needs a HIP device");
  if (!dI || !dQ) return 0;  // missing-input guard, AudioSDR.cpp:48-56
  if (!dOut) return fail("null output");
  if (n_blocks <= 0) return 0;
  if (in_stride_blocks < n_blocks || out_stride_blocks < n_blocks) return fail("row stride shorter than n_blocks");
  if (in_stride_blocks > 0x7fffffffL || out_stride_blocks > 0x7fffffffL) return fail("row stride too large");
  if ((((uintptr_t)dI | (uintptr_t)dQ | (uintptr_t)dOut) & 15u) != 0) return fail("I/Q/out device pointers must be 16-byte aligned");
  p.dI = dI; p.dQ = dQ; p.dOut = dOut; p.n_blocks = n_blocks; p.part = part; p.parts = parts; p.in_stride = in_stride_blocks; p.out_stride = out_stride_blocks;
  p.batch_stream = (stream_ == ASDR_STREAM_BATCH);
  hipStream_t stream = p.stream = p.batch_stream ? b->stream : (hipStream_t)stream_;
  HIPCHK(hipSetDevice(b->device));
  // Lanes (see asdr_batch): decided from the schedule as it stands -- a call that has setters or resets to apply runs the ordinary way (it synchronises anyway),
  // the next one is back on the lanes.
  p.use_lanes = false;
  if (parts == 1 && b->lanes_enabled && !needs_flush(b) && (p.batch_stream || n_blocks >= 2) && !b->taps_on && b->tev.empty() && !b->time_calls) {
    int total = b->left_slots;
    for (int k = 0; k < ASDR_KERNEL_KINDS; k++) total += b->kind_slots[k];
    // (a call the block pipeline may take is not a lane call: the pipeline runs on `stream` and needs that stream's ordering)
    const bool pipeline_candidate = b->stream_pipeline && n_blocks >= ASDR_STREAM_MIN_BLOCKS && b->plain_uniform_ssb &&
                                    b->kind_uniform_slots[ASDR_KERNEL_PLAIN] > 0 && b->kind_uniform_slots[ASDR_KERNEL_PLAIN] / 8 <= b->stream_max_waves;
    bool lanes_ok = !pipeline_candidate && total / 8 >= b->lanes_min_waves;
    // The first call that would take the lanes PROBES the pool on this device (once per device and process; not at asdr_create: a process that only ever calls on
    // its own streams never creates the pool's lane streams -- every stream a process creates can push its other streams onto a shared hardware queue).  Serialised
    // pool streams: the batch stays on the ordinary path unless the caller asked for the lanes explicitly (asdr_set_lanes).
    if (lanes_ok && !b->lanes_forced && lanes_overlap_probe(b->device) == 0) { b->lanes_enabled = false; lanes_ok = false; }
    p.use_lanes = lanes_ok &&
                  (p.batch_stream || total >= 8 * ASDR_PER_BLOCK_LAUNCH_WAVES || (b->sam_split && b->kind_slots[ASDR_KERNEL_SAM] + b->kind_slots[ASDR_KERNEL_SAM_ALS] > 0) ||
                   (b->als_split && b->kind_uniform_slots[ASDR_KERNEL_ALS_SMALL] > 0));   // (a strict call: only in its one-launch-per-block form)
  }
  if (!p.use_lanes && leave_lanes(b, stream) != 0) return -1;
  // one stream at a time per batch: a call on another stream first waits for the previous call's kernels (state in HBM is read-modify-written by every launch)
  if (part == 0 && b->ev_last_valid && stream != b->last_stream && !(p.use_lanes && p.batch_stream) && wait_for_last(b, stream) != 0) return -1;
  if (part == 0 && !p.use_lanes) {
    if (flush(b, stream) != 0) return -1;
    if (apply_resets(b, stream) != 0) return -1;
  }
  return 1;
}
// Everything else that is decided in front of the first launch, from the flushed schedule; the buffers a form needs are reserved here (a form whose buffers cannot
// be had steps aside).
int plan_launches(asdr_batch *b, CallPlan &p) {
  const int n_blocks = p.n_blocks, parts = p.parts;
  // Timing markers are opt-in: every event record is a packet the GPU's command processor handles between two kernels (tools/launch_gap.py: 0.134 ms per
  // back-to-back C2 call with a pair per call, 0.127 ms without).
  p.e0 = p.e1 = nullptr;
  if (parts == 1 && b->tev_used + 2 <= b->tev.size()) { p.e0 = b->tev[b->tev_used]; p.e1 = b->tev[b->tev_used + 1]; b->tev_used += 2; }
  else if (b->time_calls) { p.e0 = b->ev0; p.e1 = b->ev1; }   // (around all parts of a call)
  // Up to seven sub-ranges of the sorted schedule (the whole waves of 5 kernel kinds, the fused SAM kernel's general waves, the remainders).  They touch disjoint
  // channels, so they run CONCURRENTLY: the first on the caller's stream, the others on the batch's helper streams, forked behind an event and joined before the
  // call's end marker -- launched back to back on one stream the short ones (a handful of waves of the slowest instantiation) would each add a whole wave lifetime
  // to the step.  Heaviest instantiation first.
  static const int heaviest_first[ASDR_KERNEL_KINDS] = {ASDR_KERNEL_ALS, ASDR_KERNEL_SAM_ALS, ASDR_KERNEL_ALS_SMALL, ASDR_KERNEL_SAM, ASDR_KERNEL_PLAIN};
  Sub *const subs = p.subs; int &n_sub = p.n_sub = 0;
  if (b->left_slots > 0) subs[n_sub++] = Sub{b->left_kind, 0, b->left_first, b->left_slots};   // a few long-lived waves: started first
  for (int kk = 0; kk < ASDR_KERNEL_KINDS; kk++) {
    const int k = heaviest_first[kk];
    if (b->kind_slots[k] == 0) continue;
    const int nu = b->kind_uniform_slots[k], nm = b->kind_slots[k] - nu;
    if (nu > 0) subs[n_sub++] = Sub{k, 1, b->kind_first[k], nu};
    if (nm > 0) subs[n_sub++] = Sub{k, 0, b->kind_first[k] + nu, nm};
  }
  int total_slots = 0;
  for (int i = 0; i < n_sub; i++) total_slots += subs[i].slots;
  // SAM channels (no ALS) run as three launches per block -- everything in front of the PLL | the PLL with one LANE per channel | everything behind it -- through a
  // 1 KB-per-slot exchange buffer: as a phase of one fused kernel the PLL's 128-step dependent chain kept a workgroup's other waves waiting (ASDR_SAM_FUSED=1
  // selects that kernel, for comparison).
  const int sam_slots = b->kind_slots[ASDR_KERNEL_SAM] + b->kind_slots[ASDR_KERNEL_SAM_ALS];
  p.sam_split = b->sam_split && sam_slots > 0;
  if (p.sam_split && !reserve_tiles(b->d_xch_sam, b->xch_sam_slots, sam_slots, 2, p.stream)) return fail("SAM exchange tiles: out of device memory");
  // ... and channels with a short ALS filter as two: the chain up to the AGC | the filter and the output stage (stage taps off: the taps of the last two stages are
  // the fused kernel's)
  p.als_split = b->als_split && !b->taps_on && b->kind_uniform_slots[ASDR_KERNEL_ALS_SMALL] > 0;
  const bool io_alias = rows_overlap(b, p);
  // ALS role streams (asdr_batch::d_als_stage): the whole schedule is ONE uniform sub-range of short-filter channels of a known mode, small enough to be on the
  // in-kernel block loop otherwise; not for in-place calls (the filter of a chunk writes output rows while the chain of the next one reads input rows), not with
  // stage taps.
  bool als_roles = b->als_role_streams && n_blocks >= 2 && parts == 1 && !p.use_lanes && !b->taps_on && !p.sam_split && !p.als_split && n_sub == 1 &&
                   subs[0].kind == ASDR_KERNEL_ALS_SMALL && subs[0].uniform && total_slots <= 8 * ASDR_ALS_ROLE_MAX_WAVES &&
                   b->sched[subs[0].first].mode <= 6u && !io_alias;
  if (als_roles && !b->d_als_stage) {   // first use (a failed allocation leaves the batch on the block loop)
    float *st = nullptr;
    if (hipMalloc(&st, (size_t)(b->n + 1) * ASDR_ALS_STAGE_SLOTS * ASDR_N * sizeof(float)) == hipSuccess) b->d_als_stage = st; else { (void)hipGetLastError(); als_roles = false; }
  }
  // A multi-block call on a LARGE batch is issued as one launch per block: only the first block of a launch can read the local-oscillator cache (wave 0 leaves the
  // next LAUNCH's pairs), launches of >= 1024 waves follow each other without a gap (tools/launch_gap.py), and C2 x 64 blocks ran at 0.157 ms per block inside one
  // launch against 0.129 ms as 64 launches.  Small batches (C5: 64 waves, 646 blocks) keep the in-kernel block loop: there a launch per 19-us block would be all
  // overhead.
  p.per_block = n_blocks > 1 && (p.sam_split || p.als_split || total_slots >= 8 * ASDR_PER_BLOCK_LAUNCH_WAVES); p.n_launch = p.per_block ? n_blocks : 1;
  // Small batch, many blocks, one sub-range of uniform SSB-class waves, no taps: the block pipeline -- as a transaction: a snapshot of the state in front of it,
  // and behind it the launches that put the state back and run the call on the in-kernel block loop if a role's bounded wait fired (asdr_kernels.hip).  3 w + 1
  // workgroups must be co-resident: w <= stream_max_waves (occupancy query at asdr_create, at most one workgroup per compute unit).
  // The transaction restores channel STATE, not the caller's buffers: when the output rows alias an input row (the reference's own convention -- blockI is
  // overwritten, AudioSDR.cpp:158-165) role 3 has overwritten input blocks by the time a wait runs out and the re-run would read them.  Such calls keep the
  // in-kernel block loop, which is in-place safe.
  // The pipeline takes the plain kind's uniform waves (SSB-class and AM groups).  What else the schedule holds -- the remainders' general waves, a few SAM or ALS
  // channels among 4,000 receivers -- no longer disqualifies the call (round 3: n_sub == 1): while those sub-ranges are small they run the same call on the
  // in-kernel block loop beside the pipeline, on helper streams.
  p.pipe_sub = -1; p.other_waves = 0;
  for (int i = 0; i < n_sub; i++) { if (subs[i].kind == ASDR_KERNEL_PLAIN && subs[i].uniform) p.pipe_sub = i; else p.other_waves += subs[i].slots / 8; }
  p.take_pipeline = parts == 1 && b->stream_pipeline && !io_alias && n_blocks >= ASDR_STREAM_MIN_BLOCKS && p.pipe_sub >= 0 && b->plain_uniform_ssb &&
                    p.other_waves <= ASDR_STREAM_SIDE_WAVES && !p.sam_split && !p.als_split &&
#ifndef ASDR_TIMELINE   /* (the profiling build writes its timestamps through the taps buffer: tools/timeline.py stream) */
                    !b->taps_on &&
#endif
                    subs[p.pipe_sub].slots / 8 <= b->stream_max_waves;
  // All 3 w pipeline workgroups must be RESIDENT together (the roles wait for each other).  The sub-ranges beside the pipeline are long-running kernels on helper
  // streams started at the same fork: every one of their waves may hold a slot a role-3 workgroup needs (then roles 1 and 2 spin out their polls and the call is
  // re-run from the snapshot: exact, but several times slower).  With side waves the pipeline therefore keeps headroom for them plus a margin; alone it may fill
  // the device.
  if (p.take_pipeline && p.other_waves > 0 && b->stream_cap_workgroups > 0 &&
      3 * (subs[p.pipe_sub].slots / 8) + p.other_waves + ASDR_STREAM_SIDE_MARGIN > b->stream_cap_workgroups) { p.take_pipeline = false; b->stat_stream_headroom_refusals++; }
  if (p.take_pipeline && !reserve_pipeline(b, p.stream)) p.take_pipeline = false;
  p.n_items = 0; p.main_item = 0; p.sam_roles = p.sam_chunks = p.als_roles = false; p.n_chunks = 0;
  if (p.take_pipeline || p.use_lanes) return 0;
  // This part's waves of every sub-range, as launch items.  A large item is cut into `launch_split` pieces on as many streams (asdr_set_launch_split): kernels of
  // one stream run one after the other, each draining its last waves before the next starts; pieces on different streams fill each other's tails.
  Item *const items = p.items; int &n_items = p.n_items;
  for (int i = 0; i < n_sub; i++) {
    const long w = subs[i].slots / 8;
    const int lo = (int)(w * p.part / parts) * 8, cnt = (int)(w * (p.part + 1) / parts) * 8 - lo;
    if (cnt == 0) continue;
    int pieces = 1;
    if (b->launch_split > 1 && cnt / 8 >= b->launch_split_min_waves) pieces = std::min(b->launch_split, ASDR_AUX_STREAMS + 1 - n_items - (n_sub - 1 - i));
    if (pieces < 1) pieces = 1;
    for (int q = 0; q < pieces; q++) {
      const int qlo = (int)((long)(cnt / 8) * q / pieces) * 8, qhi = (int)((long)(cnt / 8) * (q + 1) / pieces) * 8;
      if (qhi > qlo && n_items < ASDR_AUX_STREAMS + 1) items[n_items++] = Item{i, subs[i].first + lo + qlo, qhi - qlo};
    }
  }
  // The largest item runs on the caller's stream: back-to-back calls then follow each other there without a gap, the helper streams' joins (shorter kernels) are
  // already satisfied when it ends, and only their starts pay the fork event's latency (C4: 28 us per call with the remainders' launch on the caller's stream).
  for (int i = 1; i < n_items; i++) if (items[i].slots > items[p.main_item].slots) p.main_item = i;
  const bool taps = b->taps_on && b->d_taps != nullptr;
  // SAM role streams (launch_items): a multi-block call whose schedule is ONE sub-range of SAM channels run as three launches ...
  p.sam_roles = b->sam_role_streams && p.per_block && p.n_launch >= 2 && parts == 1 && n_items == 1 && !taps && p.sam_split &&
                (subs[items[0].sub].kind == ASDR_KERNEL_SAM || subs[items[0].sub].kind == ASDR_KERNEL_SAM_ALS);
  // ... in chunks when the sub-range is uniform, plain SAM (no ALS) and small: see asdr_batch::d_xch_sam_chunk
  p.sam_chunks = p.sam_roles && b->sam_chunks && subs[items[0].sub].kind == ASDR_KERNEL_SAM && subs[items[0].sub].uniform && n_blocks >= 2 * ASDR_SAM_CHUNK &&
                 items[0].slots <= 8 * ASDR_SAM_CHUNK_MAX_WAVES;
  p.als_roles = als_roles && n_items == 1 && !taps;
  static_assert(ASDR_SAM_CHUNK == ASDR_ALS_CHUNK, "the two chunked forms share the tile sets");
  p.n_chunks = (n_blocks + ASDR_SAM_CHUNK - 1) / ASDR_SAM_CHUNK;
  return 0;
}
// The block pipeline, as a transaction, with the other sub-ranges beside it on helper streams.
int launch_pipeline(asdr_batch *b, const CallPlan &p, UpdateArgs &a) {
  hipStream_t stream = p.stream;
  const Sub &ps = p.subs[p.pipe_sub];
  const UpdateArgs a_side = a;   // (for the sub-ranges beside the pipeline: before the pipeline's own fields are set)
  const int w = ps.slots / 8;
  HIPCHK(hipMemsetAsync(b->d_stream_prog, 0, (size_t)(3 * w + 1) * sizeof(uint32_t), stream));   // stream-ordered behind the previous launch
  if (p.n_sub > 1) HIPCHK(hipEventRecord(b->ev_fork, stream));
  select_slots(b, a, ps, ps.first, ps.slots, false);
  a.lo_write = 0u;   // (the pipeline's oscillator role serves its own ring)
  a.xch_a = b->d_xch_a; a.xch_b = b->d_xch_b; a.xch_c = b->d_xch_b + (size_t)(b->n + 1) * ASDR_STREAM_DEPTH * ASDR_N; a.stream_prog = b->d_stream_prog; a.stream_err = b->d_stream_prog + 3 * ((b->n + 7) / 8) + 1;
  a.stream_waves = w; a.lo_ring = b->d_lo_ring; a.stream_spin_limit = b->stream_spin_limit;
  if (p.e0) HIPCHK(hipEventRecord(p.e0, stream));
  if (asdr_launch_stream_snapshot(&a, b->d_stream_snap, 0, stream) != 0) return fail("stream snapshot launch failed");
  // three FIR helper waves per role-2 workgroup while every pipeline workgroup has a compute unit to itself (and the residency arithmetic of plan_launches holds
  // for the 256-thread form too); otherwise the two-wave form
  const bool h3 = b->stream_h3 != 0 && b->stream_cap_h3 > 0 && 3 * w + p.other_waves + ASDR_STREAM_SIDE_MARGIN <= b->stream_cap_h3 &&
                  (b->stream_h3 == 1 || 3 * w <= b->stream_cus);
  if (h3) b->stat_stream_h3_calls++;
  if (asdr_launch_stream(&a, stream, h3 ? 3 : 1) != 0) return fail("stream kernel launch failed");
  if (asdr_launch_stream_snapshot(&a, b->d_stream_snap, 1, stream) != 0) return fail("stream restore launch failed");
  UpdateArgs f = a;   // the same call on the in-kernel block loop, gated on the error word: its waves return at once when the pipeline completed
  f.run_if = a.stream_err; f.stream_waves = 0; f.xch_a = nullptr; f.xch_b = nullptr; f.xch_c = nullptr; f.stream_prog = nullptr; f.lo_ring = nullptr;
  if (asdr_launch_update(&f, ASDR_KERNEL_PLAIN, 1, stream) != 0) return fail("stream fallback launch failed");
  if (asdr_launch_stream_ack(a.stream_err, stream) != 0) return fail("stream acknowledge launch failed");
  int n_aux = 0;   // the other sub-ranges: the whole call on the in-kernel block loop, each on a helper stream beside the pipeline
  for (int i = 0; i < p.n_sub; i++) {
    if (i == p.pipe_sub) continue;
    hipStream_t s = aux_stream(b, n_aux++);
    if (!s) return fail("stream creation failed");
    HIPCHK(hipStreamWaitEvent(s, b->ev_fork, 0));
    UpdateArgs o = a_side;
    select_slots(b, o, p.subs[i], p.subs[i].first, p.subs[i].slots, false);
    if (asdr_launch_update(&o, p.subs[i].kind, p.subs[i].uniform, s) != 0) return fail("update kernel launch failed");
    HIPCHK(hipEventRecord(b->ev_join[n_aux - 1], s));
  }
  for (int j = 0; j < n_aux; j++) HIPCHK(hipStreamWaitEvent(stream, b->ev_join[j], 0));
  b->stream_launched = true; b->stat_stream_launches++;
  return end_call(b, p, 1, p.n_blocks, false);   // (one launch, which counts its blocks for the alternating order)
}
// The lanes: every uniform sub-range cut into sched_lanes pieces on as many never-joined streams, the general-kernel sub-ranges (the remainders: a few long-lived
// waves) whole on the stream behind them.
int launch_lanes(asdr_batch *b, const CallPlan &p, const UpdateArgs &a) {
  // fork: the lanes start behind the previous ordinary call (ASDR_STREAM_BATCH) / behind everything on the caller's stream so far
  hipEvent_t ev = p.batch_stream ? b->ev_last : b->ev_fork;
  if (!p.batch_stream || (b->ev_last_valid && !b->last_was_lanes)) {
    HIPCHK(hipEventRecord(ev, p.batch_stream ? b->last_stream : p.stream));
    if (lanes_fork(b, ev) != 0) return -1;
  }
  const int NL = b->sched_lanes;
  for (int l = 0; l <= NL; l++) {   // l == NL: the sub-ranges that are not cut, on the stream behind the lanes (lane[ASDR_LANES])
    hipStream_t ls = lane_stream(b, (l == NL) ? ASDR_LANES : l);
    if (!ls) return fail("stream creation failed");
    for (int lb = 0; lb < p.n_launch; lb++) {
      for (int i = 0; i < p.n_sub; i++) {   // this lane's piece of every uniform sub-range, one kernel after the other on the lane's stream
        const Sub &su = p.subs[i];
        const long w = su.slots / 8;
        int lo = (int)(w * l / NL) * 8, cnt = (int)(w * (l + 1) / NL) * 8 - lo;
        if (l == NL) { lo = 0; cnt = su.uniform ? 0 : su.slots; } else if (!su.uniform) cnt = 0;
        if (cnt == 0) continue;
        UpdateArgs al = a;
        select_slots(b, al, su, su.first + lo, cnt, true);
        al.lo_cache = b->d_lo + (size_t)(1 + (l % ASDR_LANES)) * 2 * ASDR_LO_ENTRIES;   // this lane's own set: its writers fill it, its waves read it (general-kernel waves have no entry)
        al.lo_writer_bit = ASDR_LO_WRITER_LANE(l % ASDR_LANES);   // (lane 0: ASDR_LO_WRITER; a direct launch: its wave 0, under any name)
        if (p.sam_split && (su.kind == ASDR_KERNEL_SAM || su.kind == ASDR_KERNEL_SAM_ALS)) set_sam_rows(b, al, su.kind, su.first + lo, 0);
        const int form = (p.als_split && su.kind == ASDR_KERNEL_ALS_SMALL && su.uniform) ? 2 : su.uniform;
        if (p.per_block) point_at_blocks(b, p, al, lb, 1, lb);
        al.wg_reverse = order_bit(b, p, su, al.direct_ch0, p.per_block ? lb : 0);   // (a lane reverses within its own piece)
        int rev = 0;
        if (asdr_launch_update_ordered(&al, su.kind, form, ls, &rev) != 0) return fail("update kernel launch failed");
        b->stat_reversed_launches += rev;
      }
    }
  }
  if (!p.batch_stream && lanes_join_into(b, p.stream) != 0) return -1;   // a strict call joins at its end; on ASDR_STREAM_BATCH the lanes stay pending
  b->stat_lane_calls++;
  return end_call(b, p, p.n_launch, p.n_launch, p.batch_stream);
}
// SAM role streams, the fork: the helper streams of the pre and PLL roles behind the caller's stream (both forms below start from it)
int fork_sam_roles(asdr_batch *b, const CallPlan &p, hipStream_t &s_pre, hipStream_t &s_pll) {
  s_pre = aux_stream(b, 0); s_pll = aux_stream(b, 1);
  if (!s_pre || !s_pll) return fail("stream creation failed");
  for (int i = 0; i < 6; i++) if (!b->ev_role[i]) HIPCHK(hipEventCreateWithFlags(&b->ev_role[i], hipEventDisableTiming));
  HIPCHK(hipEventRecord(b->ev_fork, p.stream)); HIPCHK(hipStreamWaitEvent(s_pre, b->ev_fork, 0)); HIPCHK(hipStreamWaitEvent(s_pll, b->ev_fork, 0));
  b->stat_sam_role_calls++;
  return 0;
}
// SAM role streams in chunks (asdr_batch::d_xch_sam_chunk): pre | PLL | post launches of ASDR_SAM_CHUNK blocks each. TWO streams: the pre and post roles share the
// caller's stream -- pre(k + 1), then post(k) -- and the PLL has the helper stream to itself: its 32 us per block bound the call either way (pre + post are ~24),
// and a third stream is one too many for a process whose caller has a stream of its own (HIP's four hardware queues: 49 instead of 37 us per block measured with
// three, asdr.h "what the lanes rest on"). Tile sets: pre(k) overwrites those of chunk k - R, whose post role is earlier in the same stream.
int launch_sam_chunks(asdr_batch *b, const CallPlan &p, UpdateArgs &a, hipStream_t s_pll) {
  constexpr int S = ASDR_SAM_CHUNK_SETS, G = ASDR_SAM_CHUNK, R = S / G;
  static_assert(S % G == 0 && R >= 4, "tile sets for four chunks");
  hipStream_t stream = p.stream;
  for (int i = 0; i < 3 * R; i++) if (!b->ev_samc[i]) HIPCHK(hipEventCreateWithFlags(&b->ev_samc[i], hipEventDisableTiming));
  select_slots(b, a, p.subs[p.items[0].sub], p.items[0].first, p.items[0].slots, false);
  set_chunk_tiles(b, a);
  a.taps = nullptr;
  auto chunk_args = [&](int k) { point_at_blocks(b, p, a, k * G, std::min(G, p.n_blocks - k * G), k); a.sam_set = (uint32_t)(k * G % S); };
  for (int k = 0; k <= p.n_chunks; k++) {
    if (k < p.n_chunks) {
      const int kr = k % R;
      chunk_args(k);
      if (asdr_launch_sam_role(&a, ASDR_KERNEL_SAM, 1, 0, stream) != 0) return fail("update kernel launch failed");
      HIPCHK(hipEventRecord(b->ev_samc[kr], stream)); HIPCHK(hipStreamWaitEvent(s_pll, b->ev_samc[kr], 0));
      if (asdr_launch_sam_role(&a, ASDR_KERNEL_SAM, 1, 1, s_pll) != 0) return fail("update kernel launch failed");
      HIPCHK(hipEventRecord(b->ev_samc[R + kr], s_pll));
    }
    if (k >= 1) {
      chunk_args(k - 1);
      HIPCHK(hipStreamWaitEvent(stream, b->ev_samc[R + (k - 1) % R], 0));
      if (asdr_launch_sam_role(&a, ASDR_KERNEL_SAM, 1, 2, stream) != 0) return fail("update kernel launch failed");
    }
  }
  b->stat_sam_chunk_calls++;
  return 0;
}
// ALS role streams: chunks of ASDR_ALS_CHUNK blocks -- the chain up to the AGC (its block loop kept) on the helper stream, the filter + output on the caller's,
// chained by one event pair per chunk.  The chain's rows wait in the stage (slot = block % S); chain chunk k overwrites the slots filter chunk k - S / G + 1 reads
// its "previous block" from, so it waits for that launch -- the only back-pressure.  The two launches touch disjoint rows otherwise (the chain: filter states,
// rings, status; the filter: taps, output, the kept audio row).
int launch_als_roles(asdr_batch *b, const CallPlan &p, UpdateArgs &a) {
  constexpr int S = ASDR_ALS_STAGE_SLOTS, G = ASDR_ALS_CHUNK, R = S / G;
  static_assert(S % G == 0 && R >= 3, "the stage holds at least three chunks");
  hipStream_t stream = p.stream, s_chain = aux_stream(b, 0);
  if (!s_chain) return fail("stream creation failed");
  for (int i = 0; i < 2 * R; i++) if (!b->ev_als[i]) HIPCHK(hipEventCreateWithFlags(&b->ev_als[i], hipEventDisableTiming));
  HIPCHK(hipEventRecord(b->ev_fork, stream)); HIPCHK(hipStreamWaitEvent(s_chain, b->ev_fork, 0));
  select_slots(b, a, p.subs[p.items[0].sub], p.items[0].first, p.items[0].slots, false);
  // the stage's "previous block" slot of the call's first block: the als_x ring's other slot as the last call left it
  a.als_stage = b->d_als_stage; a.als_stage_cur = 0u; a.als_stage_prev = (uint32_t)(S - 1); a.als_phase = b->als_phase;
  if (asdr_launch_als_stage_seed(&a, 0, b->n, s_chain) != 0) return fail("update kernel launch failed");
  // Three stages (default): the chain itself is cut where the SAM roles cut it -- front half (scale, blanker, IF band-pass: the looped SAM pre role, into tile
  // sets) | back half (mixer .. AGC, ROLE 10, from the tiles into the stage) | filter -- on three streams: the chain as ONE stage is 23 us per block for a lone
  // wave and bounds the two-stage form; its halves are ~11 and ~13, the filter 18.
  constexpr int RT = ASDR_SAM_CHUNK_SETS / G;
  static_assert(RT == R, "the front stage's wait indexes ev_als[(k - RT) % R]: the event of back chunk k - RT only while tile sets and stage slots hold the same number of chunks");
  hipStream_t s_front = nullptr;
  bool three = b->als_role_stages == 3 && reserve_chunk_tiles(b, p.items[0].slots, stream);
  if (three) { s_front = aux_stream(b, 1); if (!s_front) three = false; }
  if (three) {
    for (int i = 2 * R; i < 3 * R; i++) if (!b->ev_als[i]) HIPCHK(hipEventCreateWithFlags(&b->ev_als[i], hipEventDisableTiming));
    HIPCHK(hipStreamWaitEvent(s_front, b->ev_fork, 0));
    set_chunk_tiles(b, a);
  }
  for (int k = 0; k < p.n_chunks; k++) {
    const int b0 = k * G;
    point_at_blocks(b, p, a, b0, std::min(G, p.n_blocks - b0), k);
    a.als_stage_cur = (uint32_t)(b0 % S); a.als_stage_prev = (uint32_t)((b0 + S - 1) % S);
    a.sam_set = (uint32_t)(b0 % ASDR_SAM_CHUNK_SETS);
    if (three) {   // front(k) writes the tile sets back(k - RT) read
      if (k >= RT) HIPCHK(hipStreamWaitEvent(s_front, b->ev_als[(k - RT) % R], 0));
      if (asdr_launch_als_role(&a, 2, s_front) != 0) return fail("update kernel launch failed");
      HIPCHK(hipEventRecord(b->ev_als[2 * R + k % R], s_front)); HIPCHK(hipStreamWaitEvent(s_chain, b->ev_als[2 * R + k % R], 0));
    }
    if (k >= R - 1) HIPCHK(hipStreamWaitEvent(s_chain, b->ev_als[R + (k + 1) % R], 0));
    if (asdr_launch_als_role(&a, three ? 3 : 0, s_chain) != 0) return fail("update kernel launch failed");
    HIPCHK(hipEventRecord(b->ev_als[k % R], s_chain)); HIPCHK(hipStreamWaitEvent(stream, b->ev_als[k % R], 0));
    if (asdr_launch_als_role(&a, 1, stream) != 0) return fail("update kernel launch failed");
    HIPCHK(hipEventRecord(b->ev_als[R + k % R], stream));
  }
  b->stat_als_role_calls++;
  return 0;
}
// The item loop: the part's items side by side -- the largest on the caller's stream, the others on helper streams, forked and joined -- once for the whole call
// (the in-kernel block loop) or once per block; a lone SAM item's blocks as role streams (s_pre, s_pll: fork_sam_roles).
int launch_items(asdr_batch *b, const CallPlan &p, UpdateArgs &a, hipStream_t s_pre, hipStream_t s_pll) {
  hipStream_t stream = p.stream;
  float *const taps = a.taps;
  for (int lb = 0; lb < p.n_launch; lb++) {
    if (p.per_block) {
      point_at_blocks(b, p, a, lb, 1, lb);
      a.taps = (lb == p.n_launch - 1) ? taps : nullptr;   // the taps are those of the call's last block
    }
    if (p.n_items > 1) HIPCHK(hipEventRecord(b->ev_fork, stream));
    int n_aux = 0;
    for (int it = 0; it < p.n_items; it++) {
      const Sub &su = p.subs[p.items[it].sub]; const int first = p.items[it].first;
      hipStream_t s = (it == p.main_item) ? stream : aux_stream(b, n_aux++);
      if (!s && it != p.main_item) return fail("stream creation failed");
      if (it != p.main_item) HIPCHK(hipStreamWaitEvent(s, b->ev_fork, 0));
      select_slots(b, a, su, first, p.items[it].slots, false);
      a.wg_reverse = order_bit(b, p, su, a.direct_ch0, p.per_block ? lb : 0);   // (a piece of a split launch reverses within itself)
      const bool sam3 = p.sam_split && (su.kind == ASDR_KERNEL_SAM || su.kind == ASDR_KERNEL_SAM_ALS);
      if (sam3) set_sam_rows(b, a, su.kind, first, p.sam_roles ? (lb & 1) : 0);   // this sub-range's tiles (1 KB per slot, 8 slots per tile) and lock words
      const int form = (p.als_split && su.kind == ASDR_KERNEL_ALS_SMALL && su.uniform) ? 2 : su.uniform;
      if (p.sam_roles) {
        // SAM role streams: block lb's pre | PLL | post on three streams, chained by events, so that pre(lb + 1) and PLL(lb + 1) run beside post(lb) -- the PLL's
        // 128-step chain per block (~32 us for any bank size) then bounds the call alone instead of adding to the other two roles.  The roles of a block touch
        // disjoint state (as the block pipeline's: status bits by atomics, the lock flag beside the tiles), the tiles alternate between two sets, and pre(lb + 2)
        // waits for post(lb) to have left its set.
        const int pa = lb & 1;
        if (lb >= 2) HIPCHK(hipStreamWaitEvent(s_pre, b->ev_role[4 + pa], 0));
        if (asdr_launch_sam_role(&a, su.kind, form, 0, s_pre) != 0) return fail("update kernel launch failed");
        HIPCHK(hipEventRecord(b->ev_role[pa], s_pre)); HIPCHK(hipStreamWaitEvent(s_pll, b->ev_role[pa], 0));
        if (asdr_launch_sam_role(&a, su.kind, form, 1, s_pll) != 0) return fail("update kernel launch failed");
        HIPCHK(hipEventRecord(b->ev_role[2 + pa], s_pll)); HIPCHK(hipStreamWaitEvent(stream, b->ev_role[2 + pa], 0));
        if (asdr_launch_sam_role(&a, su.kind, form, 2, stream) != 0) return fail("update kernel launch failed");
        HIPCHK(hipEventRecord(b->ev_role[4 + pa], stream));
        continue;
      }
      int rev = 0;
      if (asdr_launch_update_ordered(&a, su.kind, form, s, &rev) != 0) return fail("update kernel launch failed");
      b->stat_reversed_launches += rev;
      if (it != p.main_item) HIPCHK(hipEventRecord(b->ev_join[n_aux - 1], s));
    }
    for (int j = 0; j < n_aux; j++) HIPCHK(hipStreamWaitEvent(stream, b->ev_join[j], 0));   // behind the caller's stream's own launch
  }
  return 0;
}
}  // namespace
static int update_device_part(asdr_batch_t *b, const int16_t *dI, const int16_t *dQ, int16_t *dOut, int n_blocks,
                              long in_stride_blocks, long out_stride_blocks, void *stream_, int part, int parts) {
  CallPlan p;
  const int go = plan_enter(b, p, dI, dQ, dOut, n_blocks, in_stride_blocks, out_stride_blocks, stream_, part, parts);
  if (go <= 0) return go;
  if (plan_launches(b, p) != 0) return -1;
  UpdateArgs a;
  fill_args(b, a);
  a.in_i = dI; a.in_q = dQ; a.out = dOut; a.n_blocks = n_blocks; a.in_stride = (int32_t)in_stride_blocks; a.out_stride = (int32_t)out_stride_blocks;
  a.xch_sam = p.sam_split ? b->d_xch_sam : nullptr;
  a.sam_lock = p.sam_split ? reinterpret_cast<uint32_t *>(b->d_xch_sam + 2 * b->xch_sam_slots * 2 * ASDR_N) : nullptr;
  if (p.take_pipeline) return launch_pipeline(b, p, a);
  if (p.e0 && part == 0) HIPCHK(hipEventRecord(p.e0, p.stream));   // timing marker: right before the first launch
  if (p.use_lanes) return launch_lanes(b, p, a);
  hipStream_t s_pre = nullptr, s_pll = nullptr;
  if (p.sam_roles && fork_sam_roles(b, p, s_pre, s_pll) != 0) return -1;
  int lo_flips = p.n_launch;   // launches that flip the oscillator cache's halves: the chunked forms flip once per chunk
  if (p.sam_chunks && reserve_chunk_tiles(b, p.items[0].slots, p.stream)) { if (launch_sam_chunks(b, p, a, s_pll) != 0) return -1; lo_flips = p.n_chunks; }
  else if (p.als_roles) { if (launch_als_roles(b, p, a) != 0) return -1; lo_flips = p.n_chunks; }
  else if (launch_items(b, p, a, s_pre, s_pll) != 0) return -1;
  if (part + 1 < parts) return 0;   // the block counters advance with the call's last part
  return end_call(b, p, lo_flips, p.n_launch, false);
}

extern "C" {
int asdr_update_device_strided(asdr_batch_t *b, const int16_t *dI, const int16_t *dQ, int16_t *dOut, int n_blocks,
                               long in_stride_blocks, long out_stride_blocks, void *stream_) {
  if (is_sharded(b)) {
    // Device pointers belong to ONE device: a sharded batch takes them here only while all its shards live on that device (shards
    // as independent sub-batches of one GPU: tests, or several schedules side by side); shard g then works on its rows of the
    // caller's arrays.  Shards on several devices are driven through asdr_update (host rows) or shard by shard: asdr_shard().
    if (!dI || !dQ) return 0;
    if (!dOut) return fail("null output");
    for (asdr_batch *sh : b->shards) if (sh->device != b->shards[0]->device || sh->device == ASDR_NO_DEVICE)
      return fail("sharded batch over several devices: device pointers go to the shards (asdr_shard), host rows to asdr_update");
    for (size_t g = 0; g < b->shards.size(); g++) {
      const size_t f = (size_t)b->shard_first[g];
      if (update_device_part(b->shards[g], dI + f * (size_t)in_stride_blocks * ASDR_N, dQ + f * (size_t)in_stride_blocks * ASDR_N,
                             dOut + f * (size_t)out_stride_blocks * ASDR_N, n_blocks, in_stride_blocks, out_stride_blocks, stream_, 0, 1) != 0) return -1;
    }
    return 0;
  }
  return update_device_part(b, dI, dQ, dOut, n_blocks, in_stride_blocks, out_stride_blocks, stream_, 0, 1);
}

int asdr_update_device(asdr_batch_t *b, const int16_t *dI, const int16_t *dQ, int16_t *dOut, int n_blocks, void *stream_) {
  return asdr_update_device_strided(b, dI, dQ, dOut, n_blocks, n_blocks, n_blocks, stream_);
}

// ---- capture sink: each channel's audio appended to one contiguous HBM row ---------------
int asdr_capture_open(asdr_batch_t *b, long capacity_blocks) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_capture_open(sh_, capacity_blocks));   // one sink per shard, on the shard's device
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch (ASDR_NO_DEVICE): the capture sink lives in HBM");
  if (capacity_blocks <= 0 || capacity_blocks > 0x7fffffffL) return fail("bad capture capacity");
  HIPCHK(hipSetDevice(b->device));
  if (b->d_capture) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(b->d_capture)); b->d_capture = nullptr; }
  const size_t bytes = (size_t)b->n * (size_t)capacity_blocks * ASDR_N * sizeof(int16_t);
  if (hipMalloc(&b->d_capture, bytes) != hipSuccess) { b->d_capture = nullptr; return fail("capture sink: out of device memory"); }
  b->capture_cap = capacity_blocks; b->capture_pos = 0;
  return 0;
}

int asdr_capture_close(asdr_batch_t *b) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_capture_close(sh_));
  if (b->d_capture) { HIPCHK(hipSetDevice(b->device)); HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(b->d_capture)); }
  b->d_capture = nullptr; b->capture_cap = 0; b->capture_pos = 0;
  return 0;
}

long asdr_capture_capacity(const asdr_batch_t *b) { return b ? (is_sharded(b) ? b->shards[0]->capture_cap : b->capture_cap) : 0; }
long asdr_capture_position(const asdr_batch_t *b) { return b ? (is_sharded(b) ? b->shards[0]->capture_pos : b->capture_pos) : 0; }
int16_t *asdr_capture_device_ptr(asdr_batch_t *b) { return (b && !is_sharded(b)) ? b->d_capture : nullptr; }   // sharded: per shard, asdr_shard()
int asdr_capture_rewind(asdr_batch_t *b) { if (!b) return fail("null batch"); FOR_SHARDS(b, asdr_capture_rewind(sh_)); b->capture_pos = 0; return 0; }

int asdr_capture_update_device(asdr_batch_t *b, const int16_t *dI, const int16_t *dQ, int n_blocks, long in_stride_blocks, void *stream) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) {   // as asdr_update_device_strided: device pointers serve a sharded batch only while its shards share the device
    if (!dI || !dQ) return 0;
    for (asdr_batch *sh : b->shards) if (sh->device != b->shards[0]->device || sh->device == ASDR_NO_DEVICE)
      return fail("sharded batch over several devices: device pointers go to the shards (asdr_shard)");
    for (size_t g = 0; g < b->shards.size(); g++) {
      const size_t f = (size_t)b->shard_first[g] * (size_t)in_stride_blocks * ASDR_N;
      if (asdr_capture_update_device(b->shards[g], dI + f, dQ + f, n_blocks, in_stride_blocks, stream) != 0) return -1;
    }
    return 0;
  }
  if (!b->d_capture) return fail("capture sink is not open");
  if (!dI || !dQ) return 0;   // missing input: nothing is transmitted, nothing is appended (AudioSDR.cpp:48-56)
  if (n_blocks <= 0) return 0;
  if (b->capture_pos + n_blocks > b->capture_cap) return fail("capture sink overflow");
  int16_t *dst = b->d_capture + (size_t)b->capture_pos * ASDR_N;
  if (asdr_update_device_strided(b, dI, dQ, dst, n_blocks, in_stride_blocks, b->capture_cap, stream) != 0) return -1;
  b->capture_pos += n_blocks;
  return 0;
}

int asdr_capture_read(asdr_batch_t *b, int ch, long first_block, long n_blocks, int16_t *host_out) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) { asdr_batch *sh = shard_of(b, ch); if (!sh) return fail("bad channel"); return asdr_capture_read(sh, ch, first_block, n_blocks, host_out); }
  if (!b->d_capture) return fail("capture sink is not open");
  if (ch < 0 || ch >= b->n) return fail("bad channel");
  if (first_block < 0 || n_blocks < 0 || first_block + n_blocks > b->capture_pos) return fail("capture read beyond the write position");
  if (n_blocks == 0) return 0;
  if (!host_out) return fail("null output");
  HIPCHK(hipSetDevice(b->device));
  if (sync_all(b) != 0) return -1;
  HIPCHK(hipMemcpy(host_out, b->d_capture + ((size_t)ch * b->capture_cap + first_block) * ASDR_N,
                   (size_t)n_blocks * ASDR_N * sizeof(int16_t), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
// ---- the host-pointer entry point: overlapped ------------------------------------------------------------------------------
// asdr_update() replaces N x update() fed from host-resident audio blocks (AudioSDR.cpp:46-47 receiveWritable, :158-167 transmit):
// 768 bytes cross PCIe per channel-block (512 in, 256 out) and that, not the kernels, bounds the call -- 50 MB against 0.13 ms of
// kernel time for BASELINE config 2.  Round 3 ran H2D -> kernels -> D2H serially out of pageable memory.  Now the batch is cut into
// CHANNEL-RANGE chunks (state order within a channel is untouched) and three streams work on three chunks at once:
//     H2D(k + 1)  ||  kernels(k)  ||  D2H(k - 1)            (PCIe is full duplex: the two copy directions overlap too)
// The kernels of a call are launched as `parts` of every schedule sub-range (update_device_part); which part needs which input chunk,
// and which output chunk is complete after which part, is read off the host's copy of the schedule, so any settings mix is correct
// and a batch of one settings group (or of groups interleaved over the channel range) pipelines perfectly.
// Caller buffers that are pinned (asdr_host_alloc / asdr_host_register, or any hipHostMalloc'ed / registered memory) are DMA targets
// as they are; pageable buffers go through the batch's pinned staging area, copied by a few worker threads per chunk.
namespace {

// registered / hipHostMalloc'ed memory the DMA engines can address as it is -- the WHOLE range [p, p + bytes): its first and its last
// byte are both page-locked host memory (a buffer registered for less than the call's rows, or a view that runs past a pinned region,
// goes through the staging area like pageable memory)
bool is_pinned_host(const void *p, size_t bytes) {
  auto pinned_at = [](const void *q) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }   // ordinary pageable memory is an error here
    return at.type == hipMemoryTypeHost;
  };
  if (!pinned_at(p)) return false;
  return bytes <= 1 || pinned_at(static_cast<const char *>(p) + bytes - 1);
}

// Auto-pinning of recurring caller buffers (round 6).  The reference's boundary hands ordinary memory (AudioSDR.cpp:46-47,
// 158-167) and an application that reuses its buffers -- the usual case -- paid the staging copies in every call (1.4-2.5 ms per C2 call
// against 0.94 pinned).  A process-wide cache remembers the (address, length) of pageable ranges it has been handed; the SECOND time a range
// shows up it is registered in place (hipHostRegister, portable) and from then on hipPointerGetAttributes reports it pinned: the call
// DMA-copies straight from / into it.  One-shot buffers keep the staged path (and cost one table entry).  Bounded: at most
// ASDR_AUTOPIN_ENTRIES ranges / ASDR_AUTOPIN_BYTES bytes are kept registered, least recently used first out; everything is unregistered
// when the process' last batch is destroyed and by asdr_host_autopin_clear().
// OPT-IN (asdr_host_autopin(1) / ASDR_HOST_AUTOPIN=1), because of what was measured when it was on by default: a range that the application
// UNMAPS while the cache holds its registration (free() of a large malloc block is a munmap) and gets back at the same address is still
// reported page-locked by hipPointerGetAttributes, and the DMA through the stale registration ABORTS the process (ROCm 7.2, MI355X: the
// first form of tests/test_gpu_host_path.py test_a_freed_and_reallocated_buffer... did exactly that).  Nothing in user space tells the
// library that a range was unmapped, so pinning memory the caller may free cannot be made safe behind its back: an application that turns
// this on promises to call asdr_host_autopin_clear() (or destroy its batches) before it frees buffers it has passed in.  By default
// pageable buffers take the staged path in every call, freed-and-reallocated ones included (that test now holds THAT down).
#ifndef ASDR_AUTOPIN_ENTRIES
#define ASDR_AUTOPIN_ENTRIES 12
#endif
#ifndef ASDR_AUTOPIN_BYTES
#define ASDR_AUTOPIN_BYTES ((size_t)2 << 30)
#endif
struct AutoPin {
  struct Ent { const void *p; size_t bytes; unsigned long last_use; int seen; bool registered; int in_use; };   // in_use: asdr_update calls (other threads': shard workers, other batches) copying through the registration right now
  std::mutex m;
  std::vector<Ent> ents;
  unsigned long tick = 0;
  int enabled = -1;          // -1: read ASDR_HOST_AUTOPIN once (default OFF: see the hazard above)
  long stat_registered = 0, stat_evicted = 0, stat_failed = 0;
  int live_batches = 0;
  bool on() { if (enabled < 0) { const char *e = getenv("ASDR_HOST_AUTOPIN"); enabled = (e && atoi(e) != 0) ? 1 : 0; } return enabled != 0; }
  void drop(size_t i) {
    if (ents[i].registered) { if (hipHostUnregister(const_cast<void *>(ents[i].p)) != hipSuccess) (void)hipGetLastError(); stat_evicted++; }
    ents.erase(ents.begin() + (long)i);
  }
  void clear() { std::lock_guard<std::mutex> lk(m); for (size_t i = ents.size(); i-- > 0;) if (ents[i].in_use == 0) drop(i); }   // (a range a call is copying through stays until a later clear)
  // a call starts / has finished copying through the registration of (p, bytes): such a range is never evicted under it
  void hold(const void *p, size_t bytes, int d) {
    std::lock_guard<std::mutex> lk(m);
    for (Ent &e : ents) if (e.p == p && e.bytes == bytes && e.registered) { e.in_use += d; if (e.in_use < 0) e.in_use = 0; return; }
  }
  // a pageable range was handed to asdr_update: note it; true = it has just been registered (the caller re-reads its attributes)
  bool sighting(const void *p, size_t bytes) {
    std::lock_guard<std::mutex> lk(m);
    if (!on()) return false;
    tick++;
    for (size_t i = 0; i < ents.size(); i++) {
      Ent &e = ents[i];
      if (e.p == p && e.bytes == bytes) {
        e.last_use = tick; e.seen++;
        if (e.registered) return false;                      // (registered by us and still reported pageable: the registration is gone; stay on the staged path)
        if (e.seen < 2) return false;
        size_t total = bytes; int n_reg = 1;
        for (const Ent &o : ents) if (o.registered) { total += o.bytes; n_reg++; }
        while ((total > ASDR_AUTOPIN_BYTES || n_reg > ASDR_AUTOPIN_ENTRIES) && n_reg > 1) {   // make room: least recently used registered range out
          size_t lru = ents.size();
          for (size_t k = 0; k < ents.size(); k++) if (ents[k].registered && ents[k].in_use == 0 && (lru == ents.size() || ents[k].last_use < ents[lru].last_use)) lru = k;
          if (lru == ents.size()) return false;   // (everything registered is being copied through right now: this range stays on the staged path)
          total -= ents[lru].bytes; n_reg--;
          drop(lru);
        }
        for (size_t k = 0; k < ents.size(); k++) if (ents[k].p == p && ents[k].bytes == bytes) {
          if (hipHostRegister(const_cast<void *>(p), bytes, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); stat_failed++; ents[k].seen = -(1 << 20); return false; }   // (never again for this range)
          ents[k].registered = true; stat_registered++;
          return true;
        }
        return false;
      }
      // an entry that overlaps this range without being it: the application's buffers have moved -- forget the old one
      const char *a0 = static_cast<const char *>(e.p), *a1 = a0 + e.bytes, *b0 = static_cast<const char *>(p), *b1 = b0 + bytes;
      if (a0 < b1 && b0 < a1 && e.in_use == 0) { drop(i); i--; }
    }
    if (ents.size() >= 4 * ASDR_AUTOPIN_ENTRIES) {   // the table itself is bounded: the oldest unregistered sighting goes
      size_t old = ents.size();
      for (size_t k = 0; k < ents.size(); k++) if (!ents[k].registered && (old == ents.size() || ents[k].last_use < ents[old].last_use)) old = k;
      if (old != ents.size()) drop(old);
    }
    ents.push_back(Ent{p, bytes, tick, 1, false, 0});
    return false;
  }
};
AutoPin g_autopin;
void autopin_batch_created() { std::lock_guard<std::mutex> lk(g_autopin.m); g_autopin.live_batches++; }
void autopin_batch_gone() {
  bool last;
  { std::lock_guard<std::mutex> lk(g_autopin.m); last = (--g_autopin.live_batches <= 0); if (last) g_autopin.live_batches = 0; }
  if (last) g_autopin.clear();
}

int host_parts(const asdr_batch *b, int n_blocks) {
  if (b->host_chunks_forced > 0) return std::min(b->host_chunks_forced, std::max(1, b->n / 8));
  const size_t row_bytes = (size_t)b->n * n_blocks * ASDR_N * sizeof(int16_t);   // one of I, Q, out
  long k = (long)(row_bytes / ((size_t)2 << 20));                              // about 2 MB of I per chunk ...
  k = std::min<long>(k, b->n / 2048);                                          // ... and at least 256 waves per part
  return (int)std::max<long>(1, std::min<long>(k, 16));
}

void build_host_plan(asdr_batch *b, HostPlan &hp, int K) {
  hp.K = K; hp.sched_gen = b->stat_sched_rebuilds;
  hp.bound.resize(K + 1);
  for (int j = 0; j <= K; j++) hp.bound[j] = (int)((long)b->n * j / K);
  hp.need_in.assign(K, 0); hp.last_part.assign(K, 0);
  auto chunk_of = [&](int ch) { int j = (int)((long)ch * K / b->n); while (j + 1 < K && ch >= hp.bound[j + 1]) j++; while (j > 0 && ch < hp.bound[j]) j--; return j; };
  auto sub = [&](int first, int slots) {
    const long w = slots / 8;
    for (int p = 0; p < K; p++) {
      const int lo = first + (int)(w * p / K) * 8, hi = first + (int)(w * (p + 1) / K) * 8;
      for (int sl = lo; sl < hi; sl++) {
        const int ch = b->sched[sl].ch;
        if (ch >= b->n) continue;   // padding
        const int j = chunk_of(ch);
        if (j > hp.need_in[p]) hp.need_in[p] = j;
        if (p > hp.last_part[j]) hp.last_part[j] = p;
      }
    }
  };
  // the same sub-ranges update_device_part launches (uniform and general part of every kernel kind, the remainders)
  if (b->left_slots > 0) sub(b->left_first, b->left_slots);
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
    const int nu = b->kind_uniform_slots[k], nm = b->kind_slots[k] - nu;
    if (nu > 0) sub(b->kind_first[k], nu);
    if (nm > 0) sub(b->kind_first[k] + nu, nm);
  }
  for (int p = 1; p < K; p++) hp.need_in[p] = std::max(hp.need_in[p], hp.need_in[p - 1]);   // parts are enqueued in order on one stream
}

int host_update(asdr_batch *b, const int16_t *I, const int16_t *Q, int16_t *out, int n_blocks) {
  HIPCHK(hipSetDevice(b->device));
  const size_t count = (size_t)b->n * n_blocks * ASDR_N;
  if (count > b->io_cap) {
    HIPCHK(hipStreamSynchronize(b->stream));
    b->io_cap = 0;   // (a failure part-way leaves "no buffers", never pointers that disagree with the recorded capacity)
    for (int i = 0; i < 3; i++) {
      if (b->d_io[i]) HIPCHK(hipFree(b->d_io[i]));
      b->d_io[i] = nullptr;
    }
    for (int i = 0; i < 3; i++) HIPCHK(hipMalloc(&b->d_io[i], count * sizeof(int16_t)));
    b->io_cap = count;
  }
  const size_t row_bytes_all = count * sizeof(int16_t);
  bool pin_i = is_pinned_host(I, row_bytes_all), pin_q = is_pinned_host(Q, row_bytes_all), pin_o = is_pinned_host(out, row_bytes_all);
  // pageable ranges that recur are registered in place the second time they are seen (AutoPin above)
  if (!pin_i && g_autopin.sighting(I, row_bytes_all)) pin_i = is_pinned_host(I, row_bytes_all);
  if (!pin_q && g_autopin.sighting(Q, row_bytes_all)) pin_q = is_pinned_host(Q, row_bytes_all);
  if (!pin_o && g_autopin.sighting(out, row_bytes_all)) pin_o = is_pinned_host(out, row_bytes_all);
  const bool pinned = pin_i && pin_q && pin_o;
  // (ranges registered by AutoPin are held for the length of the call: another thread's registration must not evict them under the copies)
  struct PinHold {
    const void *p[3]; size_t bytes; bool on;
    ~PinHold() { if (on) for (int i = 0; i < 3; i++) g_autopin.hold(p[i], bytes, -1); }
  } pin_hold{{I, Q, out}, row_bytes_all, pinned};
  if (pinned) for (int i = 0; i < 3; i++) g_autopin.hold(pin_hold.p[i], row_bytes_all, +1);
  if (!pinned && count > b->h_io_cap) {   // the pinned staging area, one row set per call
    b->h_io_cap = 0;
    for (int i = 0; i < 3; i++) {
      if (b->h_io[i]) HIPCHK(hipHostFree(b->h_io[i]));
      b->h_io[i] = nullptr;
    }
    for (int i = 0; i < 3; i++) HIPCHK(hipHostMalloc((void **)&b->h_io[i], count * sizeof(int16_t), hipHostMallocPortable));
    b->h_io_cap = count;
  }
  if (!b->h2d_stream) {   // kernels on the pool's first stream (b->stream), copies in on its second, out on its third
    b->h2d_stream = pool_stream(b->device, 1); b->d2h_stream = pool_stream(b->device, 2);
    if (!b->h2d_stream || !b->d2h_stream) return fail("stream creation failed");
  }
  // Behind the lanes first: calls on ASDR_STREAM_BATCH may still be running on them, and what follows rewrites rows their kernels read
  // (the flush: parameters, schedule) and state they write (launch-form fuzz, seed 144: a setter, then this entry point, while lane 2 of a
  // nine-block call was still at block 3 -- its channel ran the rest of that call with the filter the setter had just enabled).
  if (leave_lanes(b, b->stream) != 0) return -1;
  // the schedule must exist before the plan can be read off it
  if (b->ev_last_valid && b->stream != b->last_stream) {
    HIPCHK(hipEventRecord(b->ev_last, b->last_stream));
    HIPCHK(hipStreamWaitEvent(b->stream, b->ev_last, 0));
    b->last_stream = b->stream;
  }
  if (flush(b, b->stream) != 0) return -1;
  const int K = host_parts(b, n_blocks);
  HostPlan &hp = b->host_plan;
  if (hp.K != K || hp.sched_gen != b->stat_sched_rebuilds || (int)hp.bound.size() != K + 1) build_host_plan(b, hp, K);
  while ((int)b->ev_host.size() < 3 * K) { hipEvent_t e; HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); b->ev_host.push_back(e); }
  hipEvent_t *ev_in = b->ev_host.data(), *ev_k = ev_in + K, *ev_out = ev_k + K;
  const size_t row = (size_t)n_blocks * ASDR_N;   // samples per channel row
  const int16_t *srcI = pinned ? I : b->h_io[0], *srcQ = pinned ? Q : b->h_io[1];
  int16_t *dstO = pinned ? out : b->h_io[2];
  std::unique_ptr<CopyPool::Job> job;
  if (!pinned) {
    if (!b->copy_pool) {
      const char *e = getenv("ASDR_HOST_COPY_THREADS");
      int nt = e ? atoi(e) : 4;
      b->copy_pool.reset(new CopyPool(std::max(1, std::min(nt, 32))));
    }
    job.reset(new CopyPool::Job(K, b->copy_pool->threads()));
    // slice s of S of chunk j: the channels [c0 + n s / S, c0 + n (s + 1) / S) of its range
    job->copy_in = [=, &hp](int j, int sl, int S) {
      const size_t c0 = (size_t)hp.bound[j], nc = (size_t)(hp.bound[j + 1] - hp.bound[j]);
      const size_t o = (c0 + nc * sl / S) * row, nsm = (nc * (sl + 1) / S - nc * sl / S) * row;
      memcpy(b->h_io[0] + o, I + o, nsm * sizeof(int16_t)); memcpy(b->h_io[1] + o, Q + o, nsm * sizeof(int16_t));
    };
    job->copy_out = [=, &hp](int j, int sl, int S) {
      const size_t c0 = (size_t)hp.bound[j], nc = (size_t)(hp.bound[j + 1] - hp.bound[j]);
      const size_t o = (c0 + nc * sl / S) * row, nsm = (nc * (sl + 1) / S - nc * sl / S) * row;
      memcpy(out + o, b->h_io[2] + o, nsm * sizeof(int16_t));
    };
    b->copy_pool->start(job.get());
  }
  // The workers must be through with the job before this frame (and the job) goes away, also on an error path.
  struct JobGuard {
    CopyPool::Job *j;
    ~JobGuard() {
      if (!j) return;
      for (int k = 0; k < j->n_chunks; k++) j->out_ready[k].store(1, std::memory_order_release);
      while (j->workers_left.load(std::memory_order_acquire) > 0) CopyPool::nap();
    }
  } guard{job.get()};
  int rc = 0;
  int next_part = 0, next_out = 0;
  for (int j = 0; j < K && rc == 0; j++) {
    const size_t o = (size_t)hp.bound[j] * row, nsm = (size_t)(hp.bound[j + 1] - hp.bound[j]) * row;
    if (job) while (job->in_done[j].load(std::memory_order_acquire) < job->slices) std::this_thread::yield();   // (the enqueuing thread is the one the DMA waits for: it may spin)
    HIPCHK(hipMemcpyAsync(b->d_io[0] + o, srcI + o, nsm * sizeof(int16_t), hipMemcpyHostToDevice, b->h2d_stream));
    HIPCHK(hipMemcpyAsync(b->d_io[1] + o, srcQ + o, nsm * sizeof(int16_t), hipMemcpyHostToDevice, b->h2d_stream));
    HIPCHK(hipEventRecord(ev_in[j], b->h2d_stream));
    // every kernel part whose channels have now arrived
    for (; next_part < K && hp.need_in[next_part] <= j; next_part++) {
      HIPCHK(hipStreamWaitEvent(b->stream, ev_in[hp.need_in[next_part]], 0));
      if (update_device_part(b, b->d_io[0], b->d_io[1], b->d_io[2], n_blocks, n_blocks, n_blocks, b->stream, next_part, K) != 0) { rc = -1; break; }
      HIPCHK(hipEventRecord(ev_k[next_part], b->stream));
    }
    // ... and every output chunk whose channels are all behind an enqueued part
    for (; rc == 0 && next_out < K && hp.last_part[next_out] < next_part; next_out++) {
      const size_t oo = (size_t)hp.bound[next_out] * row, no = (size_t)(hp.bound[next_out + 1] - hp.bound[next_out]) * row;
      HIPCHK(hipStreamWaitEvent(b->d2h_stream, ev_k[hp.last_part[next_out]], 0));
      HIPCHK(hipMemcpyAsync(dstO + oo, b->d_io[2] + oo, no * sizeof(int16_t), hipMemcpyDeviceToHost, b->d2h_stream));
      HIPCHK(hipEventRecord(ev_out[next_out], b->d2h_stream));
    }
  }
  if (rc != 0) return -1;
  if (next_part != K || next_out != K) return fail("host path: internal error (a part or an output chunk was never enqueued)");
  for (int j = 0; j < K; j++) {
    HIPCHK(hipEventSynchronize(ev_out[j]));
    if (job) job->out_ready[j].store(1, std::memory_order_release);
  }
  if (job) while (job->out_finished.load(std::memory_order_acquire) < K * job->slices) CopyPool::nap();
  HIPCHK(hipStreamSynchronize(b->stream));
  b->stat_host_chunks = K; b->stat_host_pinned = pinned ? 1 : 0;
  return check_stream_error(b);
}

// asdr_update on a sharded batch: shard g's rows [shard_first[g], shard_first[g + 1]) of I, Q and out go through shard g's own
// overlapped host path on its own device, one host thread per shard (the caller's thread takes shard 0); no collective, nothing
// crosses between devices.  Errors of the worker threads come back as the call's error text.
// The shard threads are PERSISTENT (round 5; round 4 created and joined G - 1 threads in every call): started at the first host-row call
// of the sharded batch, parked on a condition variable between calls, stopped by asdr_destroy.  The caller's thread runs shard 0 and
// gets its current device back before the call returns (asdr_update on a shard sets the shard's device).
struct ShardWorkers {
  struct Job { const int16_t *I = nullptr, *Q = nullptr; int16_t *out = nullptr; int n_blocks = 0; };
  asdr_batch *parent = nullptr;
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_go, cv_done;
  Job job;
  unsigned long gen = 0;          // a call publishes its job under a new generation
  size_t pending = 0;             // workers that have not finished the current generation
  bool stop = false;
  std::vector<int> rc;
  std::vector<std::string> err;
  static void run_shard(asdr_batch *parent, size_t g, const Job &j, int &rc, std::string &err) {
    const size_t o = (size_t)parent->shard_first[g] * (size_t)j.n_blocks * ASDR_N;
    rc = asdr_update(parent->shards[g], j.I + o, j.Q + o, j.out + o, j.n_blocks);
    if (rc != 0) err = g_err;     // (thread-local: copied out for the caller's thread)
  }
  void loop(size_t g) {
    unsigned long seen = 0;
    for (;;) {
      Job j;
      { std::unique_lock<std::mutex> lk(m);
        cv_go.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen; j = job; }
      int r = 0; std::string e;
      run_shard(parent, g, j, r, e);
      { std::lock_guard<std::mutex> lk(m); rc[g] = r; err[g] = e; if (--pending == 0) cv_done.notify_all(); }
    }
  }
  explicit ShardWorkers(asdr_batch *p) : parent(p), rc(p->shards.size(), 0), err(p->shards.size()) {
    for (size_t g = 1; g < p->shards.size(); g++) th.emplace_back([this, g] { loop(g); });
  }
  ~ShardWorkers() {
    { std::lock_guard<std::mutex> lk(m); stop = true; }
    cv_go.notify_all();
    for (std::thread &t : th) t.join();
  }
};
void shard_workers_stop(asdr_batch *b) { delete static_cast<ShardWorkers *>(b->workers); b->workers = nullptr; }

int sharded_update(asdr_batch *b, const int16_t *I, const int16_t *Q, int16_t *out, int n_blocks) {
  if (!I || !Q) return 0;   // missing-input guard, AudioSDR.cpp:48-56
  if (!out) return fail("null output");
  if (n_blocks <= 0) return 0;
  const size_t G = b->shards.size();
  if (!b->workers) b->workers = new ShardWorkers(b);
  ShardWorkers &w = *static_cast<ShardWorkers *>(b->workers);
  int dev0 = -1;
  const bool have_dev = hipGetDevice(&dev0) == hipSuccess;   // the caller's current device: shard 0's call below changes it
  if (!have_dev) (void)hipGetLastError();
  ShardWorkers::Job j; j.I = I; j.Q = Q; j.out = out; j.n_blocks = n_blocks;
  { std::lock_guard<std::mutex> lk(w.m); w.job = j; w.pending = G - 1; w.gen++; }
  w.cv_go.notify_all();
  ShardWorkers::run_shard(b, 0, j, w.rc[0], w.err[0]);
  { std::unique_lock<std::mutex> lk(w.m); w.cv_done.wait(lk, [&] { return w.pending == 0; }); }
  if (have_dev) (void)hipSetDevice(dev0);
  for (size_t g = 0; g < G; g++) if (w.rc[g] != 0) return fail("shard " + std::to_string(g) + ": " + w.err[g]);
  return 0;
}

}  // namespace

extern "C" {
int asdr_update(asdr_batch_t *b, const int16_t *I, const int16_t *Q, int16_t *out, int n_blocks) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) return sharded_update(b, I, Q, out, n_blocks);
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch (ASDR_NO_DEVICE): the signal path needs a HIP device");
  if (!I || !Q) return 0;   // missing-input guard, AudioSDR.cpp:48-56
  if (!out) return fail("null output");
  if (n_blocks <= 0) return 0;
  return host_update(b, I, Q, out, n_blocks);
}

void *asdr_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); fail("asdr_host_alloc: hipHostMalloc failed"); return nullptr; }
  return p;
}
void asdr_host_free(void *p) { if (p) (void)hipHostFree(p); }
int asdr_host_register(void *p, size_t bytes) {
  if (!p || !bytes) return fail("asdr_host_register: null buffer");
  HIPCHK(hipHostRegister(p, bytes, hipHostRegisterPortable));
  return 0;
}
int asdr_host_unregister(void *p) {
  if (!p) return fail("asdr_host_unregister: null buffer");
  HIPCHK(hipHostUnregister(p));
  return 0;
}
int asdr_set_pool_priority(int level) {   // 0 normal, 1 highest (default), 2 lowest; before the process' first batch
  if (level < 0 || level > 2) return fail("asdr_set_pool_priority: 0 = normal, 1 = highest, 2 = lowest");
  if (g_pool_created) return fail("asdr_set_pool_priority: the stream pool exists already (call it before the first asdr_create)");
  g_pool_priority = level;
  return 0;
}
int asdr_host_autopin(int on) { std::lock_guard<std::mutex> lk(g_autopin.m); const int was = g_autopin.on() ? 1 : 0; if (on >= 0) g_autopin.enabled = on ? 1 : 0; return was; }
void asdr_host_autopin_clear(void) { g_autopin.clear(); }
int asdr_host_autopin_info(long out[4]) {
  if (!out) return fail("null output");
  std::lock_guard<std::mutex> lk(g_autopin.m);
  long n_reg = 0; for (const AutoPin::Ent &e : g_autopin.ents) n_reg += e.registered ? 1 : 0;
  out[0] = n_reg; out[1] = g_autopin.stat_registered; out[2] = g_autopin.stat_evicted; out[3] = g_autopin.stat_failed;
  return 0;
}
int asdr_order_before(asdr_batch_t *b, void *stream_) {   // everything enqueued on `stream` from now on runs after the batch's calls so far
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_order_before(sh_, stream_));
  if (b->device == ASDR_NO_DEVICE) return 0;
  if (stream_ == ASDR_STREAM_BATCH) return fail("asdr_order_before: name one of your own streams");
  HIPCHK(hipSetDevice(b->device));
  hipStream_t stream = (hipStream_t)stream_;
  if (b->lanes_pending && lanes_join_into(b, stream) != 0) return -1;
  return (b->ev_last_valid && b->last_stream != stream && !b->last_was_lanes) ? wait_for_last(b, stream) : 0;
}
int asdr_order_after(asdr_batch_t *b, void *stream_) {   // the batch's calls on ASDR_STREAM_BATCH from now on run after everything enqueued on `stream` so far
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_order_after(sh_, stream_));
  if (b->device == ASDR_NO_DEVICE) return 0;
  if (stream_ == ASDR_STREAM_BATCH) return fail("asdr_order_after: name one of your own streams");
  HIPCHK(hipSetDevice(b->device));
  HIPCHK(hipEventRecord(b->ev_fork, (hipStream_t)stream_));
  for (int l = 0; l < ASDR_LANES + 1; l++) if (b->lane[l] || l < b->sched_lanes || l == ASDR_LANES) { hipStream_t ls = lane_stream(b, l); if (!ls) return fail("stream creation failed"); HIPCHK(hipStreamWaitEvent(ls, b->ev_fork, 0)); }
  HIPCHK(hipStreamWaitEvent(b->stream, b->ev_fork, 0));
  return 0;
}
int asdr_set_alternate_order(asdr_batch_t *b, int on) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) { for (asdr_batch *sh : b->shards) sh->alternate_order = on != 0; return 0; }
  b->alternate_order = on != 0;
  return 0;
}

long asdr_reversed_launches(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_reversed_launches; return t; }
  return b ? b->stat_reversed_launches : -1;
}

long asdr_lane_calls(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_lane_calls; return t; }
  return b ? b->stat_lane_calls : -1;
}
int asdr_lanes_overlap_probe(asdr_batch_t *b) {   // the last verdict of the probe on the batch's device (see lanes_overlap_probe; -1: no lane-sized call has probed yet)
  if (!b) return -1;
  if (is_sharded(b)) { int r = 1; for (asdr_batch *sh : b->shards) { const int v = asdr_lanes_overlap_probe(sh); if (v < r) r = v; } return r; }
  return (b->device >= 0 && b->device < kPoolDevices) ? g_lanes_probe_last[b->device] : -1;
}
int asdr_lanes_enabled(asdr_batch_t *b) {
  if (!b) return -1;
  if (is_sharded(b)) { for (asdr_batch *sh : b->shards) if (!asdr_lanes_enabled(sh)) return 0; return 1; }
  if (!b->lanes_enabled) return 0;
  const int probe = (b->device >= 0 && b->device < kPoolDevices) ? g_lanes_probe_last[b->device] : -1;
  return (probe == 0 && !b->lanes_forced) ? 0 : 1;   // (what the next lane-sized call will do, as far as is known now)
}
long asdr_sam_chunk_calls(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_sam_chunk_calls; return t; }
  return b ? b->stat_sam_chunk_calls : -1;
}
long asdr_als_role_calls(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_als_role_calls; return t; }
  return b ? b->stat_als_role_calls : -1;
}
long asdr_sam_role_calls(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_sam_role_calls; return t; }
  return b ? b->stat_sam_role_calls : -1;
}
int asdr_set_lanes(asdr_batch_t *b, int on, int min_waves) {
  if (!b) return fail("null batch");
  if (on < 0 || on > ASDR_LANES) return fail("lanes: 0 (off), 1 (on), or the number of lanes 2..8");
  FOR_SHARDS(b, asdr_set_lanes(sh_, on, min_waves));
  if (b->device != ASDR_NO_DEVICE && b->lanes_pending) { HIPCHK(hipSetDevice(b->device)); if (sync_all(b) != 0) return -1; }
  b->lanes_enabled = on != 0;
  b->lanes_forced = on != 0;
  if (on >= 2) { b->n_lanes = on; b->n_lanes_sam = on; b->sched_dirty = true; }   // an explicit count, for every schedule (the writers' places follow it)
  if (min_waves > 0) b->lanes_min_waves = std::max(2 * ASDR_LANES, min_waves);
  return 0;
}
int asdr_set_launch_split(asdr_batch_t *b, int pieces, int min_waves) {
  if (!b) return fail("null batch");
  if (pieces < 1 || pieces > 8) return fail("launch split must be in 1..8");
  FOR_SHARDS(b, asdr_set_launch_split(sh_, pieces, min_waves));
  b->launch_split = pieces;
  if (min_waves > 0) b->launch_split_min_waves = std::max(8, min_waves);
  return 0;
}
int asdr_set_host_chunks(asdr_batch_t *b, int chunks) {
  if (!b) return fail("null batch");
  if (chunks < 0 || chunks > 4096) return fail("bad chunk count");
  if (is_sharded(b)) { for (asdr_batch *s : b->shards) s->host_chunks_forced = chunks; return 0; }
  b->host_chunks_forced = chunks;
  return 0;
}
// The chunk plan the overlapped host path would use for `chunks` chunks of this batch's current schedule (asdr_update, build_host_plan):
// bound[0..chunks] = channel boundaries, need_in[p] = the last input chunk kernel part p waits for, last_part[j] = the kernel part after
// which output chunk j is complete.  Host logic only: works on a control-plane-only batch after asdr_control_plane_flush (the tests'
// handle on the plan's two promises -- no part runs before its channels have arrived, no chunk leaves before its channels are done).
int asdr_debug_host_plan(asdr_batch_t *b, int chunks, int *bound, int *need_in, int *last_part) {
  if (!b || is_sharded(b)) return fail("asdr_debug_host_plan: a plain batch");
  if (chunks < 1 || chunks > b->n || b->sched_dirty) return fail("asdr_debug_host_plan: bad chunk count, or no schedule yet");
  HostPlan hp;
  build_host_plan(b, hp, chunks);
  for (int j = 0; j <= chunks; j++) if (bound) bound[j] = hp.bound[j];
  for (int j = 0; j < chunks; j++) { if (need_in) need_in[j] = hp.need_in[j]; if (last_part) last_part[j] = hp.last_part[j]; }
  return 0;
}
// ... and the slots [first, first + count) of the schedule that kernel part `part` of `parts` launches, sub-range by sub-range:
// out = up to 16 (first, count) pairs; returns the number of pairs.  (The same arithmetic as update_device_part.)
int asdr_debug_part_slots(asdr_batch_t *b, int part, int parts, int *out) {
  if (!b || is_sharded(b) || !out || parts < 1 || part < 0 || part >= parts || b->sched_dirty) return fail("asdr_debug_part_slots: bad argument");
  int n = 0;
  auto sub = [&](int first, int slots) {
    const long w = slots / 8;
    const int lo = (int)(w * part / parts) * 8, cnt = (int)(w * (part + 1) / parts) * 8 - lo;
    if (cnt > 0 && n < 16) { out[2 * n] = first + lo; out[2 * n + 1] = cnt; n++; }
  };
  if (b->left_slots > 0) sub(b->left_first, b->left_slots);
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) {
    const int nu = b->kind_uniform_slots[k], nm = b->kind_slots[k] - nu;
    if (nu > 0) sub(b->kind_first[k], nu);
    if (nm > 0) sub(b->kind_first[k] + nu, nm);
  }
  return n;
}
int asdr_debug_schedule(asdr_batch_t *b, int *channels, int cap) {   // channel index of every schedule slot (n_channels = padding); returns the slot count
  if (!b || is_sharded(b) || b->sched_dirty) return fail("asdr_debug_schedule: no schedule yet");
  for (size_t i = 0; i < b->sched.size() && (int)i < cap; i++) channels[i] = b->sched[i].ch;
  return (int)b->sched.size();
}
int asdr_host_path_info(asdr_batch_t *b, int out[2]) {
  if (!b || !out) return fail("null argument");
  const asdr_batch *s = is_sharded(b) ? b->shards[0] : b;
  out[0] = s->stat_host_chunks; out[1] = s->stat_host_pinned;
  return 0;
}

int asdr_synchronize(asdr_batch_t *b) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_synchronize(sh_));
  if (b->device == ASDR_NO_DEVICE) return 0;
  HIPCHK(hipSetDevice(b->device));
  if (sync_all(b) != 0) return -1;
  return check_stream_error(b);
}

float asdr_last_kernel_ms(asdr_batch_t *b) {
  if (is_sharded(b)) { float mx = -1.0f; for (asdr_batch *sh : b->shards) mx = std::max(mx, asdr_last_kernel_ms(sh)); return mx; }   // the slowest shard
  if (!b || !b->ev_valid) return -1.0f;
  float ms = -1.0f;
  if (hipEventSynchronize(b->ev1) != hipSuccess) return -1.0f;
  if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) return -1.0f;
  return ms;
}

int asdr_set_launch_timing(asdr_batch_t *b, int on) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_set_launch_timing(sh_, on));
  b->time_calls = on != 0;
  if (!on) b->ev_valid = false;
  return 0;
}

int asdr_region_timing_begin(asdr_batch_t *b, void *stream_) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) return fail("region timing is per device: use the shard handles (asdr_shard)");
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch has no device state");
  HIPCHK(hipSetDevice(b->device));
  if (stream_ == ASDR_STREAM_BATCH) {   // the batch's own lanes: the region starts / ends when BOTH are there (lane 0 waits for lane 1)
    if (!lane_stream(b, 0)) return fail("stream creation failed");
    b->region_stream = b->lane[0]; b->region_on_lanes = true;
    for (int l = 1; l < ASDR_LANES + 1; l++) if (b->lane[l]) { HIPCHK(hipEventRecord(b->ev_lane[l], b->lane[l])); HIPCHK(hipStreamWaitEvent(b->lane[0], b->ev_lane[l], 0)); }
  } else {
    b->region_stream = (hipStream_t)stream_; b->region_on_lanes = false;
  }
  HIPCHK(hipEventRecord(b->rev0, b->region_stream));
  // ... and no lane runs ahead into the region: never-joined lanes drift apart (a lane that shares its stream with another falls behind
  // the rest), and a lane that is hundreds of calls ahead at the begin marker has done part of the region's work before it -- the
  // region then reads shorter than the work takes (C3 with four lanes on three streams read 0.45 ms per call for a true 0.49)
  if (b->region_on_lanes) for (int l = 1; l < ASDR_LANES + 1; l++) if (b->lane[l]) HIPCHK(hipStreamWaitEvent(b->lane[l], b->rev0, 0));
  b->region_calls = 0;
  return 0;
}

int asdr_region_timing_end(asdr_batch_t *b, float *ms_total, long *n_calls) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) return fail("region timing is per device: use the shard handles (asdr_shard)");
  if (b->region_calls < 0) return fail("asdr_region_timing_end without asdr_region_timing_begin");
  HIPCHK(hipSetDevice(b->device));
  if (b->region_on_lanes) {
    if (!b->last_was_lanes && b->ev_last_valid) {   // the region's last call ran the ordinary way, on the batch's stream: behind that, too
      HIPCHK(hipEventRecord(b->ev_last, b->last_stream));
      HIPCHK(hipStreamWaitEvent(b->lane[0], b->ev_last, 0));
    }
    for (int l = 1; l < ASDR_LANES + 1; l++) if (b->lane[l]) { HIPCHK(hipEventRecord(b->ev_lane[l], b->lane[l])); HIPCHK(hipStreamWaitEvent(b->lane[0], b->ev_lane[l], 0)); }
  }
  HIPCHK(hipEventRecord(b->rev1, b->region_stream));
  HIPCHK(hipEventSynchronize(b->rev1));
  float ms = 0.0f;
  HIPCHK(hipEventElapsedTime(&ms, b->rev0, b->rev1));
  if (ms_total) *ms_total = ms;
  if (n_calls) *n_calls = b->region_calls;
  b->region_calls = -1;
  return 0;
}

int asdr_kernel_timing_begin(asdr_batch_t *b, int max_launches) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) return fail("kernel timing is per device: use the shard handles (asdr_shard)");
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch has no device state");
  HIPCHK(hipSetDevice(b->device));
  for (hipEvent_t e : b->tev) hipEventDestroy(e);
  b->tev.clear(); b->tev_used = 0;
  for (int i = 0; i < 2 * max_launches; i++) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); b->tev.push_back(e); }
  return 0;
}

int asdr_kernel_timing_end(asdr_batch_t *b, float *ms, int cap) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) return fail("kernel timing is per device: use the shard handles (asdr_shard)");
  const int n = (int)(b->tev_used / 2);
  for (int i = 0; i < n && i < cap; i++) {
    HIPCHK(hipEventSynchronize(b->tev[2 * i + 1]));
    HIPCHK(hipEventElapsedTime(&ms[i], b->tev[2 * i], b->tev[2 * i + 1]));
  }
  for (hipEvent_t e : b->tev) hipEventDestroy(e);
  b->tev.clear(); b->tev_used = 0;
  return n < cap ? n : cap;
}

// ---- general ------------------------------------------------------------------------------------------
void asdr_init(asdr_batch_t *b, int ch) { each(b, ch, [&](int i, Chan &) { chan_init(b, i); }); }
void asdr_setMute(asdr_batch_t *b, int ch, int muted) {  // .cpp:249-253
  each(b, ch, [&](int, Chan &c) { c.muted = muted != 0; c.current_out_gain = c.muted ? 0.0f : c.out_gain; });
}
int asdr_getMute(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->muted : 0; }
void asdr_setInputGain(asdr_batch_t *b, int ch, float g) {  // .cpp:232-238
  if (g > 10.0) g = 10.0f;
  if (g < 0.0) g = 0.0f;
  each(b, ch, [&](int, Chan &c) { c.in_gain = g; c.in_gain_i = c.in_gain * c.gain_balance; c.in_gain_q = c.in_gain; });
}
void asdr_setIQgainBalance(asdr_batch_t *b, int ch, float balance) {  // .cpp:240-244 (a local shadows _gainBalance)
  const float gb = sqrtf(balance);
  each(b, ch, [&](int, Chan &c) { c.in_gain_i = c.in_gain * gb; c.in_gain_q = c.in_gain / gb; });
}
void asdr_setOutputGain(asdr_batch_t *b, int ch, float g) { each(b, ch, [&](int, Chan &c) { c.output_gain = g; }); }
float asdr_setDemodMode(asdr_batch_t *b, int ch, int mode) {
  float r = 0.0f;
  bool first = true;
  each(b, ch, [&](int i, Chan &) { float v = set_mode(b, i, mode); if (first) { r = v; first = false; } });
  return r;
}
int16_t asdr_getDemodMode(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? (int16_t)c->mode : 0; }
float asdr_getTuningOffset(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->freq_shift : 0.0f; }
float asdr_getBPFlower(asdr_batch_t *b, int ch) {  // .cpp:259-265
  const Chan *c = get(b, ch);
  if (!c) return 0.0f;
  const uint16_t m = c->mode;
  if (m == ASDR_USBmode || m == ASDR_LSBmode) return (float)((double)kIFcenter - (double)kBWssb / 2.0);
  else if (m == ASDR_CW_USBmode || m == ASDR_CW_LSBmode) return (float)((double)kIFcenter - (double)kBWcw / 2.0);
  else if (m == ASDR_AMmode || m == ASDR_SAMmode) return (float)((double)kIFcenter - (double)kBWam / 2.0);
  else if (m == ASDR_WSPRmode) return (float)((double)kIFcenter - (double)kBWwspr / 2.0);
  return 0.0f;
}
float asdr_getBPFupper(asdr_batch_t *b, int ch) {  // .cpp:267-273 (WSPR: `+-` at :271)
  const Chan *c = get(b, ch);
  if (!c) return 0.0f;
  const uint16_t m = c->mode;
  if (m == ASDR_USBmode || m == ASDR_LSBmode) return (float)((double)kIFcenter + (double)kBWssb / 2.0);
  else if (m == ASDR_CW_USBmode || m == ASDR_CW_LSBmode) return (float)((double)kIFcenter + (double)kBWcw / 2.0);
  else if (m == ASDR_AMmode || m == ASDR_SAMmode) return (float)((double)kIFcenter + (double)kBWam / 2.0);
  else if (m == ASDR_WSPRmode) return (float)((double)kIFcenter + -((double)kBWwspr / 2.0));
  return 0.0f;
}

// ---- audio filter ----------------------------------------------------------------------------------------
void asdr_enableAudioFilter(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.af_en = true; }); }
void asdr_disableAudioFilter(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.af_en = false; }); }
void asdr_setAudioFilter(asdr_batch_t *b, int ch, int filter) {  // .cpp:298-311
  each(b, ch, [&](int i, Chan &c) {
    if (filter == ASDR_audioBypass) c.af_en = false;
    else if (filter >= ASDR_audioAM && filter <= ASDR_audio3300) {
      c.audio_table = ASDR_TBL_AUDIO_BASE + filter;
      mark_reset(b, i, ASDR_R_AF);
    }
    c.current_filter = (int16_t)filter;
  });
}
int asdr_getAudioFilter(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->current_filter : 0; }

// ---- ALS ---------------------------------------------------------------------------------------------------
void asdr_enableALSfilter(asdr_batch_t *b, int ch) {  // .cpp:384-391
  each(b, ch, [&](int i, Chan &c) { c.als_en = true; mark_reset(b, i, ASDR_R_ALS); });
}
void asdr_disableALSfilter(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.als_en = false; }); }
void asdr_setALSfilterNotch(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.als_notch = true; }); }
void asdr_setALSfilterPeak(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.als_notch = false; }); }
void asdr_setALSfilterAdaptive(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.als_adaptive = true; }); }
void asdr_setALSfilterStatic(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.als_adaptive = false; }); }
void asdr_setALSfilterParams(asdr_batch_t *b, int ch, unsigned int m, float lambda, float delay) {  // .cpp:393-398
  each(b, ch, [&](int, Chan &c) {
    c.als_m = (int16_t)m;
    if (c.als_m >= ASDR_N) c.als_m = ASDR_N;
    c.als_lambda = lambda;
    c.als_delay = (int16_t)delay;
  });
}
int asdr_ALSfilterIsEnabled(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->als_en : 0; }
int asdr_ALSfilterIsNotch(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->als_notch : 0; }
int asdr_ALSfilterIsPeak(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? !c->als_notch : 0; }
int asdr_ALSfilterIsAdaptive(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->als_adaptive : 0; }

// ---- AGC ---------------------------------------------------------------------------------------------------
void asdr_enableAGC(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.agc_en = true; }); }
void asdr_disableAGC(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.agc_en = false; }); }
int asdr_AGCisEnabled(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->agc_en : 0; }
void asdr_setAGCthreshold(asdr_batch_t *b, int ch, float v) { each(b, ch, [&](int, Chan &c) { c.agc_threshold = v; rebuild_agc(b, c); }); }
void asdr_setAGCslope(asdr_batch_t *b, int ch, float v) { each(b, ch, [&](int, Chan &c) { c.agc_slope = v; rebuild_agc(b, c); }); }
void asdr_setAGCkneeWidth(asdr_batch_t *b, int ch, float v) { each(b, ch, [&](int, Chan &c) { c.agc_knee = v; rebuild_agc(b, c); }); }
void asdr_setAGCattackTime(asdr_batch_t *b, int ch, float ms) {  // .cpp:551-555
  const float al = time_constant(ms), be = (float)(1.0 - (double)al);
  each(b, ch, [&](int, Chan &c) { c.agc_attack_ms = ms; c.agc_alpha_att = al; c.agc_beta_att = be; });
}
void asdr_setAGCreleaseTime(asdr_batch_t *b, int ch, float ms) {  // .cpp:557-561
  const float al = time_constant(ms), be = (float)(1.0 - (double)al);
  each(b, ch, [&](int, Chan &c) { c.agc_release_ms = ms; c.agc_alpha_rel = al; c.agc_beta_rel = be; });
}
void asdr_setAGChangTime(asdr_batch_t *b, int ch, float ms) {  // .cpp:563-566: float product, then / 1000.0
  const uint32_t cnt = (uint32_t)((double)(ms * kFs) / 1000.0);
  each(b, ch, [&](int, Chan &c) { c.agc_slot129 = ms; c.agc_hang_count = cnt; });
}
void asdr_setAGCstaticGain(asdr_batch_t *b, int ch, float g) { each(b, ch, [&](int, Chan &c) { c.agc_static_gain = g; }); }
void asdr_setAGCmode(asdr_batch_t *b, int ch, int mode) {  // .cpp:524-544
  mode = (int16_t)mode;
  if (mode == ASDR_AGCoff) asdr_disableAGC(b, ch);
  else if (mode == ASDR_AGCfast) { asdr_setAGCattackTime(b, ch, 2.0f); asdr_setAGCreleaseTime(b, ch, 100.0f); asdr_setAGChangTime(b, ch, 100.0f); asdr_enableAGC(b, ch); }
  else if (mode == ASDR_AGCmedium) { asdr_setAGCattackTime(b, ch, 5.0f); asdr_setAGCreleaseTime(b, ch, 250.0f); asdr_setAGChangTime(b, ch, 500.0f); asdr_enableAGC(b, ch); }
  else if (mode == ASDR_AGCslow) { asdr_setAGCattackTime(b, ch, 10.0f); asdr_setAGCreleaseTime(b, ch, 500.0f); asdr_setAGChangTime(b, ch, 2000.0f); asdr_enableAGC(b, ch); }
}
#define GETF(name, field) float asdr_##name(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->field : 0.0f; }
GETF(getAGCthreshold, agc_threshold)
GETF(getAGCslope, agc_slope)
GETF(getAGCkneeWidth, agc_knee)
GETF(getAGCattack, agc_attack_ms)
GETF(getAGCrelease, agc_release_ms)
GETF(getAAGalphaAttack, agc_alpha_att)
GETF(getAGCbetaAttack, agc_beta_att)
GETF(getAGCalphaRelease, agc_alpha_rel)
GETF(getAGCbetaRelease, agc_beta_rel)
GETF(getAGCstaticGain, agc_static_gain)
float asdr_getAGClookup(asdr_batch_t *b, int ch, int i) {
  const Chan *c = get(b, ch);
  if (!c || i < 0 || i > 129) return 0.0f;
  return (i == 129) ? c->agc_slot129 : b->agc_pool[c->agc_table].v[i];
}

// ---- noise blanker ------------------------------------------------------------------------------------------
void asdr_enableNoiseBlanker(asdr_batch_t *b, int ch) {
  each(b, ch, [&](int i, Chan &c) { c.nb_en = true; mark_reset(b, i, ASDR_R_NB); });
}
void asdr_disableNoiseBlanker(asdr_batch_t *b, int ch) { each(b, ch, [&](int, Chan &c) { c.nb_en = false; }); }
void asdr_setNoiseBlankerThreshold(asdr_batch_t *b, int ch, float r) {
  each(b, ch, [&](int i, Chan &c) { c.nb_threshold = r; mark_reset(b, i, ASDR_R_NB); });
}
void asdr_setNoiseBlankerThresholdDb(asdr_batch_t *b, int ch, float db) {  // .cpp:671-674
  const float r = powf(10.0f, (float)((double)db / 20.0));
  each(b, ch, [&](int i, Chan &c) { c.nb_threshold = r; mark_reset(b, i, ASDR_R_NB); });
}
int asdr_NoiseBlankerisEnabled(asdr_batch_t *b, int ch) { const Chan *c = get(b, ch); return c ? c->nb_en : 0; }

// ---- getters that read hot-path state ------------------------------------------------------------------------
int asdr_AGCisActive(asdr_batch_t *b, int ch) { ChanSmall s; return read_small(b, ch, s) == 0 ? ((s.status & ASDR_S_AGC_ACTIVE) != 0) : 0; }
int asdr_NoiseBlankerDetection(asdr_batch_t *b, int ch) { ChanSmall s; return read_small(b, ch, s) == 0 ? ((s.status & ASDR_S_NB_DETECTED) != 0) : 0; }
int asdr_getSAMphaseLockStatus(asdr_batch_t *b, int ch) { ChanSmall s; return read_small(b, ch, s) == 0 ? ((s.status & ASDR_S_PLL_LOCKED) != 0) : 0; }
float asdr_getSAMfrequency(asdr_batch_t *b, int ch) { ChanSmall s; return read_small(b, ch, s) == 0 ? s.pll_freq : 0.0f; }
float asdr_getAMcarrierLevel(asdr_batch_t *b, int ch) { ChanSmall s; return read_small(b, ch, s) == 0 ? s.am_carrier : 0.0f; }

int asdr_read_status(asdr_batch_t *b, int32_t *agc_active, int32_t *nb_detected, int32_t *sam_locked, float *sam_frequency,
                     float *am_carrier) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) {   // every shard fills its channel range of the caller's arrays
    for (size_t g = 0; g < b->shards.size(); g++) {
      const int f = b->shard_first[g];
      if (asdr_read_status(b->shards[g], agc_active ? agc_active + f : nullptr, nb_detected ? nb_detected + f : nullptr, sam_locked ? sam_locked + f : nullptr,
                           sam_frequency ? sam_frequency + f : nullptr, am_carrier ? am_carrier + f : nullptr) != 0) return -1;
    }
    return 0;
  }
  ChanSmall probe;
  if (read_small(b, 0, probe) != 0) return -1;  // synchronises + applies pending resets
  std::vector<ChanSmall> all(b->n);
  HIPCHK(hipMemcpy(all.data(), b->d_small, (size_t)b->n * sizeof(ChanSmall), hipMemcpyDeviceToHost));
  for (int i = 0; i < b->n; i++) {
    if (agc_active) agc_active[i] = (all[i].status & ASDR_S_AGC_ACTIVE) != 0;
    if (nb_detected) nb_detected[i] = (all[i].status & ASDR_S_NB_DETECTED) != 0;
    if (sam_locked) sam_locked[i] = (all[i].status & ASDR_S_PLL_LOCKED) != 0;
    if (sam_frequency) sam_frequency[i] = all[i].pll_freq;
    if (am_carrier) am_carrier[i] = all[i].am_carrier;
  }
  return 0;
}

unsigned int asdr_get_chain_constants(asdr_batch_t *b, int ch, float out[12]) {
  if (!b) return 0;
  const ChainConsts &k = b->k;
  if (out) {
    const float v[12] = {k.pll_b0, k.pll_b1, k.pll_a1, k.pll_alpha_freq, k.pll_beta_freq, k.pll_f_conv, k.pll_lock_lo, k.pll_lock_hi,
                         k.two_pi_f, k.half_pi_f, k.phase_inc_unit, k.nb_beta};
    memcpy(out, v, sizeof v);
  }
  const Chan *c = get(b, ch);
  return c ? c->agc_hang_count : 0u;
}

long asdr_stream_pipeline_launches(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_stream_launches; return t; }
  return b ? b->stat_stream_launches : -1;
}
long asdr_stream_pipeline_recoveries(asdr_batch_t *b) {
  if (!b) return -1;
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) { const long r = asdr_stream_pipeline_recoveries(sh); if (r < 0) return -1; t += r; } return t; }
  if (b->device != ASDR_NO_DEVICE && b->stream_launched) { if (hipSetDevice(b->device) != hipSuccess || check_stream_error(b) != 0) return -1; }
  return b->stat_stream_recoveries;
}
long asdr_stream_pipeline_alloc_failures(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_stream_alloc_failures; return t; }
  return b ? b->stat_stream_alloc_failures : -1;
}
long asdr_stream_pipeline_headroom_refusals(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_stream_headroom_refusals; return t; }
  return b ? b->stat_stream_headroom_refusals : -1;
}
long asdr_stream_pipeline_h3_calls(asdr_batch_t *b) {
  if (is_sharded(b)) { long t = 0; for (asdr_batch *sh : b->shards) t += sh->stat_stream_h3_calls; return t; }
  return b ? b->stat_stream_h3_calls : -1;
}
int asdr_set_stream_fir_helpers(asdr_batch_t *b, int mode) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_set_stream_fir_helpers(sh_, mode));
  if (mode < -1 || mode > 1) return fail("bad mode (-1 = by the rule, 0 = always one helper wave, 1 = three wherever they are resident)");
  b->stream_h3 = mode;
  return 0;
}
int asdr_stream_pipeline_max_groups(asdr_batch_t *b) {   // (per shard: every shard is a launch of its own)
  if (is_sharded(b)) { int m = 0x7fffffff; for (asdr_batch *sh : b->shards) m = std::min(m, sh->stream_max_waves); return m; }
  return b ? b->stream_max_waves : -1;
}
int asdr_set_stream_pipeline(asdr_batch_t *b, int on) { if (!b) return fail("null batch"); FOR_SHARDS(b, asdr_set_stream_pipeline(sh_, on)); b->stream_pipeline = on != 0; return 0; }
int asdr_set_als_launch_form(asdr_batch_t *b, int split_min_channels) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_set_als_launch_form(sh_, split_min_channels));
  b->als_split_min = split_min_channels > 0 ? split_min_channels : 0x7fffffff;
  b->sched_dirty = true;
  return 0;
}
int asdr_set_sam_launch_form(asdr_batch_t *b, int fused, int split_min_channels) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_set_sam_launch_form(sh_, fused, split_min_channels));
  b->sam_fused = fused != 0;
  b->sam_split_min = split_min_channels > 0 ? split_min_channels : ASDR_SAM_SPLIT_MIN_CHANNELS;
  b->sched_dirty = true;
  return 0;
}
int asdr_debug_set_stream_max_groups(asdr_batch_t *b, int groups) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_debug_set_stream_max_groups(sh_, groups));
  if (groups < 0 || groups > ASDR_STREAM_MAX_WAVES) return fail("bad group count");
  // never beyond what the device holds at once (the occupancy query of asdr_create): more groups than resident workgroups cannot
  // make progress and every call would sit out its 2^18 polls before the recovery launches run
  if (b->stream_query_waves > 0 && groups > b->stream_query_waves) groups = b->stream_query_waves;
  b->stream_max_waves = groups;
  return 0;
}
int asdr_debug_set_stream_spin_limit(asdr_batch_t *b, unsigned int polls) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_debug_set_stream_spin_limit(sh_, polls));
  b->stream_spin_limit = polls ? polls : ASDR_STREAM_SPIN_LIMIT;
  return 0;
}

int asdr_set_exact_unknown_mode(asdr_batch_t *b, int on) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_set_exact_unknown_mode(sh_, on));
  const bool want = on != 0;
  if (want && !b->exact_unknown_mode && b->device != ASDR_NO_DEVICE) {   // rows not kept meanwhile: silence until a block stores them again
    HIPCHK(hipSetDevice(b->device));
    if (sync_all(b) != 0) return -1;
    HIPCHK(hipMemset(b->d_audio_prev, 0, ((size_t)b->n + 1) * 128 * sizeof(float)));
    HIPCHK(hipStreamSynchronize(nullptr));   // (the fill runs on the null stream: see asdr_create)
  }
  b->exact_unknown_mode = want;
  return 0;
}
int asdr_get_exact_unknown_mode(asdr_batch_t *b) { if (is_sharded(b)) b = b->shards[0]; return b ? (b->exact_unknown_mode ? 1 : 0) : -1; }

int asdr_schedule_layout(asdr_batch_t *b, int out[8]) {
  if (!b || !out) return fail("null argument");
  if (is_sharded(b)) {   // slots summed over the shards (each shard pads its own sub-ranges); kinds / launch forms: any shard's
    int acc[8] = {0, 0, 0, 0, 0, 0, -1, 0};
    for (asdr_batch *sh : b->shards) {
      int o[8];
      if (asdr_schedule_layout(sh, o) != 0) return -1;
      for (int k = 0; k < 6; k++) acc[k] += o[k];
      acc[6] = std::max(acc[6], o[6]); acc[7] |= o[7];
    }
    memcpy(out, acc, sizeof acc);
    return 0;
  }
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) out[k] = b->kind_slots[k];
  out[5] = b->left_slots; out[6] = b->left_slots ? b->left_kind : -1; out[7] = (b->sam_split ? 1 : 0) | (b->als_split ? 2 : 0);
  return 0;
}

int asdr_params_uniform_groups(asdr_batch_t *b, long *rows_compared) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) {
    int acc = 0; long rows = 0;
    for (asdr_batch *sh : b->shards) { long r = 0; const int g = asdr_params_uniform_groups(sh, &r); if (g < 0) return -1; acc += g; rows += r; }
    if (rows_compared) *rows_compared = rows;
    return acc;
  }
  int g = 0;
  for (int k = 0; k < ASDR_KERNEL_KINDS; k++) g += (b->kind_direct[k] && b->kind_puni[k]) ? 1 : 0;
  if (rows_compared) *rows_compared = b->stat_puni_rows_compared;
  return g;
}

int asdr_control_plane_flush(asdr_batch_t *b, long long stats[4]) {
  if (!b) return fail("null batch");
  if (is_sharded(b)) {   // rows refilled / waves / live tables summed over the shards, "rebuilt" if any shard rebuilt
    long long acc[4] = {0, 0, 0, 0};
    for (asdr_batch *sh : b->shards) {
      long long st[4];
      if (asdr_control_plane_flush(sh, st) != 0) return -1;
      acc[0] += st[0]; acc[1] |= st[1]; acc[2] += st[2]; acc[3] += st[3];
    }
    if (stats) memcpy(stats, acc, sizeof acc);
    return 0;
  }
  if (b->device != ASDR_NO_DEVICE) return fail("asdr_control_plane_flush is for control-plane-only batches: a device batch flushes in update()");
  std::vector<int32_t> changed;
  bool bulk = false, rebuilt = false;
  flush_host(b, changed, bulk, rebuilt);
  b->agc_pool_dirty = false;
  if (stats) {
    stats[0] = b->stat_rows_refilled; stats[1] = rebuilt ? 1 : 0;
    const int lw = b->left_slots / 8;   // the remainders' waves count with the kind whose general kernel runs them
    stats[2] = (long long)(b->kind_slots[ASDR_KERNEL_PLAIN] / 8 + (b->left_kind == ASDR_KERNEL_PLAIN ? lw : 0)) | ((long long)(b->kind_slots[ASDR_KERNEL_SAM] / 8) << 21) |
               ((long long)((b->kind_slots[ASDR_KERNEL_ALS] + b->kind_slots[ASDR_KERNEL_ALS_SMALL] + b->kind_slots[ASDR_KERNEL_SAM_ALS]) / 8 + (b->left_kind == ASDR_KERNEL_ALS ? lw : 0)) << 42);
    long long live = 0;
    for (uint32_t r : b->agc_refs) live += (r != 0);
    stats[3] = live;
  }
  return 0;
}

int asdr_enable_taps(asdr_batch_t *b, int on) {
  if (!b) return fail("null batch");
  FOR_SHARDS(b, asdr_enable_taps(sh_, on));
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch has no device state");
  HIPCHK(hipSetDevice(b->device));
  if (on && !b->d_taps) {
    const size_t bytes = (size_t)ASDR_N_TAPS * b->n * ASDR_N * sizeof(float);
    HIPCHK(hipMalloc(&b->d_taps, bytes));
    HIPCHK(hipMemset(b->d_taps, 0, bytes));
    HIPCHK(hipStreamSynchronize(nullptr));   // (the fill runs on the null stream: see asdr_create)
  }
  b->taps_on = on != 0;
  return 0;
}

int asdr_read_taps(asdr_batch_t *b, float *dst) {
  if (is_sharded(b)) {   // [tap][global channel][128] from the shards' [tap][local channel][128]
    if (!dst) return fail("taps not enabled");
    std::vector<float> tmp;
    for (size_t g = 0; g < b->shards.size(); g++) {
      asdr_batch *sh = b->shards[g];
      tmp.resize((size_t)ASDR_N_TAPS * sh->n * ASDR_N);
      if (asdr_read_taps(sh, tmp.data()) != 0) return -1;
      for (int t = 0; t < ASDR_N_TAPS; t++)
        memcpy(dst + ((size_t)t * b->n + b->shard_first[g]) * ASDR_N, tmp.data() + (size_t)t * sh->n * ASDR_N, (size_t)sh->n * ASDR_N * sizeof(float));
    }
    return 0;
  }
  if (!b || !b->d_taps || !dst) return fail("taps not enabled");
  if (asdr_synchronize(b) != 0) return -1;
  HIPCHK(hipMemcpy(dst, b->d_taps, (size_t)ASDR_N_TAPS * b->n * ASDR_N * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

// ---- receiver state records (include/asdr.h "receiver state records"; kernels: asdr_state.hip) ------------------------------------------
// A record = header | control part (every member of struct Chan, the gain table as its (threshold, slope, knee) triple) | signal part (the nine
// state rows in canonical order).  The host writes and reads the first ASDR_STATE_OFF_SMALL bytes; the two kernels move the rest.
extern "C" int asdr_launch_state_gather(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, void *records, const void *ctl, hipStream_t stream);
extern "C" int asdr_launch_state_scatter(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, const void *records, hipStream_t stream);

namespace {

constexpr size_t kRec = ASDR_STATE_RECORD_BYTES, kCtl = ASDR_STATE_OFF_SMALL;
constexpr int kStateChunk = 4096;   // records per staging round of the host forms (26 MB pinned + 26 MB of HBM)
// control words, in record order (word i lives at byte ASDR_STATE_OFF_CONTROL + 4 i)
enum { CW_IN_GAIN, CW_IN_GAIN_I, CW_IN_GAIN_Q, CW_GAIN_BALANCE, CW_OUTPUT_GAIN, CW_OUT_GAIN, CW_CURRENT_OUT_GAIN, CW_FREQ_SHIFT, CW_MODE, CW_MUTED,
       CW_CURRENT_FILTER, CW_AF_EN, CW_IF_TABLE, CW_AUDIO_TABLE, CW_ALS_M, CW_ALS_DELAY, CW_ALS_LAMBDA, CW_ALS_EN, CW_ALS_NOTCH, CW_ALS_ADAPTIVE,
       CW_ALPHA_ATT, CW_BETA_ATT, CW_ALPHA_REL, CW_BETA_REL, CW_ATTACK_MS, CW_RELEASE_MS, CW_KNEE, CW_SLOPE, CW_THRESHOLD, CW_STATIC_GAIN,
       CW_SLOT129, CW_HANG_COUNT, CW_AGC_EN, CW_NB_THRESHOLD, CW_NB_EN, CW_ZERO, CW_COUNT };
static_assert(ASDR_STATE_OFF_CONTROL + 4 * CW_COUNT == ASDR_STATE_OFF_SMALL, "control part");

struct StateField { const char *name; int offset, count; };
#define SF_CW(name, type, w) {name ":" type, ASDR_STATE_OFF_CONTROL + 4 * (w), 1}
#define SF_SM(name, type, word, count) {name ":" type, ASDR_STATE_OFF_SMALL + 4 * (word), count}
const StateField kStateFields[] = {
  {"magic:u32", 0, 1}, {"version:u32", 4, 1}, {"bytes:u32", 8, 1}, {"content:u32", 12, 1},
  SF_CW("in_gain", "f32", CW_IN_GAIN), SF_CW("in_gain_i", "f32", CW_IN_GAIN_I), SF_CW("in_gain_q", "f32", CW_IN_GAIN_Q), SF_CW("gain_balance", "f32", CW_GAIN_BALANCE),
  SF_CW("output_gain", "f32", CW_OUTPUT_GAIN), SF_CW("out_gain", "f32", CW_OUT_GAIN), SF_CW("current_out_gain", "f32", CW_CURRENT_OUT_GAIN),
  SF_CW("freq_shift", "f32", CW_FREQ_SHIFT), SF_CW("mode", "u32", CW_MODE), SF_CW("muted", "u32", CW_MUTED), SF_CW("current_filter", "i32", CW_CURRENT_FILTER),
  SF_CW("af_en", "u32", CW_AF_EN), SF_CW("if_table", "i32", CW_IF_TABLE), SF_CW("audio_table", "i32", CW_AUDIO_TABLE), SF_CW("als_m", "i32", CW_ALS_M),
  SF_CW("als_delay", "i32", CW_ALS_DELAY), SF_CW("als_lambda", "f32", CW_ALS_LAMBDA), SF_CW("als_en", "u32", CW_ALS_EN), SF_CW("als_notch", "u32", CW_ALS_NOTCH),
  SF_CW("als_adaptive", "u32", CW_ALS_ADAPTIVE), SF_CW("agc_alpha_att", "f32", CW_ALPHA_ATT), SF_CW("agc_beta_att", "f32", CW_BETA_ATT),
  SF_CW("agc_alpha_rel", "f32", CW_ALPHA_REL), SF_CW("agc_beta_rel", "f32", CW_BETA_REL), SF_CW("agc_attack_ms", "f32", CW_ATTACK_MS),
  SF_CW("agc_release_ms", "f32", CW_RELEASE_MS), SF_CW("agc_knee", "f32", CW_KNEE), SF_CW("agc_slope", "f32", CW_SLOPE), SF_CW("agc_threshold", "f32", CW_THRESHOLD),
  SF_CW("agc_static_gain", "f32", CW_STATIC_GAIN), SF_CW("agc_slot129", "f32", CW_SLOT129), SF_CW("agc_hang_count", "u32", CW_HANG_COUNT),
  SF_CW("agc_en", "u32", CW_AGC_EN), SF_CW("nb_threshold", "f32", CW_NB_THRESHOLD), SF_CW("nb_en", "u32", CW_NB_EN),
  SF_SM("if_state", "f32", 0, 32), SF_SM("img_state", "f32", 32, 32), SF_SM("af_state", "f32", 64, 16), SF_SM("phase_ssb", "f32", 80, 1), SF_SM("phase_am", "f32", 81, 1),
  SF_SM("nb_avg", "f32", 82, 1), SF_SM("am_carrier", "f32", 83, 1), SF_SM("agc_gain", "f32", 84, 1), SF_SM("agc_old_abs", "f32", 85, 1), SF_SM("agc_hang_counter", "u32", 86, 1),
  SF_SM("pll_y_re", "f32", 87, 1), SF_SM("pll_y_im", "f32", 88, 1), SF_SM("pll_prev_filt", "f32", 89, 1), SF_SM("pll_d0", "f32", 90, 1), SF_SM("pll_d1", "f32", 91, 1),
  SF_SM("pll_phase_est", "f32", 92, 1), SF_SM("pll_freq", "f32", 93, 1), SF_SM("hil_slot", "u32", 95, 1), SF_SM("status", "u32", 96, 1), SF_SM("nb_gain", "f32", 97, 6),
  {"nb_hist:i16", ASDR_STATE_OFF_NB_HIST, 768}, {"nb_mask:u8", ASDR_STATE_OFF_NB_MASK, ASDR_NB_MASK_ROW}, {"hil_q:f32", ASDR_STATE_OFF_HIL_Q, 256},
  {"hil_i:f32", ASDR_STATE_OFF_HIL_I, 256}, {"als_x:f32", ASDR_STATE_OFF_ALS_X, 256}, {"als_w:f32", ASDR_STATE_OFF_ALS_W, 128},
  {"audio_prev:f32", ASDR_STATE_OFF_AUDIO_PREV, 128},
};
#undef SF_CW
#undef SF_SM
// (word = index in the record's signal part, which keeps ChanSmall's members in their original order -- not their offsets in the 512-byte row: asdr_state.hip)

// header + control part of a record from the host half of a channel
void control_to_record(const Chan &c, uint32_t content, uint8_t *dst) {
  uint32_t w[kCtl / 4] = {};
  w[0] = ASDR_STATE_MAGIC; w[1] = ASDR_STATE_VERSION; w[2] = (uint32_t)kRec; w[3] = content;
  uint32_t *cw = w + ASDR_STATE_OFF_CONTROL / 4;
  auto F = [&](int i, float v) { memcpy(&cw[i], &v, 4); };
  auto I = [&](int i, int32_t v) { memcpy(&cw[i], &v, 4); };
  F(CW_IN_GAIN, c.in_gain); F(CW_IN_GAIN_I, c.in_gain_i); F(CW_IN_GAIN_Q, c.in_gain_q); F(CW_GAIN_BALANCE, c.gain_balance);
  F(CW_OUTPUT_GAIN, c.output_gain); F(CW_OUT_GAIN, c.out_gain); F(CW_CURRENT_OUT_GAIN, c.current_out_gain); F(CW_FREQ_SHIFT, c.freq_shift);
  cw[CW_MODE] = c.mode; cw[CW_MUTED] = c.muted; I(CW_CURRENT_FILTER, c.current_filter); cw[CW_AF_EN] = c.af_en;
  I(CW_IF_TABLE, c.if_table); I(CW_AUDIO_TABLE, c.audio_table); I(CW_ALS_M, c.als_m); I(CW_ALS_DELAY, c.als_delay); F(CW_ALS_LAMBDA, c.als_lambda);
  cw[CW_ALS_EN] = c.als_en; cw[CW_ALS_NOTCH] = c.als_notch; cw[CW_ALS_ADAPTIVE] = c.als_adaptive;
  F(CW_ALPHA_ATT, c.agc_alpha_att); F(CW_BETA_ATT, c.agc_beta_att); F(CW_ALPHA_REL, c.agc_alpha_rel); F(CW_BETA_REL, c.agc_beta_rel);
  F(CW_ATTACK_MS, c.agc_attack_ms); F(CW_RELEASE_MS, c.agc_release_ms);
  // the gain table as its triple: the members ARE the key of the channel's row of the pool (every setter that changes one rebuilds the table)
  F(CW_KNEE, c.agc_knee); F(CW_SLOPE, c.agc_slope); F(CW_THRESHOLD, c.agc_threshold);
  F(CW_STATIC_GAIN, c.agc_static_gain); F(CW_SLOT129, c.agc_slot129); cw[CW_HANG_COUNT] = c.agc_hang_count; cw[CW_AGC_EN] = c.agc_en;
  F(CW_NB_THRESHOLD, c.nb_threshold); cw[CW_NB_EN] = c.nb_en; cw[CW_ZERO] = 0u;
  memcpy(dst, w, kCtl);
}

// what is wrong with a record's first kCtl bytes, or nullptr
const char *check_record(const uint8_t *p) {
  uint32_t w[kCtl / 4];
  memcpy(w, p, kCtl);
  if (w[0] != ASDR_STATE_MAGIC) return "bad magic";
  if (w[1] != ASDR_STATE_VERSION) return "version mismatch (records are not portable across versions)";
  if (w[2] != (uint32_t)kRec) return "wrong size in the `bytes` word";
  if ((w[3] & ~(ASDR_STATE_HAS_SIGNAL | ASDR_STATE_HAS_AUDIO_PREV)) != 0u) return "unknown content bits";
  if ((w[3] & ASDR_STATE_HAS_AUDIO_PREV) && !(w[3] & ASDR_STATE_HAS_SIGNAL)) return "content: audio_prev flag without the signal part";
  const uint32_t *cw = w + ASDR_STATE_OFF_CONTROL / 4;
  const int32_t if_t = (int32_t)cw[CW_IF_TABLE], au_t = (int32_t)cw[CW_AUDIO_TABLE], m = (int32_t)cw[CW_ALS_M], d = (int32_t)cw[CW_ALS_DELAY], cf = (int32_t)cw[CW_CURRENT_FILTER];
  if (if_t < ASDR_TBL_IF_SSB || if_t > ASDR_TBL_IF_AM) return "IF table id out of range";
  if (au_t < ASDR_TBL_AUDIO_BASE + ASDR_audioAM || au_t > ASDR_TBL_AUDIO_BASE + ASDR_audio3300) return "audio table id out of range";
  if (m < -32768 || m > ASDR_N || d < -32768 || d > 32767 || cf < -32768 || cf > 32767) return "ALS length / delay / filter id out of range";
  if (cw[CW_MODE] > 0xFFFFu) return "mode out of range";
  for (int i : {CW_MUTED, CW_AF_EN, CW_ALS_EN, CW_ALS_NOTCH, CW_ALS_ADAPTIVE, CW_AGC_EN, CW_NB_EN}) if (cw[i] > 1u) return "a boolean word is neither 0 nor 1";
  if (cw[CW_ZERO] != 0u) return "pad word not zero";
  return nullptr;
}

// the host half of channel `ch` from a checked record: every member, the gain table found or built in THIS batch's pool (reference counts kept)
void record_to_chan(asdr_batch *b, int ch, const uint8_t *p) {
  uint32_t w[kCtl / 4];
  memcpy(w, p, kCtl);
  const uint32_t *cw = w + ASDR_STATE_OFF_CONTROL / 4;
  auto F = [&](int i) { float v; memcpy(&v, &cw[i], 4); return v; };
  Chan &c = b->ch[ch];
  c.in_gain = F(CW_IN_GAIN); c.in_gain_i = F(CW_IN_GAIN_I); c.in_gain_q = F(CW_IN_GAIN_Q); c.gain_balance = F(CW_GAIN_BALANCE);
  c.output_gain = F(CW_OUTPUT_GAIN); c.out_gain = F(CW_OUT_GAIN); c.current_out_gain = F(CW_CURRENT_OUT_GAIN); c.freq_shift = F(CW_FREQ_SHIFT);
  c.mode = (uint16_t)cw[CW_MODE]; c.muted = cw[CW_MUTED] != 0u; c.current_filter = (int16_t)(int32_t)cw[CW_CURRENT_FILTER]; c.af_en = cw[CW_AF_EN] != 0u;
  c.if_table = (int32_t)cw[CW_IF_TABLE]; c.audio_table = (int32_t)cw[CW_AUDIO_TABLE];
  c.als_m = (int16_t)(int32_t)cw[CW_ALS_M]; c.als_delay = (int16_t)(int32_t)cw[CW_ALS_DELAY]; c.als_lambda = F(CW_ALS_LAMBDA);
  c.als_en = cw[CW_ALS_EN] != 0u; c.als_notch = cw[CW_ALS_NOTCH] != 0u; c.als_adaptive = cw[CW_ALS_ADAPTIVE] != 0u;
  c.agc_alpha_att = F(CW_ALPHA_ATT); c.agc_beta_att = F(CW_BETA_ATT); c.agc_alpha_rel = F(CW_ALPHA_REL); c.agc_beta_rel = F(CW_BETA_REL);
  c.agc_attack_ms = F(CW_ATTACK_MS); c.agc_release_ms = F(CW_RELEASE_MS);
  c.agc_knee = F(CW_KNEE); c.agc_slope = F(CW_SLOPE); c.agc_threshold = F(CW_THRESHOLD);
  rebuild_agc(b, c);   // the setters' own find-or-create: moves the reference from the channel's old table to the triple's (and clobbers slot 129 ...)
  c.agc_slot129 = F(CW_SLOT129);   // ... which the record carries as the exporting channel had it)
  c.agc_static_gain = F(CW_STATIC_GAIN); c.agc_hang_count = cw[CW_HANG_COUNT]; c.agc_en = cw[CW_AGC_EN] != 0u;
  c.nb_threshold = F(CW_NB_THRESHOLD); c.nb_en = cw[CW_NB_EN] != 0u;
}

// the entries of one call that one (unsharded) batch owns: local channel and index into the caller's record array; a NULL channel list gives
// ranges (entry e = channel ch0 + e, record rec0 + e) and no lists
struct StateEntries {
  asdr_batch *b = nullptr;
  std::vector<int> pairs;   // (channel, record) x n, or empty: the range
  int n = 0, ch0 = 0, rec0 = 0;
  int ch(int e) const { return pairs.empty() ? ch0 + e : pairs[2 * (size_t)e]; }
  int rec(int e) const { return pairs.empty() ? rec0 + e : pairs[2 * (size_t)e + 1]; }
};

int state_stage_reserve(asdr_batch *b, size_t h_bytes, size_t d_bytes) {
  if (!b->st_ev) HIPCHK(hipEventCreateWithFlags(&b->st_ev, hipEventDisableTiming));
  if (b->st_ev_pending) { HIPCHK(hipEventSynchronize(b->st_ev)); b->st_ev_pending = false; }   // the pinned half is free again
  if (h_bytes > b->st_h_cap) {
    if (b->st_h) { HIPCHK(hipHostFree(b->st_h)); b->st_h = nullptr; b->st_h_cap = 0; }
    HIPCHK(hipHostMalloc((void **)&b->st_h, h_bytes, hipHostMallocDefault));
    b->st_h_cap = h_bytes;
  }
  if (d_bytes > b->st_d_cap) {
    if (b->st_d) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(b->st_d)); b->st_d = nullptr; b->st_d_cap = 0; }
    HIPCHK(hipMalloc((void **)&b->st_d, d_bytes));
    b->st_d_cap = d_bytes;
  }
  return 0;
}

// `stream` joins the batch's stream order: behind every launch the batch has been given, and the next call on another stream waits for it
// (the rule of update_device_part)
int state_order_in(asdr_batch *b, hipStream_t stream) {
  if (b->lanes_pending) { if (lanes_join_into(b, stream) != 0) return -1; b->lanes_pending = false; b->last_stream = stream; b->last_was_lanes = false; }
  return (b->ev_last_valid && stream != b->last_stream) ? wait_for_last(b, stream) : 0;
}
void state_order_out(asdr_batch *b, hipStream_t stream) { b->last_stream = stream; b->ev_last_valid = true; b->last_was_lanes = false; }

uint32_t state_content(const asdr_batch *b) {
  return b->device == ASDR_NO_DEVICE ? 0u : (ASDR_STATE_HAS_SIGNAL | (b->exact_unknown_mode ? ASDR_STATE_HAS_AUDIO_PREV : 0u));
}

// resets that setters left pending: applied as the next update would apply them first (asdr_read_status does the same)
int state_apply_resets(asdr_batch *b) {
  if (!b->reset_pending) return 0;
  if (sync_all(b) != 0) return -1;
  return apply_resets(b, b->stream);
}

int export_host(const StateEntries &en, uint8_t *out) {
  asdr_batch *b = en.b;
  const uint32_t content = state_content(b);
  if (b->device == ASDR_NO_DEVICE) {
    for (int e = 0; e < en.n; e++) {
      uint8_t *r = out + (size_t)en.rec(e) * kRec;
      const Chan &c = b->ch[en.ch(e)];
      control_to_record(c, content, r);
      memset(r + kCtl, 0, kRec - kCtl);
    }
    return 0;
  }
  HIPCHK(hipSetDevice(b->device));
  if (sync_all(b) != 0) return -1;
  if (check_stream_error(b) != 0) return -1;
  if (apply_resets(b, b->stream) != 0) return -1;
  UpdateArgs a;
  fill_args(b, a);
  for (int e0 = 0; e0 < en.n; e0 += kStateChunk) {
    const int m = std::min(kStateChunk, en.n - e0);
    const size_t rec_bytes = (size_t)m * kRec, list_bytes = (size_t)m * 2 * sizeof(int);
    if (state_stage_reserve(b, rec_bytes + list_bytes, rec_bytes + list_bytes) != 0) return -1;
    int *list = reinterpret_cast<int *>(b->st_h + rec_bytes);
    for (int i = 0; i < m; i++) { list[2 * i] = en.ch(e0 + i); list[2 * i + 1] = i; }
    HIPCHK(hipMemcpyAsync(b->st_d + rec_bytes, list, list_bytes, hipMemcpyHostToDevice, b->stream));
    if (asdr_launch_state_gather(&a, reinterpret_cast<const int *>(b->st_d + rec_bytes), m, 0, 0, b->st_d, nullptr, b->stream) != 0) return fail("state gather kernel launch failed");
    HIPCHK(hipMemcpyAsync(b->st_h, b->st_d, rec_bytes, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < m; i++) {
      uint8_t *r = out + (size_t)en.rec(e0 + i) * kRec;
      const Chan &c = b->ch[en.ch(e0 + i)];
      memcpy(r + kCtl, b->st_h + (size_t)i * kRec + kCtl, kRec - kCtl);
      control_to_record(c, content, r);
    }
  }
  return 0;
}

int export_device(const StateEntries &en, void *d_records, void *stream_) {
  asdr_batch *b = en.b;
  if (b->device == ASDR_NO_DEVICE) return fail("control-plane-only batch (ASDR_NO_DEVICE) has no device: use asdr_export_state");
  hipStream_t stream = (stream_ == ASDR_STREAM_BATCH) ? b->stream : (hipStream_t)stream_;
  HIPCHK(hipSetDevice(b->device));
  if (state_apply_resets(b) != 0) return -1;
  const uint32_t content = state_content(b);
  const size_t ctl_bytes = (size_t)en.n * kCtl, list_bytes = en.pairs.empty() ? 0 : (size_t)en.n * 2 * sizeof(int);
  if (state_stage_reserve(b, ctl_bytes + list_bytes, ctl_bytes + list_bytes) != 0) return -1;
  for (int e = 0; e < en.n; e++) { const Chan &c = b->ch[en.ch(e)]; control_to_record(c, content, b->st_h + (size_t)e * kCtl); }
  if (list_bytes) memcpy(b->st_h + ctl_bytes, en.pairs.data(), list_bytes);
  if (state_order_in(b, stream) != 0) return -1;
  HIPCHK(hipMemcpyAsync(b->st_d, b->st_h, ctl_bytes + list_bytes, hipMemcpyHostToDevice, stream));
  UpdateArgs a;
  fill_args(b, a);
  if (asdr_launch_state_gather(&a, list_bytes ? reinterpret_cast<const int *>(b->st_d + ctl_bytes) : nullptr, en.n, en.ch0, en.rec0, d_records, b->st_d, stream) != 0)
    return fail("state gather kernel launch failed");
  HIPCHK(hipEventRecord(b->st_ev, stream)); b->st_ev_pending = true;
  state_order_out(b, stream);
  return 0;
}

// host half of an import (every record has been checked): members, dirty marks, reset bits
void import_host_half(const StateEntries &en, const uint8_t *ctl, size_t ctl_stride) {
  asdr_batch *b = en.b;
  for (int e = 0; e < en.n; e++) {
    const int ch = en.ch(e);
    const uint8_t *p = ctl + (size_t)en.rec(e) * ctl_stride;
    uint32_t content; memcpy(&content, p + 12, 4);
    record_to_chan(b, ch, p);
    mark_dirty(b, ch);
    b->reset[ch] = 0u;   // the next update's reset pass must not wipe what this call loads
    if (!(content & ASDR_STATE_HAS_SIGNAL)) mark_reset(b, ch, ASDR_R_ALL);   // a control-only record: the signal state at power-on
  }
}

bool any_signal(const StateEntries &en, const uint8_t *ctl, size_t ctl_stride) {
  for (int e = 0; e < en.n; e++) { uint32_t content; memcpy(&content, ctl + (size_t)en.rec(e) * ctl_stride + 12, 4); if (content & ASDR_STATE_HAS_SIGNAL) return true; }
  return false;
}

int import_host(const StateEntries &en, const uint8_t *in) {
  asdr_batch *b = en.b;
  if (b->device != ASDR_NO_DEVICE && any_signal(en, in, kRec)) {
    HIPCHK(hipSetDevice(b->device));
    if (sync_all(b) != 0) return -1;
    if (check_stream_error(b) != 0) return -1;
    UpdateArgs a;
    fill_args(b, a);
    for (int e0 = 0; e0 < en.n; e0 += kStateChunk) {
      const int m = std::min(kStateChunk, en.n - e0);
      const size_t rec_bytes = (size_t)m * kRec, list_bytes = (size_t)m * 2 * sizeof(int);
      if (state_stage_reserve(b, rec_bytes + list_bytes, rec_bytes + list_bytes) != 0) return -1;
      int *list = reinterpret_cast<int *>(b->st_h + rec_bytes);
      for (int i = 0; i < m; i++) { memcpy(b->st_h + (size_t)i * kRec, in + (size_t)en.rec(e0 + i) * kRec, kRec); list[2 * i] = en.ch(e0 + i); list[2 * i + 1] = i; }
      HIPCHK(hipMemcpyAsync(b->st_d, b->st_h, rec_bytes + list_bytes, hipMemcpyHostToDevice, b->stream));
      if (asdr_launch_state_scatter(&a, reinterpret_cast<const int *>(b->st_d + rec_bytes), m, 0, 0, b->st_d, b->stream) != 0) return fail("state scatter kernel launch failed");
      HIPCHK(hipStreamSynchronize(b->stream));
    }
  }
  import_host_half(en, in, kRec);
  return 0;
}

// `ctl`: the records' first kCtl bytes as the caller's array has them, already on the host ([record index][kCtl])
int import_device(const StateEntries &en, const void *d_records, const uint8_t *ctl, hipStream_t stream) {
  asdr_batch *b = en.b;
  if (any_signal(en, ctl, kCtl)) {
    HIPCHK(hipSetDevice(b->device));
    const size_t list_bytes = en.pairs.empty() ? 0 : (size_t)en.n * 2 * sizeof(int);
    if (list_bytes) {
      if (state_stage_reserve(b, list_bytes, list_bytes) != 0) return -1;
      memcpy(b->st_h, en.pairs.data(), list_bytes);
    }
    if (state_order_in(b, stream) != 0) return -1;
    if (list_bytes) HIPCHK(hipMemcpyAsync(b->st_d, b->st_h, list_bytes, hipMemcpyHostToDevice, stream));
    UpdateArgs a;
    fill_args(b, a);
    if (asdr_launch_state_scatter(&a, list_bytes ? reinterpret_cast<const int *>(b->st_d) : nullptr, en.n, en.ch0, en.rec0, d_records, stream) != 0)
      return fail("state scatter kernel launch failed");
    if (list_bytes) { HIPCHK(hipEventRecord(b->st_ev, stream)); b->st_ev_pending = true; }
    state_order_out(b, stream);
  }
  import_host_half(en, ctl, kCtl);
  return 0;
}

// index checks of a call, and its entries by owner
int state_route(asdr_batch *b, const int *channels, int n, bool no_duplicates, std::vector<StateEntries> &out) {
  if (n > b->n && no_duplicates) return fail("more records than channels: a destination would be named twice");
  if (channels) {
    std::vector<uint8_t> seen(no_duplicates ? (size_t)b->n : 0, 0);
    for (int i = 0; i < n; i++) {
      const int c = channels[i];
      if (c < 0 || c >= b->n) return fail("record " + std::to_string(i) + ": channel " + std::to_string(c) + " out of range (0.." + std::to_string(b->n - 1) + ")");
      if (no_duplicates) { if (seen[c]) return fail("record " + std::to_string(i) + ": channel " + std::to_string(c) + " named twice"); seen[c] = 1; }
    }
  } else if (n > b->n) return fail("n exceeds the batch's channel count (channels == NULL names channels 0 .. n-1)");
  out.clear();
  if (!is_sharded(b)) {
    StateEntries en; en.b = b; en.n = n;
    if (channels) { en.pairs.resize(2 * (size_t)n); for (int i = 0; i < n; i++) { en.pairs[2 * (size_t)i] = channels[i]; en.pairs[2 * (size_t)i + 1] = i; } }
    out.push_back(std::move(en));
    return 0;
  }
  out.resize(b->shards.size());
  for (size_t g = 0; g < b->shards.size(); g++) {
    StateEntries &en = out[g];
    en.b = b->shards[g];
    if (!channels) { const int lo = b->shard_first[g], hi = std::min(b->shard_first[g + 1], n); en.n = std::max(0, hi - lo); en.ch0 = 0; en.rec0 = lo; }
  }
  if (channels) for (int i = 0; i < n; i++) {
    int local = channels[i];
    const std::vector<int> &f = b->shard_first;
    const int g = (int)(std::upper_bound(f.begin(), f.end(), local) - f.begin()) - 1;
    local -= f[g];
    out[g].pairs.push_back(local); out[g].pairs.push_back(i); out[g].n++;
  }
  return 0;
}

int state_one_device(asdr_batch *b) {   // the rule of asdr_update_device_strided: device pointers belong to ONE device
  if (!is_sharded(b)) return b->device == ASDR_NO_DEVICE ? fail("control-plane-only batch (ASDR_NO_DEVICE) has no device: use the host form") : 0;
  for (asdr_batch *sh : b->shards) if (sh->device != b->shards[0]->device || sh->device == ASDR_NO_DEVICE)
    return fail("sharded batch over several devices: device-resident records go to the shards (asdr_shard), host records to asdr_export_state / asdr_import_state");
  return 0;
}

}  // namespace

extern "C" {

size_t asdr_state_record_bytes(void) { return kRec; }

const char *asdr_state_record_field(int i, int *offset, int *count) {
  if (i < 0 || i >= (int)(sizeof kStateFields / sizeof kStateFields[0])) return nullptr;
  if (offset) *offset = kStateFields[i].offset;
  if (count) *count = kStateFields[i].count;
  return kStateFields[i].name;
}

int asdr_export_state(asdr_batch_t *b, const int *channels, int n, void *host_records) {
  if (!b) return fail("null batch");
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  if (!host_records) return fail("null records");
  std::vector<StateEntries> parts;
  if (state_route(b, channels, n, false, parts) != 0) return -1;
  for (const StateEntries &en : parts) if (en.n > 0 && export_host(en, static_cast<uint8_t *>(host_records)) != 0) return -1;
  return 0;
}

int asdr_export_state_device(asdr_batch_t *b, const int *channels, int n, void *d_records, void *stream) {
  if (!b) return fail("null batch");
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  if (!d_records || ((uintptr_t)d_records & 15u) != 0) return fail("device records: null or not 16-byte aligned");
  if (state_one_device(b) != 0) return -1;
  std::vector<StateEntries> parts;
  if (state_route(b, channels, n, false, parts) != 0) return -1;
  for (const StateEntries &en : parts) if (en.n > 0 && export_device(en, d_records, stream) != 0) return -1;
  return 0;
}

int asdr_import_state(asdr_batch_t *b, const int *channels, int n, const void *host_records) {
  if (!b) return fail("null batch");
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  if (!host_records) return fail("null records");
  std::vector<StateEntries> parts;
  if (state_route(b, channels, n, true, parts) != 0) return -1;
  const uint8_t *in = static_cast<const uint8_t *>(host_records);
  for (int i = 0; i < n; i++) {   // every record, before anything is written
    const char *why = check_record(in + (size_t)i * kRec);
    if (why) return fail("record " + std::to_string(i) + " (channel " + std::to_string(channels ? channels[i] : i) + "): " + why);
  }
  for (const StateEntries &en : parts) if (en.n > 0 && import_host(en, in) != 0) return -1;
  return 0;
}

int asdr_import_state_device(asdr_batch_t *b, const int *channels, int n, const void *d_records, void *stream_) {
  if (!b) return fail("null batch");
  if (n < 0) return fail("n < 0");
  if (n == 0) return 0;
  if (!d_records || ((uintptr_t)d_records & 15u) != 0) return fail("device records: null or not 16-byte aligned");
  if (state_one_device(b) != 0) return -1;
  std::vector<StateEntries> parts;
  if (state_route(b, channels, n, true, parts) != 0) return -1;
  asdr_batch *b0 = is_sharded(b) ? b->shards[0] : b;
  hipStream_t stream = (stream_ == ASDR_STREAM_BATCH) ? b0->stream : (hipStream_t)stream_;
  HIPCHK(hipSetDevice(b0->device));
  // header + control part of every record to the host: validated before any launch (this waits for the work in front of it on `stream`)
  std::vector<uint8_t> ctl((size_t)n * kCtl);
  HIPCHK(hipMemcpy2DAsync(ctl.data(), kCtl, d_records, kRec, kCtl, (size_t)n, hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int i = 0; i < n; i++) {
    const char *why = check_record(ctl.data() + (size_t)i * kCtl);
    if (why) return fail("record " + std::to_string(i) + " (channel " + std::to_string(channels ? channels[i] : i) + "): " + why);
  }
  for (const StateEntries &en : parts) if (en.n > 0 && import_device(en, d_records, ctl.data(), stream) != 0) return -1;
  return 0;
}

}  // extern "C"
