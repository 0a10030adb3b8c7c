// host_trace_driver.cpp -- the scenarios of tools/host_trace.py: every launch form of the receiver batch's device-call dispatcher
// (asdr_host.cpp), driven through the C ABI against the recording stubs of host_trace_stub.cpp.
//
//   host_trace --list          the scenario names
//   host_trace <scenario>      run one scenario; the trace goes to stdout
//
// One scenario per process: the stream pool, the lanes' probe and the environment switches are per process.  Lines that begin with
// '#' are the driver's own: `#call` in front of every update call, `#layout` behind it (what the schedule looks like: the launch-plan
// test reads the slot counts there).  Banks are small; the thresholds between the launch forms are lowered through the public switches.
// Where a switch has a floor (asdr_set_lanes: 16 waves) or none exists (the lanes' probe, the pipeline's headroom rule) the bank is as
// large as the rule needs -- on the stub's arena that costs address space only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "asdr.h"

extern "C" void host_trace_malloc_budget(long n);   // host_trace_stub.cpp

namespace {

asdr_batch_t *b = nullptr;
int n = 0, cap_blocks = 0;
int16_t *dI = nullptr, *dQ = nullptr, *dOut = nullptr;
hipStream_t s1 = nullptr, s2 = nullptr;

#define OK(call) do { if ((call) != 0) { fprintf(stderr, "%s failed: %s\n", #call, asdr_last_error()); exit(2); } } while (0)

void buffers(int blocks) {
  cap_blocks = blocks;
  const size_t bytes = (size_t)n * blocks * 128 * sizeof(int16_t);
  if (hipMalloc((void **)&dI, bytes) != hipSuccess || hipMalloc((void **)&dQ, bytes) != hipSuccess || hipMalloc((void **)&dOut, bytes) != hipSuccess) exit(2);
  if (hipStreamCreateWithFlags(&s1, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&s2, hipStreamNonBlocking) != hipSuccess) exit(2);
}
void create(int channels, int blocks) {
  n = channels;
  b = asdr_create(n, 0);
  if (!b) { fprintf(stderr, "asdr_create failed: %s\n", asdr_last_error()); exit(2); }
  buffers(blocks);
}
void layout() {
  for (int g = 0; g < asdr_n_shards(b); g++) {
    asdr_batch_t *sh = asdr_shard(b, g);
    int o[8];
    OK(asdr_schedule_layout(sh, o));
    printf("#layout shard=%d slots=%d kinds=%d,%d,%d,%d,%d left=%d left_kind=%d forms=%d\n", g, asdr_debug_schedule(sh, nullptr, 0), o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
  }
}
const char *sn(void *s) { return s == ASDR_STREAM_BATCH ? "batch" : s == (void *)s1 ? "s1" : s == (void *)s2 ? "s2" : "null"; }
void call_io(const int16_t *i, const int16_t *q, int16_t *o, int blocks, void *stream) {
  printf("#call device n_blocks=%d stream=%s in_place=%d\n", blocks, sn(stream), o == i);
  OK(asdr_update_device(b, i, q, o, blocks, stream));
  layout();
}
void call(int blocks, void *stream = ASDR_STREAM_BATCH) { call_io(dI, dQ, dOut, blocks, stream); }

// channel kinds
void sam(int c0, int c1) { for (int c = c0; c < c1; c++) asdr_setDemodMode(b, c, ASDR_SAMmode); }
void usb(int c0, int c1) { for (int c = c0; c < c1; c++) asdr_setDemodMode(b, c, ASDR_USBmode); }
void als_small(int c0, int c1) { for (int c = c0; c < c1; c++) asdr_enableALSfilter(b, c); }   // 55 taps, delay 3: the compact rows
void als_long(int c0, int c1) { for (int c = c0; c < c1; c++) { asdr_enableALSfilter(b, c); asdr_setALSfilterParams(b, c, 100, 0.5f, 3.0f); } }
// plain, SAM and short-ALS whole waves plus remainders of three kinds: several sub-ranges, several helper streams
void mixed(int blocks) {
  create(64, blocks);
  sam(24, 40); als_small(40, 56); usb(56, 59); sam(59, 61); als_long(61, 64);
}
void all_sam(int blocks) { create(64, blocks); asdr_setDemodMode(b, ASDR_ALL, ASDR_SAMmode); OK(asdr_set_sam_launch_form(b, 0, 8)); }
void all_als(int blocks) { create(64, blocks); asdr_enableALSfilter(b, ASDR_ALL); }
void finish() { OK(asdr_synchronize(b)); asdr_destroy(b); b = nullptr; }

// ---- 1-3: ordinary sub-range launches ----
void sc_mixed_blocks() { mixed(3); call(1); call(3); call(1, s1); call(3, s1); finish(); }
void sc_mixed_setters() {
  mixed(3);
  call(1, s1); asdr_setOutputGain(b, 5, 0.25f); call(1, s1); asdr_init(b, 7); call(3, s1);
  asdr_setDemodMode(b, 3, ASDR_AMmode); call(3, s1); asdr_setNoiseBlankerThreshold(b, ASDR_ALL, 1.5f); call(1, s1);
  finish();
}
void sc_mixed_streams() { mixed(3); call(1, s1); call(1, s2); call(3); call(3, s1); call(1, nullptr); call(1); finish(); }
// ---- 4: one launch per block, through the three-launch SAM form; the taps are the last block's ----
void sc_per_block() {
  mixed(3); OK(asdr_set_sam_launch_form(b, 0, 8));
  call(3, s1); call(1, s1); OK(asdr_enable_taps(b, 1)); call(3, s1); call(2, s1); OK(asdr_enable_taps(b, 0)); call(2, s1);
  finish();
}
// ---- 5: lanes ----
void lanes_bank(int lanes, bool with_sam) {
  create(with_sam ? 160 : 131, 4);
  if (with_sam) { sam(128, 152); usb(152, 155); OK(asdr_set_sam_launch_form(b, 0, 8)); } else usb(128, 131);
  OK(asdr_set_lanes(b, lanes, 1));
}
void sc_lanes2_batch() { lanes_bank(1, false); call(1); call(1); call(1); call(4); call(1); finish(); }
void sc_lanes3_batch() { lanes_bank(3, false); call(1); call(1); call(4); call(1); finish(); }
void sc_lanes2_caller() { lanes_bank(1, true); call(4, s1); call(4, s1); call(2, s1); call(1, s1); call(4, s2); finish(); }
void sc_lanes3_caller() { lanes_bank(3, true); call(4, s1); call(4, s1); call(4); call(1); call(4, s1); finish(); }
void sc_lanes_join() { lanes_bank(1, false); call(1); call(1); call(1, s1); call(1); call(1); call(4, s1); call(1); finish(); }
void sc_lanes_setter() { lanes_bank(1, false); call(1); call(1); asdr_setOutputGain(b, 9, 0.75f); call(1); call(1); asdr_init(b, 3); call(1, s1); call(1); finish(); }
void sc_lanes_probe() { create(8192, 2); call(1); call(1); call(2); call(1, s1); call(1); finish(); }   // unforced: the overlap probe runs at the first lane-sized call
// ---- 6: the block pipeline ----
void pipeline_side(int blocks) { create(64, blocks); sam(48, 56); usb(56, 59); als_long(59, 61); }
void sc_pipeline_alone() {
  create(64, 19); call(8, s1); call(19, s1); OK(asdr_set_stream_fir_helpers(b, 0)); call(8, s1); OK(asdr_set_stream_fir_helpers(b, 1)); call(19, s1); call(3, s1); call(8);
  finish();
}
void sc_pipeline_side() {
  pipeline_side(19); call(8, s1); call(19, s1); OK(asdr_set_stream_fir_helpers(b, 0)); call(19, s1); OK(asdr_set_stream_fir_helpers(b, 1)); call(8, s1); call(1, s1);
  finish();
}
void sc_pipeline_in_place() { pipeline_side(8); call(8, s1); call_io(dI, dQ, dI, 8, s1); call_io(dI, dQ, dQ, 8, s1); call(8, s1); finish(); }
void sc_pipeline_max_groups() { create(64, 8); call(8, s1); OK(asdr_debug_set_stream_max_groups(b, 2)); call(8, s1); OK(asdr_debug_set_stream_max_groups(b, 8)); call(8, s1); OK(asdr_set_stream_pipeline(b, 0)); call(8, s1); finish(); }
void sc_pipeline_headroom() { create(4059, 8); usb(4056, 4059); call(8, s1); call(8, s1); finish(); }   // 507 groups + a side wave: past the margin
// ---- 7: SAM role streams ----
void sc_sam_roles_blocks() { all_sam(15); call(2, s1); call(3, s1); call(15, s1); call(1, s1); call(2); finish(); }
void sc_sam_roles_chunks() { all_sam(43); call(16, s1); call(19, s1); call(43, s1); call(16); finish(); }
void sc_sam_roles_no_chunks() { setenv("ASDR_NO_SAM_CHUNKS", "1", 1); all_sam(19); call(16, s1); call(19, s1); finish(); }
void sc_sam_als_roles() { create(64, 16); asdr_setDemodMode(b, ASDR_ALL, ASDR_SAMmode); asdr_enableALSfilter(b, ASDR_ALL); OK(asdr_set_sam_launch_form(b, 0, 8)); call(3, s1); call(16, s1); finish(); }
// ---- 8: ALS role streams ----
void als_roles() { all_als(19); call(2, s1); call(8, s1); call(19, s1); call_io(dI, dQ, dI, 8, s1); call(1, s1); call(8); finish(); }
void sc_als_roles_3() { als_roles(); }
void sc_als_roles_2() { setenv("ASDR_ALS_ROLE_STAGES", "2", 1); als_roles(); }
// ---- the forms that allocate at first use step aside when they cannot ----
void sc_alloc_failures_pipeline() { create(64, 8); call(1, s1); host_trace_malloc_budget(2); call(8, s1); host_trace_malloc_budget(-1); call(8, s1); finish(); }
void sc_alloc_failures_als() {
  all_als(8); call(1, s1); host_trace_malloc_budget(0); call(8, s1); host_trace_malloc_budget(1); call(8, s1); host_trace_malloc_budget(-1); call(8, s1);
  finish();
}
void sc_alloc_failures_sam() { all_sam(16); call(1, s1); host_trace_malloc_budget(0); call(16, s1); host_trace_malloc_budget(-1); call(16, s1); finish(); }
// ---- 9: chain | filter ----
void sc_als_split() { mixed(3); OK(asdr_set_als_launch_form(b, 8)); call(1, s1); call(3, s1); OK(asdr_enable_taps(b, 1)); call(3, s1); finish(); }
// ---- 10: launch split ----
void sc_split_direct() { create(64, 3); OK(asdr_set_launch_split(b, 2, 8)); call(1, s1); call(3, s1); OK(asdr_set_launch_split(b, 4, 8)); call(1, s1); call(3, s1); finish(); }
void sc_split_groups() { create(64, 3); usb(32, 64); OK(asdr_set_launch_split(b, 2, 8)); call(1, s1); call(3, s1); OK(asdr_set_launch_split(b, 4, 8)); call(1, s1); call(3, s1); finish(); }
void sc_split_per_block() { create(72, 3); sam(64, 72); OK(asdr_set_sam_launch_form(b, 0, 8)); OK(asdr_set_launch_split(b, 4, 8)); call(3, s1); call(2, s1); finish(); }
// ---- 11: host rows ----
void host_rows(int chunks, bool pinned, int blocks) {
  const size_t bytes = (size_t)n * blocks * 128 * sizeof(int16_t);
  int16_t *h[3];
  for (int i = 0; i < 3; i++) { h[i] = (int16_t *)(pinned ? asdr_host_alloc(bytes) : calloc(bytes, 1)); if (!h[i]) exit(2); }
  OK(asdr_set_host_chunks(b, chunks));
  printf("#call host n_blocks=%d chunks=%d pinned=%d\n", blocks, chunks, pinned);
  OK(asdr_update(b, h[0], h[1], h[2], blocks));
  layout();
  for (int i = 0; i < 3; i++) { if (pinned) asdr_host_free(h[i]); else free(h[i]); }
}
void sc_host_rows() {
  mixed(3);
  host_rows(1, true, 1); host_rows(2, true, 3); host_rows(4, true, 2); host_rows(2, false, 1); call(1, s1); host_rows(4, true, 1); host_rows(0, true, 1);
  finish();
}
void sc_host_rows_sam() { mixed(3); OK(asdr_set_sam_launch_form(b, 0, 8)); host_rows(2, true, 3); host_rows(4, true, 3); host_rows(1, true, 2); finish(); }
// ---- 12: timing ----
void sc_timing() {
  mixed(3);
  OK(asdr_set_launch_timing(b, 1)); call(1, s1); (void)asdr_last_kernel_ms(b); call(3, s1); host_rows(2, true, 1); OK(asdr_set_launch_timing(b, 0));
  float ms[8]; OK(asdr_kernel_timing_begin(b, 2)); call(1, s1); call(3, s1); call(1, s1); if (asdr_kernel_timing_end(b, ms, 8) != 2) exit(2);
  float total = 0; long calls = 0;
  OK(asdr_region_timing_begin(b, s1)); call(1, s1); call(3, s1); OK(asdr_region_timing_end(b, &total, &calls)); if (calls != 2) exit(2);
  finish();
}
void sc_timing_pipeline() {
  create(64, 8);
  OK(asdr_set_launch_timing(b, 1)); call(8, s1); (void)asdr_last_kernel_ms(b); OK(asdr_set_launch_timing(b, 0));
  float ms[4]; OK(asdr_kernel_timing_begin(b, 1)); call(8, s1); if (asdr_kernel_timing_end(b, ms, 4) != 1) exit(2);
  float total = 0; long calls = 0;
  OK(asdr_region_timing_begin(b, s1)); call(8, s1); OK(asdr_region_timing_end(b, &total, &calls)); if (calls != 1) exit(2);
  finish();
}
void sc_timing_lanes() {
  lanes_bank(1, false);
  float total = 0; long calls = 0;
  call(1); OK(asdr_region_timing_begin(b, ASDR_STREAM_BATCH)); call(1); call(1); call(1, s1); OK(asdr_region_timing_end(b, &total, &calls)); if (calls != 3) exit(2);
  OK(asdr_set_launch_timing(b, 1)); call(1); OK(asdr_set_launch_timing(b, 0)); call(1);
  finish();
}
// ---- 13: alternating order ----
void sc_alternate_order() {
  create(72, 3); sam(64, 72); OK(asdr_set_sam_launch_form(b, 0, 8)); OK(asdr_set_alternate_order(b, 1));
  call(1, s1); call(1, s1); call(3, s1); call(2, s1); call(1, s1); call(3, s1); call(1, s1);
  if (asdr_reversed_launches(b) <= 0) exit(2);
  finish();
}
void sc_alternate_order_lanes() {
  lanes_bank(1, true); OK(asdr_set_alternate_order(b, 1));
  call(1); call(1); call(1); call(3, s1); call(1); call(4, s1); call(1);
  finish();
}
// ---- 14: shards of one device, strided rows ----
void sc_sharded_strided() {
  n = 60;
  const int dev[3] = {0, 0, 0};
  b = asdr_create_sharded(n, 3, dev);
  if (!b) exit(2);
  buffers(5);
  sam(8, 16); als_small(30, 38); usb(57, 60);
  for (int blocks : {3, 1, 2}) {
    printf("#call device n_blocks=%d stream=s1 in_place=0\n", blocks);
    OK(asdr_update_device_strided(b, dI, dQ, dOut, blocks, 5, 5, s1));
    layout();
  }
  finish();
}
// ---- 15: the capture sink ----
void sc_capture() {
  mixed(3);
  OK(asdr_capture_open(b, 10));
  for (int blocks : {3, 1, 3}) {
    printf("#call device n_blocks=%d stream=s1 in_place=0\n", blocks);
    OK(asdr_capture_update_device(b, dI, dQ, blocks, 3, s1));
    layout();
  }
  OK(asdr_capture_close(b));
  finish();
}

const struct { const char *name; void (*run)(); } kScenarios[] = {
  {"mixed_blocks", sc_mixed_blocks}, {"mixed_setters", sc_mixed_setters}, {"mixed_streams", sc_mixed_streams}, {"per_block", sc_per_block},
  {"lanes2_batch", sc_lanes2_batch}, {"lanes3_batch", sc_lanes3_batch}, {"lanes2_caller", sc_lanes2_caller}, {"lanes3_caller", sc_lanes3_caller},
  {"lanes_join", sc_lanes_join}, {"lanes_setter", sc_lanes_setter}, {"lanes_probe", sc_lanes_probe},
  {"pipeline_alone", sc_pipeline_alone}, {"pipeline_side", sc_pipeline_side}, {"pipeline_in_place", sc_pipeline_in_place},
  {"pipeline_max_groups", sc_pipeline_max_groups}, {"pipeline_headroom", sc_pipeline_headroom},
  {"sam_roles_blocks", sc_sam_roles_blocks}, {"sam_roles_chunks", sc_sam_roles_chunks}, {"sam_roles_no_chunks", sc_sam_roles_no_chunks}, {"sam_als_roles", sc_sam_als_roles},
  {"als_roles_3", sc_als_roles_3}, {"als_roles_2", sc_als_roles_2}, {"als_split", sc_als_split},
  {"alloc_failures_pipeline", sc_alloc_failures_pipeline}, {"alloc_failures_als", sc_alloc_failures_als}, {"alloc_failures_sam", sc_alloc_failures_sam},
  {"split_direct", sc_split_direct}, {"split_groups", sc_split_groups}, {"split_per_block", sc_split_per_block},
  {"host_rows", sc_host_rows}, {"host_rows_sam", sc_host_rows_sam},
  {"timing", sc_timing}, {"timing_pipeline", sc_timing_pipeline}, {"timing_lanes", sc_timing_lanes},
  {"alternate_order", sc_alternate_order}, {"alternate_order_lanes", sc_alternate_order_lanes},
  {"sharded_strided", sc_sharded_strided}, {"capture", sc_capture},
};

}  // namespace

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "--list") == 0) { for (const auto &s : kScenarios) puts(s.name); return 0; }
  if (argc == 2) for (const auto &s : kScenarios) if (strcmp(argv[1], s.name) == 0) { s.run(); return 0; }
  fprintf(stderr, "usage: host_trace --list | <scenario>\n");
  return 1;
}
