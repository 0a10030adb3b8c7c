// host_trace_stub.cpp -- the device side of libasdr_hip.so as a recorder, for tools/host_trace.py and tests/test_launch_plan.py.
//
// asdr_host.cpp compiled with a plain host compiler leaves undefined the HIP runtime functions it calls and the launchers of
// asdr_kernels.hip / asdr_state.hip.  This file defines them: every call appends one line to stdout, and the memory operations are
// carried out on host memory, so that the library's own read-backs (flush, resets, the pipeline's error word) work.  Two runs are
// comparable line by line:
//   - "device" memory is one zeroed bump arena mapped at a fixed address: a device address is logged as dev+<offset>, any other
//     address as `host`; hipFree gives nothing back (a scenario is one process);
//   - streams and events are small ordinals in order of creation (s0 = the null stream);
//   - hipEventElapsedTime answers 1 ms for every pair: the lanes' overlap probe then votes "concurrent";
//   - asdr_stream_capacity answers 1536 resident workgroups on 256 compute units for the one-helper form, 768 for the three-helper form;
//   - hipMalloc fails on request (host_trace_malloc_budget): the forms that allocate at first use step aside when they cannot;
//   - a launcher's line carries its scalar arguments, its stream, the fields of UpdateArgs the launch-plan test reads, and the whole
//     struct as bytes (fill_args zeroes it first, so the bytes are deterministic).
// No device is touched and nothing here is loaded into another process.
#include <hip/hip_runtime.h>

#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "asdr_device.h"

namespace {

constexpr uintptr_t kArenaBase = 0x600000000000ull;
constexpr size_t kArenaBytes = size_t(4) << 30;   // reserved, not committed: pages are zero until written
char *g_arena = nullptr;
size_t g_arena_used = 0;
std::mutex g_mu;   // (the host path's copy threads never call in here, the sharded host path's threads do)
std::vector<std::pair<const char *, size_t>> g_pinned;
int g_streams = 0, g_events = 0;
long g_malloc_budget = -1;   // hipMalloc calls that still succeed (host_trace_malloc_budget; -1: all)

void arena_init() {
  if (g_arena) return;
  void *p = mmap((void *)kArenaBase, kArenaBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE | MAP_FIXED_NOREPLACE, -1, 0);
  if (p != (void *)kArenaBase) { fprintf(stderr, "host_trace_stub: cannot map the arena at its fixed address\n"); exit(3); }
  g_arena = (char *)p;
}
std::string addr(const void *p) {
  const uintptr_t v = (uintptr_t)p;
  if (!p) return "null";
  if (v >= kArenaBase && v < kArenaBase + kArenaBytes) { char t[40]; snprintf(t, sizeof t, "dev+0x%zx", (size_t)(v - kArenaBase)); return t; }
  return "host";
}
// streams and events are never dereferenced by the library: an ordinal in a pointer's clothes
std::string sname(hipStream_t s) { return "s" + std::to_string((uintptr_t)s >> 4); }
std::string ename(hipEvent_t e) { return "e" + std::to_string((uintptr_t)e >> 4); }
const char *kind(hipMemcpyKind k) {
  return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : k == hipMemcpyHostToHost ? "H2H" : "default";
}
#define LOG(...) do { std::lock_guard<std::mutex> g_(g_mu); printf(__VA_ARGS__); putchar('\n'); } while (0)

std::string args(const UpdateArgs *a) {
  char head[512];
  snprintf(head, sizeof head, "sched=%s n_sched=%d in_i=%s out=%s n_blocks=%d nb_phase=%u als_phase=%u lo_parity=%u lo_write=%u lo_writer_bit=0x%x direct_ch0=%d run_if=%d taps=%d args=",
           addr(a->sched).c_str(), a->n_sched, addr(a->in_i).c_str(), addr(a->out).c_str(), a->n_blocks, a->nb_phase, a->als_phase, a->lo_parity, a->lo_write, a->lo_writer_bit,
           a->direct_ch0, a->run_if ? 1 : 0, a->taps ? 1 : 0);
  std::string s = head;
  static const char hex[] = "0123456789abcdef";
  const unsigned char *p = reinterpret_cast<const unsigned char *>(a);
  for (size_t i = 0; i < sizeof *a; i++) { s += hex[p[i] >> 4]; s += hex[p[i] & 15]; }
  return s;
}

}  // namespace

extern "C" {

// the driver's handle on the allocation-failure paths: the next `n` hipMalloc calls succeed, the ones after them fail (-1: all succeed)
void host_trace_malloc_budget(long n) { std::lock_guard<std::mutex> g(g_mu); g_malloc_budget = n; }

// ---- the HIP runtime ------------------------------------------------------------------------------------------------------------
hipError_t hipGetDeviceCount(int *n) { *n = 1; LOG("hipGetDeviceCount"); return hipSuccess; }
hipError_t hipSetDevice(int d) { LOG("hipSetDevice %d", d); return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; LOG("hipGetDevice"); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { LOG("hipDeviceSynchronize"); return hipSuccess; }
hipError_t hipGetLastError(void) { LOG("hipGetLastError"); return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "host_trace_stub"; }
hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest) { *least = 0; *greatest = -1; LOG("hipDeviceGetStreamPriorityRange"); return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int flags) {
  std::lock_guard<std::mutex> g(g_mu);
  *s = (hipStream_t)((uintptr_t)++g_streams << 4);
  printf("hipStreamCreateWithFlags -> s%d flags=%u\n", g_streams, flags);
  return hipSuccess;
}
hipError_t hipStreamCreateWithPriority(hipStream_t *s, unsigned int flags, int priority) {
  std::lock_guard<std::mutex> g(g_mu);
  *s = (hipStream_t)((uintptr_t)++g_streams << 4);
  printf("hipStreamCreateWithPriority -> s%d flags=%u priority=%d\n", g_streams, flags, priority);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { LOG("hipStreamSynchronize %s", sname(s).c_str()); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int flags) { LOG("hipStreamWaitEvent %s %s flags=%u", sname(s).c_str(), ename(e).c_str(), flags); return hipSuccess; }

hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned int flags) {
  std::lock_guard<std::mutex> g(g_mu);
  *e = (hipEvent_t)((uintptr_t)++g_events << 4);
  printf("hipEventCreateWithFlags -> e%d flags=%u\n", g_events, flags);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) {
  std::lock_guard<std::mutex> g(g_mu);
  *e = (hipEvent_t)((uintptr_t)++g_events << 4);
  printf("hipEventCreate -> e%d\n", g_events);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) { LOG("hipEventDestroy %s", ename(e).c_str()); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { LOG("hipEventRecord %s %s", ename(e).c_str(), sname(s).c_str()); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { LOG("hipEventSynchronize %s", ename(e).c_str()); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t e0, hipEvent_t e1) { *ms = 1.0f; LOG("hipEventElapsedTime %s %s", ename(e0).c_str(), ename(e1).c_str()); return hipSuccess; }

hipError_t hipMalloc(void **p, size_t bytes) {
  std::lock_guard<std::mutex> g(g_mu);
  arena_init();
  if (g_malloc_budget == 0) { printf("hipMalloc %zu -> refused\n", bytes); return hipErrorOutOfMemory; }
  if (g_malloc_budget > 0) g_malloc_budget--;
  const size_t at = (g_arena_used + 255) & ~size_t(255);
  if (at + bytes > kArenaBytes) { printf("hipMalloc %zu -> out of memory\n", bytes); return hipErrorOutOfMemory; }
  g_arena_used = at + bytes;
  *p = g_arena + at;
  printf("hipMalloc %zu -> dev+0x%zx\n", bytes, at);
  return hipSuccess;
}
hipError_t hipFree(void *p) { LOG("hipFree %s", addr(p).c_str()); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags) {
  *p = calloc(bytes ? bytes : 1, 1);
  std::lock_guard<std::mutex> g(g_mu);
  g_pinned.push_back({(const char *)*p, bytes});
  printf("hipHostMalloc %zu flags=%u\n", bytes, flags);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *p) {
  std::lock_guard<std::mutex> g(g_mu);
  for (size_t i = 0; i < g_pinned.size(); i++) if (g_pinned[i].first == p) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
  free(p);
  printf("hipHostFree\n");
  return hipSuccess;
}
hipError_t hipHostRegister(void *p, size_t bytes, unsigned int flags) {
  std::lock_guard<std::mutex> g(g_mu);
  g_pinned.push_back({(const char *)p, bytes});
  printf("hipHostRegister %zu flags=%u\n", bytes, flags);
  return hipSuccess;
}
hipError_t hipHostUnregister(void *p) {
  std::lock_guard<std::mutex> g(g_mu);
  for (size_t i = 0; i < g_pinned.size(); i++) if (g_pinned[i].first == p) { g_pinned.erase(g_pinned.begin() + (long)i); break; }
  printf("hipHostUnregister\n");
  return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *at, const void *p) {   // page-locked host memory, device memory, or an error (pageable)
  std::lock_guard<std::mutex> g(g_mu);
  memset(at, 0, sizeof *at);
  const char *q = (const char *)p;
  if (addr(p) != "host") { at->type = hipMemoryTypeDevice; printf("hipPointerGetAttributes %s -> device\n", addr(p).c_str()); return hipSuccess; }
  for (const auto &r : g_pinned) if (q >= r.first && q < r.first + r.second) { at->type = hipMemoryTypeHost; printf("hipPointerGetAttributes host -> pinned\n"); return hipSuccess; }
  printf("hipPointerGetAttributes host -> pageable\n");
  return hipErrorInvalidValue;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind k) {
  memcpy(dst, src, n);
  LOG("hipMemcpy %s <- %s %zu %s", addr(dst).c_str(), addr(src).c_str(), n, kind(k));
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind k, hipStream_t s) {
  memcpy(dst, src, n);
  LOG("hipMemcpyAsync %s <- %s %zu %s %s", addr(dst).c_str(), addr(src).c_str(), n, kind(k), sname(s).c_str());
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind k, hipStream_t s) {
  for (size_t r = 0; r < height; r++) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
  LOG("hipMemcpy2DAsync %s/%zu <- %s/%zu %zux%zu %s %s", addr(dst).c_str(), dpitch, addr(src).c_str(), spitch, width, height, kind(k), sname(s).c_str());
  return hipSuccess;
}
hipError_t hipMemset(void *dst, int v, size_t n) { memset(dst, v, n); LOG("hipMemset %s %d %zu", addr(dst).c_str(), v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t s) { memset(dst, v, n); LOG("hipMemsetAsync %s %d %zu %s", addr(dst).c_str(), v, n, sname(s).c_str()); return hipSuccess; }

// ---- the launchers of asdr_kernels.hip / asdr_state.hip -------------------------------------------------------------------------
int asdr_kernels_upload_tables(void) { LOG("asdr_kernels_upload_tables"); return 0; }
int asdr_stream_capacity(int device, int *compute_units, int fir_helpers) {
  if (compute_units) *compute_units = 256;
  LOG("asdr_stream_capacity device=%d fir_helpers=%d", device, fir_helpers);
  return fir_helpers == 3 ? 768 : 1536;
}
int asdr_launch_spin(unsigned long long ticks, hipStream_t s) { LOG("asdr_launch_spin %llu %s", ticks, sname(s).c_str()); return 0; }
int asdr_launch_update(const UpdateArgs *a, int variant, int uniform, hipStream_t s) {
  LOG("asdr_launch_update variant=%d uniform=%d role=- %s %s", variant, uniform, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_update_ordered(const UpdateArgs *a, int variant, int uniform, hipStream_t s, int *reversed) {
  if (reversed) *reversed = (a->wg_reverse && variant == ASDR_KERNEL_PLAIN && uniform == 1 && a->direct_ch0 >= 0 && a->n_blocks == 1) ? 1 : 0;
  LOG("asdr_launch_update_ordered variant=%d uniform=%d role=- %s %s", variant, uniform, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_sam_role(const UpdateArgs *a, int variant, int uniform, int role, hipStream_t s) {
  LOG("asdr_launch_sam_role variant=%d uniform=%d role=%d %s %s", variant, uniform, role, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_als_role(const UpdateArgs *a, int role, hipStream_t s) {
  LOG("asdr_launch_als_role variant=- uniform=- role=%d %s %s", role, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_als_stage_seed(const UpdateArgs *a, int ch0, int n, hipStream_t s) {
  LOG("asdr_launch_als_stage_seed ch0=%d n=%d %s %s", ch0, n, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_reset(const UpdateArgs *a, const uint32_t *d_reset_bits, int first_row, int n_rows, hipStream_t s) {
  LOG("asdr_launch_reset bits=%s first_row=%d n_rows=%d %s %s", addr(d_reset_bits).c_str(), first_row, n_rows, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_stream(const UpdateArgs *a, hipStream_t s, int fir_helpers) {
  LOG("asdr_launch_stream variant=- uniform=- role=h%d %s %s", fir_helpers, sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_stream_snapshot(const UpdateArgs *a, void *snap, int restore, hipStream_t s) {
  LOG("asdr_launch_stream_snapshot variant=- uniform=- role=%s %s snap=%s %s", restore ? "restore" : "snapshot", sname(s).c_str(), addr(snap).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_stream_ack(uint32_t *err, hipStream_t s) { LOG("asdr_launch_stream_ack %s %s", addr(err).c_str(), sname(s).c_str()); return 0; }
int asdr_launch_state_gather(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, void *records, const void *ctl, hipStream_t s) {
  LOG("asdr_launch_state_gather list=%s n=%d ch0=%d rec0=%d records=%s ctl=%s %s %s", addr(list).c_str(), n, ch0, rec0, addr(records).c_str(), addr(ctl).c_str(), sname(s).c_str(), args(a).c_str());
  return 0;
}
int asdr_launch_state_scatter(const UpdateArgs *a, const int *list, int n, int ch0, int rec0, const void *records, hipStream_t s) {
  LOG("asdr_launch_state_scatter list=%s n=%d ch0=%d rec0=%d records=%s %s %s", addr(list).c_str(), n, ch0, rec0, addr(records).c_str(), sname(s).c_str(), args(a).c_str());
  return 0;
}

}  // extern "C"
