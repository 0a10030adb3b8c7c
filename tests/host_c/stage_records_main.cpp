// stage_records_main.cpp -- StageRecords, StageMirror and stage_check_block_rows of audiosdr_amd/csrc/asdr_stage_host.h against plain
// loops, as a stand-alone host program for tests/test_stage_records_host.py to build with -fsanitize=address,undefined and run.
// The HIP functions the header names come from tools/host_trace_stub.cpp, which carries memory operations out on host memory: an
// ASDR_NO_DEVICE handle never reaches them; the handles with a "device" here keep their records in a host buffer, so that the
// chunked transfers of fill and rewrite run under the sanitizers too.  No GPU is touched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "asdr_stage_host.h"

static std::string g_error;
int asdr_internal_fail(const std::string &m) { g_error = m; return -1; }

#define CHECK(cond)                                                               \
  do {                                                                            \
    if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

struct Small { uint32_t id; uint8_t fill[44]; };    // 48 bytes, as asdr_fm_state_t
struct Large { uint32_t id; uint8_t fill[700]; };   // 704 bytes, as asdr_tone_state_t
static_assert(sizeof(Small) == 48 && sizeof(Large) == 704, "the record sizes of the FM demodulator and the tone squelch");

template <class Rec>
Rec record(uint32_t id, uint8_t v) {
  Rec r;
  r.id = id;
  std::memset(r.fill, v, sizeof(r.fill));
  return r;
}

template <class Rec>
bool same(const std::vector<Rec> &a, const std::vector<Rec> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(Rec)) == 0;
}

// every operation of the record holder on a handle of n channels; `device` is ASDR_NO_DEVICE or 0 (records in a host buffer)
template <class Rec>
void records(int n, int device) {
  StageDev d;
  d.n = n; d.device = device;
  StageRecords<Rec> st;
  std::vector<Rec> backing(device == ASDR_NO_DEVICE ? 0 : n);
  if (device != ASDR_NO_DEVICE) st.dev = backing.data();
  std::vector<Rec> want(n), got(n);

  CHECK(st.fill(d, record<Rec>(7, 0xA5)) == 0);
  for (Rec &r : want) r = record<Rec>(7, 0xA5);
  CHECK(st.read(d, got.data()) == 0 && same(want, got));
  CHECK(st.read(d, nullptr) == -1 && g_error == "null destination");

  uint32_t next = 0;
  CHECK(st.rewrite(d, [&](Rec &r) { r.id = next++; r.fill[3] ^= 0xFF; }) == 0);
  for (int k = 0; k < n; k++) { want[k].id = (uint32_t)k; want[k].fill[3] ^= 0xFF; }
  CHECK(next == (uint32_t)n && st.read(d, got.data()) == 0 && same(want, got));

  // without a list: the first m channels
  const int m = n > 1 ? n - 1 : 1;
  std::vector<Rec> src(n);
  for (int k = 0; k < n; k++) src[k] = record<Rec>(1000 + k, (uint8_t)k);
  CHECK(st.write(d, nullptr, m, src.data()) == 0);
  for (int k = 0; k < m; k++) want[k] = src[k];
  CHECK(st.read(d, got.data()) == 0 && same(want, got));
  CHECK(st.write(d, nullptr, n + 1, src.data()) == -1 && g_error == "more records than channels");
  CHECK(st.write(d, nullptr, -1, src.data()) == -1 && g_error == "negative record count");
  CHECK(st.write(d, nullptr, 1, nullptr) == -1 && g_error == "null source");
  CHECK(st.write(d, nullptr, 0, nullptr) == 0);

  // with a list: record k to channels[k], in any order
  std::vector<int> ch;
  for (int k = n - 1; k >= 0; k -= 2) ch.push_back(k);
  for (size_t k = 0; k < ch.size(); k++) { src[k] = record<Rec>(2000 + (uint32_t)k, 0x3C); want[ch[k]] = src[k]; }
  CHECK(st.write(d, ch.data(), (int)ch.size(), src.data()) == 0);
  CHECK(st.read(d, got.data()) == 0 && same(want, got));

  // refused lists write nothing: a bad channel at the last position, and a record the stage's check refuses
  for (size_t k = 0; k < ch.size(); k++) src[k] = record<Rec>(3000, 0x11);
  const int last = ch.back();
  for (int bad : {n, -1}) {
    ch.back() = bad;
    CHECK(st.write(d, ch.data(), (int)ch.size(), src.data()) == -1);
    CHECK(g_error == "record " + std::to_string(ch.size() - 1) + ": bad channel");
    CHECK(st.read(d, got.data()) == 0 && same(want, got));
  }
  ch.back() = last;
  int seen = 0;
  auto refuse_last = [&](int k, const Rec &r) { seen++; return r.id == 3000 && k + 1 == (int)ch.size() ? asdr_internal_fail("refused") : 0; };
  CHECK(st.write(d, ch.data(), (int)ch.size(), src.data(), refuse_last) == -1 && g_error == "refused" && seen == (int)ch.size());
  CHECK(st.read(d, got.data()) == 0 && same(want, got));

  CHECK(st.zero(d) == 0);
  std::memset((void *)want.data(), 0, want.size() * sizeof(Rec));
  CHECK(st.read(d, got.data()) == 0 && same(want, got));
}

template <class Set>
void mirror(int n) {
  StageMirror<Set> mi;
  mi.host.assign(n, record<Set>(0, 0));
  std::vector<Set> want(n, record<Set>(0, 0)), dev(n, record<Set>(9, 9));
  mi.dev = dev.data();
  CHECK(mi.dirty);                                       // a new mirror is pushed by the first call
  CHECK(mi.push(nullptr) == 0 && !mi.dirty && same(want, dev));

  mi.apply(n - 1, [](Set &s) { s.id = 5; s.fill[0] = 1; });
  want[n - 1].id = 5; want[n - 1].fill[0] = 1;
  CHECK(mi.dirty && same(want, mi.host) && mi[n - 1].id == 5);
  CHECK(!same(want, dev));                               // only push moves it
  CHECK(mi.push(nullptr) == 0 && !mi.dirty && same(want, dev));

  mi.apply(ASDR_ALL, [](Set &s) { s.fill[1] = 2; });
  for (Set &s : want) s.fill[1] = 2;
  CHECK(mi.dirty && same(want, mi.host));
  dev[0].id = 77;                                        // a clean mirror is not pushed again
  CHECK(mi.push(nullptr) == 0 && mi.push(nullptr) == 0 && same(want, dev));
  dev[0].id = 77;
  CHECK(mi.push(nullptr) == 0 && dev[0].id == 77);
}

// the order of the block-row refusals, on host addresses (nothing is dereferenced)
void block_rows() {
  alignas(16) static int16_t a[2 * 4 * 128], b[2 * 4 * 128];
  const char *text = "output span overlaps the input span";
  auto check = [&](const void *in, long si, const void *out, long so, int n_blocks) {
    g_error.clear();
    return stage_check_block_rows({{in}, 2, si}, {{out}, 2, so}, n_blocks, text);
  };
  CHECK(check(a, 4, b, 4, 4) == 0 && g_error.empty());
  CHECK(check(nullptr, 1, b, 1, -1) == -1 && g_error == "null device pointer");
  CHECK(check(a + 1, 1, b, 4, 70000) == -1 && g_error == "n_blocks must be in 0..65535");
  CHECK(check(a + 1, 4, b, 3, 4) == -1 && g_error == "row stride shorter than n_blocks");
  CHECK(check(a + 1, 4, b, (1L << 30) + 1, 4) == -1 && g_error == "row stride too large");
  CHECK(check(a, 4, a + 1, 4, 4) == -1 && g_error == "device pointers must be 16-byte aligned");
  CHECK(check(a, 4, a + 128, 4, 4) == -1 && g_error == text);
  CHECK(check(a, 4, a, 4, 0) == 0 && g_error.empty());   // nothing to do: no overlap test
  CHECK(check(a, 4, a + 2 * 4 * 128 - 8, 4, 4) == -1);   // the last 16 bytes of the span
  g_error.clear();
  CHECK(stage_check_block_rows({{a}, 2, 4}, {}, 4, nullptr) == 0 && g_error.empty());            // a call that writes no rows
  CHECK(stage_check_block_rows({{a}, 2, 3}, {}, 4, nullptr) == -1 && g_error == "row stride shorter than n_blocks");
  CHECK(stage_check_block_rows({{a, b}, 2, 4}, {{b + 128}, 2, 4}, 4, "an input span") == -1 && g_error == "an input span");   // the second input

  StageDev d;
  d.n = 2;
  CHECK(stage_check_channel(nullptr, 0, true, "null thing") == -1 && g_error == "null thing");
  CHECK(stage_check_channel(&d, ASDR_ALL, true, "null thing") == 0 && stage_check_channel(&d, 1, false, "null thing") == 0);
  CHECK(stage_check_channel(&d, ASDR_ALL, false, "null thing") == -1 && g_error == "bad channel");
  CHECK(stage_check_channel(&d, 2, true, "null thing") == -1 && stage_check_channel(&d, -2, true, "null thing") == -1);
}

int main() {
  for (int n : {1, 2, 5}) {
    records<Small>(n, ASDR_NO_DEVICE);
    records<Large>(n, ASDR_NO_DEVICE);
    mirror<Small>(n);
    mirror<Large>(n);
  }
  // one chunk exactly, one record more, and two chunks and a rest: the transfers of fill and rewrite
  for (int n : {3, 4096, 4097, 2 * 4096 + 5}) {
    records<Small>(n, 0);
    records<Large>(n, 0);
  }
  block_rows();
  std::puts("stage records ok");
  return 0;
}
