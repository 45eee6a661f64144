// The host's staging of the group checkpoints (gmix_amd/csrc/gmx_ckpt_stage.h) against a fake link that plays the
// device: transfers and kernels are queued and run only at wait() -- as late as a stream may run them -- or, in the
// second pass, at once -- as early as it may.  A pipeline that reads a host buffer before the wait that fills it, or
// hands one back to the device before it has been copied out, yields wrong bytes in one of the two.  No GPU, no HIP.
//   g++ -std=c++17 -Wall -I gmix_amd/csrc tests/cpp/test_ckpt_stage.cpp && ./a.out
#include "gmx_ckpt_stage.h"

#include <stdio.h>

#include <functional>
#include <string>

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// The device: one staging buffer, and a stream that runs what was queued in order.  The log takes one letter per
// operation: W wait, D download, U upload, and P / S for the caller's pack and scatter launches.
struct FakeLink {
  bool lazy;
  std::vector<uint8_t> dev;
  std::vector<std::function<void()>> queue;
  std::string log;
  void submit(char what, std::function<void()> op) {
    log += what;
    if (lazy)
      queue.push_back(op);
    else
      op();
  }
  int wait() {
    log += 'W';
    for (auto& op : queue) op();
    queue.clear();
    return 0;
  }
  int to_host(uint8_t* h, size_t bytes) {
    submit('D', [=] { memcpy(h, dev.data(), bytes); memset(dev.data(), 0xdd, dev.size()); });
    return 0;
  }
  int to_device(uint8_t* h, size_t bytes) {
    submit('U', [=] { memcpy(dev.data(), h, bytes); });
    return 0;
  }
};

// Allocations of the staging buffers: which were asked for, and that none shrinks.  (One byte more than asked for:
// no buffer of a call whose sections are all empty is a null pointer.)
static int g_dev_asked, g_host_asked;
static int grow(uint8_t*& p, size_t& cap, size_t bytes) {
  if (p && bytes <= cap) return 0;
  free(p);
  p = (uint8_t*)malloc(bytes + 1);
  cap = bytes;
  return p ? 0 : -2;
}
static int grow_dev(uint8_t*& p, size_t& cap, size_t bytes) { return ++g_dev_asked, grow(p, cap, bytes); }
static int grow_host(uint8_t*& p, size_t& cap, size_t bytes) { return ++g_host_asked, grow(p, cap, bytes); }

struct Case {
  const char* name;
  std::vector<size_t> sizes;  // bytes of every stream's section
  size_t cap;
  int max_streams;
  std::vector<int> bounds;  // what the plan must say
};

static uint8_t byte_of(size_t stream, size_t k) { return (uint8_t)(1 + 37 * stream + 11 * k); }

static int run(const Case& c, size_t off0, bool lazy) {
  const int count = (int)c.sizes.size();
  std::vector<size_t> off(1, off0);
  for (size_t b : c.sizes) off.push_back(off.back() + b);
  std::vector<uint8_t> image(off.back() + 1, 0xaa);  // the caller's buffer as a correct export leaves it
  for (int i = 0; i < count; ++i)
    for (size_t k = 0; k < c.sizes[i]; ++k) image[off[i] + k] = byte_of(i, k);

  // ---- the plan, against a restatement: fill a slice while the next stream fits, never leave one empty
  CkptPlan plan;
  CHECK(ckpt_plan(off.data(), count, c.cap, plan, c.max_streams));
  std::vector<int> bounds(1, 0);
  std::vector<size_t> shift;
  size_t in_slice = 0, max_slice = 0;
  for (int i = 0; i < count; ++i) {
    const bool full = i - bounds.back() >= c.max_streams || in_slice + c.sizes[i] > c.cap;
    if (i > bounds.back() && full) bounds.push_back(i), in_slice = 0;
    shift.push_back(in_slice);
    max_slice = std::max(max_slice, in_slice += c.sizes[i]);
  }
  bounds.push_back(count);
  CHECK(plan.sl == bounds && plan.sl == c.bounds);
  CHECK(plan.shift == shift && plan.max_slice == max_slice);
  const size_t n = plan.slices();

  // ---- the buffers: the second pinned one only for a call that has two slices in flight
  CkptStaging st;
  g_dev_asked = g_host_asked = 0;
  CHECK(st.grow(plan.max_slice, n, grow_dev, grow_host) == 0);
  CHECK(g_dev_asked == 1 && g_host_asked == (n > 1 ? 2 : 1) && st.n_host == g_host_asked);
  CHECK((st.host[1] != nullptr) == (n > 1) && st.dev_cap >= max_slice);
  const size_t cap0 = st.dev_cap;
  CHECK(st.grow(plan.max_slice / 2, 1, grow_dev, grow_host) == 0 && st.dev_cap == cap0 && st.n_host == 1);  // grow-only
  CHECK(st.grow(plan.max_slice, n, grow_dev, grow_host) == 0);
  FakeLink link{lazy, std::vector<uint8_t>(max_slice + 1, 0xdd), {}, ""};

  // ---- export: the pack launch of a slice writes its streams' sections where the plan's shifts put them
  std::vector<uint8_t> out(off.back() + 1, 0xaa);
  int rc = ckpt_export_slices(link, plan, off.data(), out.data(), st, [&](size_t s, int i0, int ns) -> int {
    if (i0 != plan.sl[s] || i0 + ns != plan.sl[s + 1]) return -1;
    link.submit('P', [&, i0, ns] {
      for (int i = i0; i < i0 + ns; ++i)
        for (size_t k = 0; k < c.sizes[i]; ++k) link.dev[plan.shift[i] + k] = byte_of(i, k);
    });
    return 0;
  });
  CHECK(rc == 0 && link.queue.empty());
  CHECK(out == image);
  std::string want = "PD";
  for (size_t s = 1; s < n; ++s) want += "WPD";
  CHECK(link.log == want + "W" && link.log.size() == 3 * n);

  // ---- import: the scatter launch of a slice reads them there
  link.log.clear();
  std::vector<uint8_t> banks(off.back() + 1, 0xaa);
  rc = ckpt_import_slices(link, plan, off.data(), image.data(), st, [&](size_t s, int i0, int ns) -> int {
    if (i0 != plan.sl[s] || i0 + ns != plan.sl[s + 1]) return -1;
    link.submit('S', [&, i0, ns] {
      for (int i = i0; i < i0 + ns; ++i) memcpy(banks.data() + off[i], link.dev.data() + plan.shift[i], c.sizes[i]);
      memset(link.dev.data(), 0xdd, link.dev.size());
    });
    return 0;
  });
  CHECK(rc == 0 && link.queue.empty());
  CHECK(banks == image);
  want.clear();
  for (size_t s = 0; s < n; ++s) want += "WUS";
  CHECK(link.log == want + "W" && link.log.size() == 3 * n + 1);

  // ---- a status that is not 0 ends the call and is returned
  link.log.clear();
  CHECK(ckpt_export_slices(link, plan, off.data(), out.data(), st, [](size_t, int, int) { return -3; }) == -3);
  CHECK(ckpt_import_slices(link, plan, off.data(), image.data(), st, [](size_t, int, int) { return -3; }) == -3);
  CHECK(link.log == "WU");
  link.wait();
  free(st.dev);
  free(st.host[0]);
  free(st.host[1]);
  return 0;
}

int main() {
  const Case cases[] = {
      {"one slice", {5, 7, 3}, 100, kCkptMaxSliceStreams, {0, 3}},
      {"two slices", {40, 40, 40}, 80, kCkptMaxSliceStreams, {0, 2, 3}},
      {"three slices", {10, 10, 10}, 10, kCkptMaxSliceStreams, {0, 1, 2, 3}},
      {"five slices", {8, 9, 7, 10, 6, 4}, 10, kCkptMaxSliceStreams, {0, 1, 2, 3, 4, 6}},
      {"a stream above the cap", {3, 50, 3}, 10, kCkptMaxSliceStreams, {0, 1, 2, 3}},
      {"empty sections, one slice", {0, 6, 0, 0, 5, 0}, 11, kCkptMaxSliceStreams, {0, 6}},
      {"empty sections, an empty slice in front", {0, 6, 0, 0, 5, 0}, 5, kCkptMaxSliceStreams, {0, 1, 2, 6}},
      {"empty sections only", {0, 0, 0}, 4, kCkptMaxSliceStreams, {0, 3}},
      {"the stream-count limit", {1, 1, 1, 1, 1}, 100, 2, {0, 2, 4, 5}},
  };
  for (const Case& c : cases) {
    for (size_t off0 : {(size_t)0, (size_t)13})  // (import allows a first offset that is not 0)
      for (bool lazy : {true, false})
        if (run(c, off0, lazy)) {
          fprintf(stderr, "failed: %s, off[0] = %zu, %s link\n", c.name, off0, lazy ? "lazy" : "eager");
          return 1;
        }
    printf("ok: %s\n", c.name);
  }
  return 0;
}
