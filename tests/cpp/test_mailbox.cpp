// The host's half of the session mailbox protocol (gmix_amd/csrc/gmx_mailbox.h) against a std::thread that plays the
// persistent wave: ordering of payload and command word, restart after an idle exit, the bounded wait of a session
// whose wave does not answer, and the STOP that the next instance must not take for a command.  No GPU, no HIP.
//   g++ -std=c++17 -O1 -pthread -I gmix_amd/csrc tests/cpp/test_mailbox.cpp && ./a.out
#include "gmx_mailbox.h"

#include <stdio.h>
#include <string.h>

#include <chrono>
#include <thread>

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// The same shape as the banks' blocks: the command word first, two payload slots; done_seq, state, the answer.
struct Cmd {
  uint32_t cmd_seq;
  uint32_t pad[15];
  uint32_t payload[2][4];
};
struct Reply {
  uint32_t done_seq;
  uint32_t state;
  uint32_t echo[4];
};
static const uint32_t kForward = 1u, kExitStop = 2u;

static uint32_t echo_of(uint32_t v, uint32_t word) { return v * 2654435761u + word; }

// One instance of the wave.  Like the kernels it takes a command word for new when it differs from done_seq as it
// found it.  `idle_after`: it leaves "on its idle timer" once it has answered that many commands (0: at once, before
// it looks at the command word; < 0: never, only a STOP ends it).
static void wave(Cmd* c, Reply* r, int idle_after) {
  uint32_t last = __atomic_load_n(&r->done_seq, __ATOMIC_ACQUIRE);
  for (int answered = 0; idle_after < 0 || answered < idle_after;) {
    const uint32_t w = __atomic_load_n(&c->cmd_seq, __ATOMIC_ACQUIRE);
    if (w == last) {
      std::this_thread::yield();
      continue;
    }
    if ((w & 7u) == kMbStop) {
      __atomic_store_n(&r->state, kExitStop, __ATOMIC_RELEASE);
      __atomic_store_n(&r->done_seq, w, __ATOMIC_RELEASE);
      return;
    }
    const uint32_t* pay = c->payload[(w >> kMbSlotShift) & 1u];
    for (int i = 0; i < 4; ++i) r->echo[i] = echo_of(pay[i], w);
    __atomic_store_n(&r->done_seq, w, __ATOMIC_RELEASE);
    last = w;
    ++answered;
  }
  __atomic_store_n(&r->state, kMbExitIdle, __ATOMIC_RELEASE);
}

// What a bank's session is around the protocol state, with a thread for the stream.
struct Session : GmxMailbox {
  Cmd c;
  Reply r;
  std::thread t;
  int restarts = 0;
  Session() {
    memset(&c, 0, sizeof c);
    memset(&r, 0, sizeof r);
    cmd_seq = &c.cmd_seq;
    done_seq = &r.done_seq;
    state = &r.state;
  }
  ~Session() {  // (a failed CHECK on the way: let the thread end)
    if (t.joinable()) {
      mb_publish_stop(this);
      t.join();
    }
  }
  // the start prologue of the banks: the previous instance has left or is leaving
  void start(int idle_after) {
    if (launched) {
      t.join();
    } else {
      g_open_sessions.fetch_add(1);
    }
    __atomic_store_n(state, kMbRunning, __ATOMIC_RELEASE);
    launched = true;
    t = std::thread(wave, &c, &r, idle_after);
  }
  int wait(long timeout_s = 10) {
    return mb_wait(this, timeout_s, [this] {
      ++restarts;
      start(-1);
      return 0;
    });
  }
  void put(uint32_t slot, uint32_t v) {
    for (uint32_t i = 0; i < 4; ++i) c.payload[slot][i] = v + i;  // plain stores, before the doorbell
  }
  bool echo_is(uint32_t v) const {
    for (uint32_t i = 0; i < 4; ++i)
      if (r.echo[i] != echo_of(v + i, word)) return false;
    return true;
  }
  // the stop sequence of the banks
  int stop() {
    if (!launched) return 0;
    int rc = wait();
    if (rc) return rc;
    if (mb_load(state) == kMbRunning) mb_publish_stop(this);
    t.join();
    __atomic_store_n(done_seq, word, __ATOMIC_RELEASE);
    launched = false;
    g_open_sessions.fetch_sub(1);
    return 0;
  }
};

static double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

static int test_ordering() {
  Session s;
  s.start(-1);
  for (uint32_t i = 0; i < 10000; ++i) {
    const uint32_t slot = i & 1u;
    s.put(slot, i * 4);
    mb_publish(&s, slot, kForward);
    CHECK(s.word == (((i + 1) << kMbSeqShift) | (slot << kMbSlotShift) | kForward));
    CHECK(s.wait() == 0);
    CHECK(s.echo_is(i * 4));
  }
  CHECK(s.restarts == 0);
  CHECK(s.stop() == 0);
  CHECK(g_open_sessions.load() == 0);
  return 0;
}

static int test_idle_exit_before_the_command() {
  Session s;
  s.start(0);
  while (mb_load(s.state) == kMbRunning) std::this_thread::yield();  // it has left; nobody has noticed yet
  s.put(0, 77);
  mb_publish(&s, 0, kForward);
  CHECK(s.wait() == 0);
  CHECK(s.restarts == 1);
  CHECK(s.echo_is(77));
  CHECK(g_open_sessions.load() == 1);  // a restart is the same session
  CHECK(s.stop() == 0);
  CHECK(g_open_sessions.load() == 0);
  return 0;
}

static int test_idle_exit_after_answering() {
  Session s;
  for (uint32_t i = 0; i < 200; ++i) {  // (the wave's exit races with the wait: many rounds)
    s.start(1);
    s.put(i & 1u, i);
    mb_publish(&s, i & 1u, kForward);
    if (i & 2u)
      while (mb_load(s.state) == kMbRunning) std::this_thread::yield();  // ... and rounds where it has left for sure
    CHECK(s.wait() == 0);
    CHECK(s.echo_is(i));
    CHECK(s.restarts == 0);
  }
  CHECK(s.stop() == 0);  // (a STOP published while the wave was leaving is never seen: stop marks it consumed)
  CHECK(mb_load(s.done_seq) == s.word);
  CHECK(g_open_sessions.load() == 0);
  return 0;
}

static int test_no_wave_at_all() {
  Session s;
  const int before = g_open_sessions.load();
  g_open_sessions.fetch_add(1);  // launched, running as far as anybody can tell -- and never answers
  s.launched = true;
  s.put(1, 5);
  mb_publish(&s, 1, kForward);
  auto t0 = std::chrono::steady_clock::now();
  CHECK(s.wait(1) == kMbDead);
  const double dt = seconds_since(t0);
  CHECK(dt > 1.0 && dt < 5.0);
  CHECK(s.restarts == 0);
  CHECK((mb_load(s.cmd_seq) & 7u) == kMbStop && mb_load(s.cmd_seq) == s.word);
  CHECK(s.dead && !s.launched);
  CHECK(g_open_sessions.load() == before);
  t0 = std::chrono::steady_clock::now();
  CHECK(s.wait(1) == kMbDead);
  CHECK(seconds_since(t0) < 0.5);
  CHECK(g_open_sessions.load() == before);
  return 0;
}

static int test_stop() {
  Session s;
  s.start(-1);
  s.put(0, 9);
  mb_publish(&s, 0, kForward);
  CHECK(s.stop() == 0);
  CHECK((s.word & 7u) == kMbStop);
  CHECK(mb_load(s.done_seq) == s.word && mb_load(s.cmd_seq) == s.word);
  CHECK(mb_load(s.state) == kExitStop);
  CHECK(g_open_sessions.load() == 0);
  // the next instance finds the STOP in the command word and must wait for something newer (had it taken the STOP
  // it would have left, and the wait below would have had to restart it)
  s.start(-1);
  CHECK(g_open_sessions.load() == 1);
  s.put(1, 11);
  mb_publish(&s, 1, kForward);
  CHECK(s.wait() == 0);
  CHECK(s.echo_is(11));
  CHECK(s.restarts == 0 && mb_load(s.state) == kMbRunning);
  CHECK(s.stop() == 0);
  CHECK(g_open_sessions.load() == 0);
  return 0;
}

int main() {
  struct {
    const char* name;
    int (*fn)();
  } tests[] = {{"ordering", test_ordering},
               {"idle exit before the command is seen", test_idle_exit_before_the_command},
               {"idle exit after answering", test_idle_exit_after_answering},
               {"no wave at all", test_no_wave_at_all},
               {"stop", test_stop}};
  for (auto& t : tests) {
    if (t.fn()) {
      fprintf(stderr, "FAILED: %s\n", t.name);
      return 1;
    }
    printf("ok: %s\n", t.name);
  }
  return 0;
}
