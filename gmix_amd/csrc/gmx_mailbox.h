// gmx_mailbox.h -- the host's half of the mailbox protocol of the persistent per-bit / per-byte sessions.
//
// One persistent wave (the mixers', gmx_stock.hip; the Indirect models', gmx_indirect.hip; the LSTM's, gmx_lstm.hip)
// polls a command word.  The host writes a payload, then the word (seq << 4 | payload slot << 3 | command, release);
// the wave answers by writing its results, then the same word into done_seq.  At most one command is outstanding.
// A wave that saw no command for kIdleTicks leaves with `state` != running, and whoever waits for an answer restarts
// it; a wave that does not answer within the time-out is given up for good (`dead`).  The layouts of the payloads,
// the kernels and the HIP objects of a session are the banks' own (gmx_session.inc, gmx_indirect.inc, gmx_lstm.inc):
// nothing here needs HIP, so that a thread can play the wave (tests/cpp/test_mailbox.cpp).
#ifndef GMX_MAILBOX_H_
#define GMX_MAILBOX_H_

#include <stdint.h>
#include <time.h>

#include <atomic>

// The words of the protocol that the host's half needs; gmx_internal.h has them for the kernels as GMX_MB_*, and
// gmx_session.inc checks that the two agree.
static const uint32_t kMbStop = 4u, kMbSlotShift = 3, kMbSeqShift = 4;
static const uint32_t kMbRunning = 0u, kMbExitIdle = 1u;

static const unsigned long long kIdleTicks = 2ull * 1000 * 1000;  // 20 ms of s_memrealtime (100 MHz)
static const int kMaxOpenSessions = 3;
static std::atomic<int> g_open_sessions{0};

// Stores to the command block may be write-combined (BAR mapping): make them globally visible,
// in order, before the command word follows.
static inline void mb_store_fence() {
#if defined(__x86_64__)
  __builtin_ia32_sfence();
#else
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}

static inline uint32_t mb_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }

struct GmxMailbox {
  uint32_t* cmd_seq = nullptr;   // the command word: first word of the command block
  uint32_t* done_seq = nullptr;  // last completed command word: first word of the reply block ...
  uint32_t* state = nullptr;     // ... and kMbRunning / how the wave left, right behind it
  uint32_t seq = 0;              // sequence number of the newest command
  uint32_t word = 0;             // its command word
  bool launched = false;         // an instance was started and not yet known to have left
  bool dead = false;             // its wave stopped answering: every later call fails at once
};

// The next command word; the doorbell is rung by mb_ring -- or, for a chained forward of the mixers, by the wave of
// the Indirect models once it has put its predictions into the payload.
static inline void mb_next_word(GmxMailbox* m, uint32_t slot, uint32_t cmd) {
  m->seq += 1;
  m->word = (m->seq << kMbSeqShift) | (slot << kMbSlotShift) | cmd;
}
static inline void mb_ring(GmxMailbox* m) {
  mb_store_fence();
  __atomic_store_n(m->cmd_seq, m->word, __ATOMIC_RELEASE);
  mb_store_fence();
}
static inline void mb_publish(GmxMailbox* m, uint32_t slot, uint32_t cmd) {
  mb_next_word(m, slot, cmd);
  mb_ring(m);
}
// A STOP names no payload: its word keeps the slot bit of the command before it.
static inline void mb_publish_stop(GmxMailbox* m) { mb_publish(m, (m->word >> kMbSlotShift) & 1u, kMbStop); }

static const int kMbDead = 1;  // mb_wait: the session is dead (no status of the library is positive)

// Wait until the newest command has been completed.  A wave that left before it saw the command is restarted:
// `restart()` starts the next instance and returns 0, or a status that ends the wait and is returned as it is.
// After more than timeout_s seconds without an answer the session is given up for good -- one stall, not one per
// later call: a STOP is published for a wave that may still be there, the session's place in the count of open
// sessions is given back, and this and every later wait return kMbDead.
template <class Restart>
static int mb_wait(GmxMailbox* m, long timeout_s, Restart&& restart) {
  if (m->dead) return kMbDead;
  uint64_t spins = 0;
  timespec t_start = {0, 0};
  while (mb_load(m->done_seq) != m->word) {
    if ((++spins & 0xff) == 0) {
      if (mb_load(m->state) != kMbRunning && mb_load(m->done_seq) != m->word) {
        int rc = restart();  // it left before it saw the command: the next one will
        if (rc) return rc;
      }
      timespec now;
      clock_gettime(CLOCK_MONOTONIC, &now);
      if (spins == 0x100) t_start = now;
      if (now.tv_sec - t_start.tv_sec > timeout_s) {
        mb_publish_stop(m);
        m->dead = true;
        if (m->launched) g_open_sessions.fetch_sub(1);
        m->launched = false;
        return kMbDead;
      }
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return 0;
}

#endif  // GMX_MAILBOX_H_
