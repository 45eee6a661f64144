// gmx_ckpt_stage.h -- the host's staging of a group checkpoint: the one copy that gmx_group_export / _import
// (gmx_ckpt.inc), gmx_indirect_group_export / _import (gmx_ind_ckpt.inc), gmx_ctx_group_export / _import
// (gmx_ctx_ckpt.inc) and gmx_lstm_group_export / _import (gmx_lstm_ckpt.inc: sections of one size, one pass per half)
// share.  Nothing here needs HIP: the device and the link to it are the caller's `link`, so that a fake one can play
// them (tests/cpp/test_ckpt_stage.cpp).
//
// The packed bytes pass through ONE device buffer and two pinned host buffers (used in turn, so the host's copy to or
// from the caller's memory runs beside the device's work on the next slice).  A group may fill most of HBM, so the
// device buffer does not grow with the group: the streams are processed in slices of consecutive streams whose
// sections fit the cap together (64 MiB: large enough that a slice's transfer runs at the link's rate).  A slice is
// never less than one stream, so the buffer's upper bound is the larger of the cap and one stream's section.
// GMX_CKPT_STAGE_BYTES in the environment, read at every call, replaces the cap (tests: a few bytes make every stream
// a slice of its own).
//
// The Match group checkpoint (gmx_match_ckpt.inc) does not pass through here: its per-call arena holds the whole image
// and the call fails with GMX_ERR_NOMEM when that does not fit -- a contract its tests and documents assert.
#ifndef GMX_CKPT_STAGE_H_
#define GMX_CKPT_STAGE_H_

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

static const size_t kCkptStageBytes = 64u << 20;
static const int kCkptMaxSliceStreams = 32768;  // grid y / z of the kernels

static inline size_t ckpt_stage_cap() {
  const char* e = getenv("GMX_CKPT_STAGE_BYTES");
  if (e && *e) {
    const unsigned long long v = strtoull(e, nullptr, 10);
    if (v > 0) return (size_t)v;
  }
  return kCkptStageBytes;
}

// Slices of consecutive streams whose sections fit `cap` together; a slice is never less than one stream, nor more
// than `max_streams`.
static inline void ckpt_slices(const size_t* off, int count, size_t cap, std::vector<int>& bounds,
                               int max_streams = kCkptMaxSliceStreams) {
  bounds.assign(1, 0);
  for (int i0 = 0; i0 < count;) {
    int i1 = i0 + 1;
    while (i1 < count && i1 - i0 < max_streams && off[i1 + 1] - off[i0] <= cap) ++i1;
    bounds.push_back(i1);
    i0 = i1;
  }
}

// The slices of a call over sections off[0 .. count]: slice s is the streams [sl[s], sl[s + 1]) and lies in the
// staging buffers from byte 0, so an offset inside stream i's section becomes one inside its slice's buffer by adding
// shift[i].
struct CkptPlan {
  std::vector<int> sl;
  std::vector<size_t> shift;
  size_t max_slice = 0;
  size_t slices() const { return sl.size() - 1; }
  size_t bytes(const size_t* off, size_t s) const { return off[sl[s + 1]] - off[sl[s]]; }
};
// (false: out of host memory)
static inline bool ckpt_plan(const size_t* off, int count, size_t cap, CkptPlan& p,
                             int max_streams = kCkptMaxSliceStreams) {
  try {
    ckpt_slices(off, count, cap, p.sl, max_streams);
    p.shift.assign((size_t)count, 0);
  } catch (const std::bad_alloc&) {
    return false;
  }
  p.max_slice = 0;
  for (size_t s = 0; s < p.slices(); ++s) {
    p.max_slice = std::max(p.max_slice, p.bytes(off, s));
    for (int i = p.sl[s]; i < p.sl[s + 1]; ++i) p.shift[(size_t)i] = off[i] - off[p.sl[s]];
  }
  return true;
}

// One device buffer and two pinned host buffers, grow-only: the next checkpoint of the bank finds them.
struct CkptStaging {
  uint8_t* dev = nullptr;
  uint8_t* host[2] = {nullptr, nullptr};
  size_t dev_cap = 0, host_cap[2] = {0, 0};  // bytes
  int n_host = 1;                            // pinned buffers that the call at hand takes in turn

  // grow_dev / grow_host(pointer, capacity, bytes) make a buffer hold `bytes` and return a status, 0 for success.
  // A call of one slice never has two slices in flight: it asks for no second pinned buffer.
  template <class GrowDev, class GrowHost>
  int grow(size_t max_slice, size_t n_slices, GrowDev grow_dev, GrowHost grow_host) {
    n_host = n_slices > 1 ? 2 : 1;
    int rc = grow_dev(dev, dev_cap, max_slice);
    for (int h = 0; h < n_host && !rc; ++h) rc = grow_host(host[h], host_cap[h], max_slice);
    return rc;
  }
};

// The two pipelines.  `link` has wait() -- everything queued so far is done --, to_host(host, bytes) and
// to_device(host, bytes), which queue a transfer between a pinned buffer and the staging device buffer; pack(s, i0, n)
// and scatter(s, i0, n) queue the caller's kernels for slice s = streams [i0, i0 + n), writing or reading the device
// buffer.  All return a status, 0 for success; the first other one ends the call and is returned.
//
// Hazards.  The device buffer is one: slice s + 1 may be packed, or uploaded, only behind a wait that covers the
// transfer (export) or the scatter (import) of slice s.  The pinned buffers are two, taken in turn.  Export: the
// download of slice s + 1 goes to the other buffer while this one is copied out; the download of slice s + 2, which
// comes back to this one, is queued after that copy.  Import: the upload that last read host[s % 2] is two slices
// back, and the wait of slice s - 1 was behind it.

template <class Link, class Pack>
static int ckpt_export_slices(Link& link, const CkptPlan& p, const size_t* off, void* out, CkptStaging& st,
                              Pack&& pack) {
  const size_t n = p.slices();
  auto launch = [&](size_t s) -> int {
    const int rc = pack(s, p.sl[s], p.sl[s + 1] - p.sl[s]);
    return rc ? rc : link.to_host(st.host[s % st.n_host], p.bytes(off, s));
  };
  int rc = n ? launch(0) : 0;
  for (size_t s = 0; s < n && !rc; ++s) {
    if ((rc = link.wait())) break;
    if (s + 1 < n && (rc = launch(s + 1))) break;  // the next slice packs while this one is copied out
    memcpy((uint8_t*)out + off[p.sl[s]], st.host[s % st.n_host], p.bytes(off, s));
  }
  return rc;
}

template <class Link, class Scatter>
static int ckpt_import_slices(Link& link, const CkptPlan& p, const size_t* off, const void* in, CkptStaging& st,
                              Scatter&& scatter) {
  for (size_t s = 0; s < p.slices(); ++s) {
    uint8_t* const h = st.host[s % st.n_host];
    memcpy(h, (const uint8_t*)in + off[p.sl[s]], p.bytes(off, s));  // beside the device's work on the slice before
    int rc = link.wait();                                           // the device buffer is free again
    if (!rc) rc = link.to_device(h, p.bytes(off, s));
    if (!rc) rc = scatter(s, p.sl[s], p.sl[s + 1] - p.sl[s]);
    if (rc) return rc;
  }
  return link.wait();
}

#endif  // GMX_CKPT_STAGE_H_
