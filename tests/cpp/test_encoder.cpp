// test_encoder.cpp -- gmix_amd/csrc/gmx_encoder.h built for the host (tests/test_encoder_cpu.py compiles and runs it):
//   test_encoder <dir> <case>...
// Per case <dir>/<case>.{bits,p,state,count,out,start}: replays the recorded run of the reference's Encoder state by
// state and byte by byte, flushes, compares the whole output, and -- from the constructor's state -- decodes its own
// output with gmx_coder_decode back to the bits.  Then 10^6 random tuples of state, p and bit against the reference's
// loop spelled out: a bit never emits more than 4 bytes, a flush returns 1..5.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "gmx_encoder.h"

template <class T>
static std::vector<T> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

static int fail(const char* what, const std::string& name, size_t t) {
  printf("FAIL: %s %s at %zu\n", name.c_str(), what, t);
  return 1;
}

static int run_case(const std::string& dir, const std::string& name) {
  const std::string base = dir + "/" + name;
  const auto bits = slurp<uint8_t>(base + ".bits");
  const auto p = slurp<float>(base + ".p");
  const auto state = slurp<uint32_t>(base + ".state");
  const auto count = slurp<uint32_t>(base + ".count");
  const auto want = slurp<uint8_t>(base + ".out");
  const auto start = slurp<uint32_t>(base + ".start");
  const size_t n = bits.size();
  if (!n || p.size() != n || state.size() != 2 * n || count.size() != n || start.size() != 2) return fail("inputs", name, 0);
  GmxEncoderState st = {start[0], start[1]};
  std::vector<uint8_t> out;
  uint32_t hist[5] = {0, 0, 0, 0, 0};
  for (size_t t = 0; t < n; ++t) {
    if (!gmx_encoder_p_ok(p[t])) return fail("p outside the domain", name, t);
    uint8_t buf[8];
    const uint32_t k = gmx_encoder_bit(&st, bits[t], p[t], buf);
    if (k > 4) return fail("more than 4 bytes", name, t);
    ++hist[k];
    out.insert(out.end(), buf, buf + k);
    if (st.x1 != state[2 * t] || st.x2 != state[2 * t + 1]) return fail("state", name, t);
    if (out.size() != count[t]) return fail("byte count", name, t);
    if (memcmp(out.data(), want.data(), out.size()) != 0) return fail("bytes", name, t);
  }
  uint8_t buf[8];
  const uint32_t k = gmx_encoder_flush(&st, buf);
  if (k < 1 || k > 5) return fail("flush count", name, n);
  out.insert(out.end(), buf, buf + k);
  if (out != want) return fail("output after Flush", name, n);
  size_t decoded = 0;
  if (start[0] == 0u && start[1] == 0xffffffffu) {
    GmxCoderState ds;
    gmx_coder_init(&ds, out.data(), (uint32_t)out.size());
    for (size_t t = 0; t < n; ++t, ++decoded)
      if (gmx_coder_decode(&ds, p[t], out.data(), (uint32_t)out.size()) != (bits[t] ? 1u : 0u)) return fail("decode", name, t);
  }
  printf("ok: %s %zu bits, %zu bytes, emits %u/%u/%u/%u/%u, %zu bits decoded back\n", name.c_str(), n, out.size(), hist[0],
         hist[1], hist[2], hist[3], hist[4], decoded);
  return 0;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}

// Encoder::Encode and Flush as the reference spells them
static uint32_t plain_loop(uint32_t& x1, uint32_t& x2, uint8_t* out) {
  uint32_t k = 0;
  while (((x1 ^ x2) & 0xff000000u) == 0) {
    out[k++] = (uint8_t)(x2 >> 24);
    x1 <<= 8;
    x2 = (x2 << 8) + 255;
    if (k > 8) break;
  }
  return k;
}

static int random_tuples() {
  const float special[] = {0.0f, 1.0f, 0.5f, 0.0001f, 1.0f - 0.0001f};
  uint32_t hist[5] = {0, 0, 0, 0, 0}, fh[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 1000000; ++i) {
    uint32_t x1 = rnd(), x2 = rnd();
    const uint32_t mode = rnd() % 4;
    if (mode == 1) x2 = x1 + (rnd() & 0xffffu);      // narrow ranges: the long emits
    if (mode == 2) x2 = x1 ^ (1u << (rnd() % 32));
    const uint32_t sel = rnd() % 8, bit = rnd() & 1u;
    const float p = sel < 5 ? special[sel] : (float)(rnd() >> 8) / 16777216.0f;
    GmxEncoderState st = {x1, x2};
    uint8_t a[8], b[8];
    const uint32_t k = gmx_encoder_bit(&st, bit, p, a);
    const uint32_t pr = (uint32_t)(1.0f + 65534.0f * p);
    const uint32_t xmid = x1 + ((x2 - x1) >> 16) * pr + (((x2 - x1) & 0xffff) * pr >> 16);
    if (bit)
      x2 = xmid;
    else
      x1 = xmid + 1;
    const uint32_t kp = plain_loop(x1, x2, b);
    if (k > 4 || k != kp || memcmp(a, b, k) != 0 || st.x1 != x1 || st.x2 != x2) return fail("random tuple", "bit", (size_t)i);
    ++hist[k];
    GmxEncoderState fs = {rnd(), rnd()};
    if (mode == 1) fs.x2 = fs.x1 ^ (rnd() & 0xffffu);
    uint32_t f1 = fs.x1, f2 = fs.x2;
    const uint32_t fk = gmx_encoder_flush(&fs, a);
    uint32_t fp = plain_loop(f1, f2, b);
    b[fp++] = (uint8_t)(f2 >> 24);
    if (fk < 1 || fk > 5 || fk != fp || memcmp(a, b, fk) != 0 || fs.x1 != f1 || fs.x2 != f2) return fail("random tuple", "flush", (size_t)i);
    ++fh[fk];
  }
  printf("ok: tuples emits %u/%u/%u/%u/%u, flushes %u/%u/%u/%u/%u\n", hist[0], hist[1], hist[2], hist[3], hist[4], fh[1], fh[2],
         fh[3], fh[4], fh[5]);
  return (hist[4] && fh[5]) ? 0 : fail("no long emit among the tuples", "tuples", 0);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  for (int i = 2; i < argc; ++i)
    if (run_case(argv[1], argv[i])) return 1;
  return random_tuples();
}
