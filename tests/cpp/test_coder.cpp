// test_coder.cpp -- gmix_amd/csrc/gmx_coder.h built for the host (tests/test_coder_cpu.py compiles and runs it):
//   1. decodes recorded traces: <dir>/<case>.in (compressed input), .p (float32 probabilities), .bits (expected bits)
//      and, where present, .state (x1, x2, x after every Decode, recorded from the reference's own Decoder);
//   2. resumes every trace from its state in the middle (Decoder::ReadCheckpoint plus the read position);
//   3. checks the PPMd range walk against a plain std::accumulate loop on distributions with zeros (denom == 0) and on
//      one that gives p == 0.5 exactly.
// usage: test_coder <dir> <case> [<case> ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "gmx_coder.h"

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (g_fail < 20) {                 \
        fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
        fprintf(stderr, __VA_ARGS__);    \
        fprintf(stderr, "\n");           \
      }                                  \
      ++g_fail;                          \
    }                                    \
  } while (0)

template <class T>
static bool read_file(const std::string& path, std::vector<T>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize((size_t)n / sizeof(T));
  const size_t got = n ? fread(out->data(), sizeof(T), out->size(), f) : 0;
  fclose(f);
  return got == out->size();
}

static void run_case(const std::string& dir, const std::string& name) {
  std::vector<uint8_t> in, bits;
  std::vector<float> p;
  std::vector<uint32_t> state;
  if (!read_file(dir + "/" + name + ".in", &in) || !read_file(dir + "/" + name + ".p", &p) ||
      !read_file(dir + "/" + name + ".bits", &bits)) {
    CHECK(false, "%s: missing files", name.c_str());
    return;
  }
  const bool has_state = read_file(dir + "/" + name + ".state", &state);
  const size_t T = p.size();
  CHECK(bits.size() == T && (!has_state || state.size() == 3 * T), "%s: sizes", name.c_str());
  if (bits.size() != T || (has_state && state.size() != 3 * T)) return;
  // (a copy of exactly the input's length: a read past its end is an address the sanitizer knows)
  std::vector<uint8_t> exact(in);
  const uint32_t n = (uint32_t)exact.size();
  GmxCoderState st;
  gmx_coder_init(&st, exact.data(), n);
  std::vector<GmxCoderState> trail(T);
  size_t past_end = 0, multi = 0;
  for (size_t t = 0; t < T; ++t) {
    const uint32_t before = st.pos;
    const bool dry = st.pos >= n;
    const uint32_t x1 = st.x1, x2 = st.x2;
    const uint32_t bit = gmx_coder_decode(&st, p[t], exact.data(), n);
    CHECK(bit == bits[t], "%s: bit %zu is %u", name.c_str(), t, bit);
    if (has_state)
      CHECK(st.x1 == state[3 * t] && st.x2 == state[3 * t + 1] && st.x == state[3 * t + 2],
            "%s: state after bit %zu: %08x %08x %08x, recorded %08x %08x %08x", name.c_str(), t, st.x1, st.x2, st.x,
            state[3 * t], state[3 * t + 1], state[3 * t + 2]);
    CHECK(st.pos <= n && st.pos - before <= 4, "%s: read position", name.c_str());
    // how many bytes this bit shifted: the same bit replayed from the same range over four spare bytes
    {
      const uint8_t zeros[4] = {0, 0, 0, 0};
      GmxCoderState r = {x1, x2, bit ? 0u : 0xffffffffu, 0};  // (x <= xmid iff the bit is 1)
      gmx_coder_decode(&r, p[t], zeros, 4);
      if (r.pos >= 2) ++multi;
      if (dry && r.pos > 0) ++past_end;
    }
    trail[t] = st;
  }
  // resume in the middle from {x1, x2, x, pos}
  for (size_t from : {T / 3, T / 2, T - 1}) {
    GmxCoderState r = trail[from - 1];
    for (size_t t = from; t < T; ++t) {
      const uint32_t bit = gmx_coder_decode(&r, p[t], exact.data(), n);
      CHECK(bit == bits[t] && r.x1 == trail[t].x1 && r.x2 == trail[t].x2 && r.x == trail[t].x && r.pos == trail[t].pos,
            "%s: resumed at %zu, bit %zu", name.c_str(), from, t);
    }
  }
  printf("ok: %s %zu bits, %u of %u input bytes read, %zu multi-byte shifts, %zu shifts past the end\n", name.c_str(), T,
         st.pos, n, multi, past_end);
}

// mod_ppmd.cpp:1662-1681 as it stands there
struct PlainWalk {
  int top = 255, mid = 127, bot = 0;
  bool step(const float* ppm, bool opens, int new_bit, float* p_out) {
    if (opens) {
      top = 255;
      bot = 0;
    } else {
      if (new_bit)
        bot = mid + 1;
      else
        top = mid;
    }
    mid = bot + ((top - bot) / 2);
    float num = std::accumulate(&ppm[mid + 1], &ppm[top + 1], 0.0f);
    float denom = std::accumulate(&ppm[bot], &ppm[mid + 1], num);
    if (denom != 0) {
      *p_out = num / denom;
      return true;
    }
    return false;
  }
};

static uint32_t f2u(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static void walk_distribution(const char* name, const float* ppm, size_t* silent, size_t* halves, size_t* writes) {
  for (int byte = 0; byte < 256; ++byte) {
    PlainWalk pw;
    GmxCoderWalk w;
    for (int j = 0; j < 8; ++j) {
      const int prev_bit = j ? (byte >> (8 - j)) & 1 : 0;
      float p = 0.0f;
      const bool wrote = pw.step(ppm, j == 0, prev_bit, &p);
      if (j == 0)
        gmx_coder_walk_open(&w);
      else
        gmx_coder_walk_bit(&w, (uint32_t)prev_bit);
      CHECK(w.top == pw.top && w.bot == pw.bot, "%s: range of byte %d bit %d", name, byte, j);
      float slot = -123.0f;
      bool active = true;
      const bool got = gmx_coder_walk_predict(&w, ppm, &slot, &active);
      CHECK(got == wrote, "%s: byte %d bit %d: wrote %d, plain loop %d", name, byte, j, (int)got, (int)wrote);
      if (!wrote) {
        CHECK(f2u(slot) == f2u(-123.0f) && active, "%s: a silent bit writes nothing", name);
        ++*silent;
        continue;
      }
      ++*writes;
      CHECK(f2u(slot) == f2u(gmx_logit(p)), "%s: byte %d bit %d: slot %08x, Logit(%a) = %08x", name, byte, j, f2u(slot),
            p, f2u(gmx_logit(p)));
      CHECK(active == (p != 0.5f), "%s: byte %d bit %d: active", name, byte, j);
      if (p == 0.5f) ++*halves;
    }
  }
}

static void walk_cases() {
  size_t silent = 0, halves = 0, writes = 0;
  float ppm[256];
  // uniform: every quotient is 128/256, 64/128, ... = 0.5 exactly
  for (float& v : ppm) v = 1.0f / 256;
  size_t s0 = 0, h0 = 0, w0 = 0;
  walk_distribution("uniform", ppm, &s0, &h0, &w0);
  CHECK(s0 == 0 && h0 == w0 && w0 == 256 * 8, "uniform: every bit is p == 0.5 (%zu of %zu)", h0, w0);
  // the upper half zero, the lower half ragged: denom == 0 everywhere above 127
  uint64_t r = 88172645463325252ull;
  auto rnd = [&r]() {
    r ^= r << 13;
    r ^= r >> 7;
    r ^= r << 17;
    return (float)((r >> 40) & 0xffff) / 65536.0f;
  };
  for (int i = 0; i < 256; ++i) ppm[i] = i < 128 ? rnd() + 1e-3f : 0.0f;
  size_t s1 = 0, h1 = 0, w1 = 0;
  walk_distribution("upper half zero", ppm, &s1, &h1, &w1);
  CHECK(s1 == 128 * 7, "upper half zero: %zu silent bits", s1);
  // zeros in runs of 1, 2, 4, ... scattered, values of very different magnitude (the order of the sums matters)
  for (int i = 0; i < 256; ++i) ppm[i] = rnd() * ((i % 7 == 0) ? 1e-7f : (i % 5 == 0) ? 1e3f : 1.0f);
  for (int at : {0, 16, 17, 32, 33, 34, 35, 64, 65, 66, 67, 68, 69, 70, 71, 200, 254, 255}) ppm[at] = 0.0f;
  size_t s2 = 0, h2 = 0, w2 = 0;
  walk_distribution("scattered zeros", ppm, &s2, &h2, &w2);
  CHECK(s2 > 0, "scattered zeros: silent bits");
  // all zero: nothing is ever written
  for (float& v : ppm) v = 0.0f;
  size_t s3 = 0, h3 = 0, w3 = 0;
  walk_distribution("all zero", ppm, &s3, &h3, &w3);
  CHECK(w3 == 0 && s3 == 256 * 8, "all zero");
  silent = s0 + s1 + s2 + s3;
  halves = h0 + h1 + h2 + h3;
  writes = w0 + w1 + w2 + w3;
  printf("ok: range walk, %zu predictions, %zu silent bits (denom == 0), %zu of p == 0.5\n", writes, silent, halves);
}

static void discretize_cases() {
  // both clamps and 0.5, and the ends of the float range Discretize may see
  const float eps = 0.0001f;
  CHECK(gmx_coder_discretize(eps) == (uint32_t)(1 + 65534 * eps), "Discretize(1e-4)");
  CHECK(gmx_coder_discretize(1.0f - eps) == (uint32_t)(1 + 65534 * (1.0f - eps)), "Discretize(1 - 1e-4)");
  CHECK(gmx_coder_discretize(0.5f) == 32768u, "Discretize(0.5)");
  CHECK(gmx_coder_discretize(eps) == 7u && gmx_coder_discretize(1.0f - eps) == 65528u, "the clamps' values");
  printf("ok: Discretize\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s <dir> <case>...\n", argv[0]);
    return 2;
  }
  for (int i = 2; i < argc; ++i) run_case(argv[1], argv[i]);
  walk_cases();
  discretize_cases();
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  return 0;
}
