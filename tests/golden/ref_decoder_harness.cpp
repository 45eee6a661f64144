// ref_decoder_harness.cpp -- the reference's own Decoder (coder/decoder.cpp, compiled where it lies) on top of a stub
// Predictor that returns recorded probabilities: records x1_, x2_, x_ and the bit after every Decode.  Built and run by
// tests/golden/make_decoder_golden.py (build container only); the fixture it writes holds inputs and recorded results.
//
//   ref_decoder_harness <payload.bin> <p.f32> <out.bin> <checkpoint scratch file>
//
// out.bin: n_bits x {x1, x2, x, bit} little-endian uint32, one row per value of p.f32.  The state is read through the
// Decoder's own WriteCheckpoint.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

// the Decoder needs three calls of its Predictor and nothing else of the model
#define PREDICTOR_H_
class Predictor {
 public:
  explicit Predictor(std::vector<float> p) : p_(std::move(p)) {}
  float Predict() { return p_[i_]; }
  void Perceive(int) {}
  void Learn() { ++i_; }

 private:
  std::vector<float> p_;
  size_t i_ = 0;
};

#include "coder/decoder.cpp"

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: %s payload.bin p.f32 out.bin scratch\n", argv[0]);
    return 2;
  }
  std::vector<float> p;
  {
    std::ifstream f(argv[2], std::ios::binary);
    float v;
    while (f.read(reinterpret_cast<char*>(&v), 4)) p.push_back(v);
  }
  const size_t n = p.size();
  Predictor pred(p);
  std::ifstream in(argv[1], std::ios::binary);
  if (!in.is_open()) return 3;
  Decoder dec(&in, &pred);
  std::ofstream out(argv[3], std::ios::binary);
  for (size_t t = 0; t < n; ++t) {
    const uint32_t bit = (uint32_t)dec.Decode();
    dec.WriteCheckpoint(argv[4]);
    uint32_t row[4] = {0, 0, 0, bit};
    std::ifstream ck(argv[4], std::ios::binary);
    if (!ck.read(reinterpret_cast<char*>(row), 12)) return 4;
    out.write(reinterpret_cast<const char*>(row), 16);
  }
  return out.good() ? 0 : 5;
}
