// ref_encoder_harness.cpp -- the reference's own Encoder (coder/encoder.cpp, compiled where it lies): records x1_, x2_
// and the byte count after every Encode, and the whole output after Flush.  Built and run by
// tests/golden/make_encoder_golden.py (build container only); the fixture it writes holds inputs and recorded results.
//
//   ref_encoder_harness <bits.u8> <p.f32> <rows.bin> <payload.bin> <checkpoint scratch file> [x1 x2]
//
// rows.bin: n_bits x {x1, x2, bytes so far} little-endian uint32.  The state is read through the Encoder's own
// WriteCheckpoint; with x1 x2 the run resumes from a checkpoint file the harness writes itself, through ReadCheckpoint.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

// the Encoder needs nothing of the model
#define PREDICTOR_H_

#include "coder/encoder.cpp"

int main(int argc, char** argv) {
  if (argc != 6 && argc != 8) {
    fprintf(stderr, "usage: %s bits.u8 p.f32 rows.bin payload.bin scratch [x1 x2]\n", argv[0]);
    return 2;
  }
  std::vector<uint8_t> bits;
  std::vector<float> p;
  {
    std::ifstream f(argv[1], std::ios::binary);
    char c;
    while (f.get(c)) bits.push_back((uint8_t)c);
    std::ifstream g(argv[2], std::ios::binary);
    float v;
    while (g.read(reinterpret_cast<char*>(&v), 4)) p.push_back(v);
  }
  if (bits.size() != p.size()) return 3;
  std::ofstream payload(argv[4], std::ios::binary);
  Encoder enc(&payload);
  if (argc == 8) {
    const uint32_t w[2] = {(uint32_t)strtoul(argv[6], nullptr, 0), (uint32_t)strtoul(argv[7], nullptr, 0)};
    std::ofstream ck(argv[5], std::ios::binary);
    ck.write(reinterpret_cast<const char*>(w), 8);
    ck.close();
    enc.ReadCheckpoint(argv[5]);
  }
  std::ofstream rows(argv[3], std::ios::binary);
  for (size_t t = 0; t < p.size(); ++t) {
    enc.Encode(bits[t], p[t]);
    enc.WriteCheckpoint(argv[5]);
    uint32_t row[3] = {0, 0, (uint32_t)payload.tellp()};
    std::ifstream ck(argv[5], std::ios::binary);
    if (!ck.read(reinterpret_cast<char*>(row), 8)) return 4;
    rows.write(reinterpret_cast<const char*>(row), 12);
  }
  enc.Flush();
  payload.close();
  return rows.good() ? 0 : 5;
}
