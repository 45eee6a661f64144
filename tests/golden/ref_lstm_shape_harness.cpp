// ref_lstm_shape_harness.cpp -- TEST INFRASTRUCTURE, compiled by make_lstm_shape_golden.py where the reference's sources
// exist (-I<reference>/src, into a temporary directory).
//
// The REFERENCE's own Lstm(256, 256, cells, 1, horizon, learning_rate, gradient_clip, ltm) at a shape of the caller's,
// constructed after srand(seed) and driven the way LstmModel drives its lstm_ (models/lstm-model.cpp): per byte
// SetInput(ppm), Predict(last_byte), the range walk of the eight bits, Perceive(byte).
//
// usage: ref_lstm_shape_harness cells horizon learning_rate gradient_clip seed n_bytes in.bin out_prefix
//   in.bin: float ppm[n][256], then uint8 bytes[n]
//   out_prefix.probs: float [n][256], what Lstm::Predict returned for every byte
//   out_prefix.long:  lstm_output_layer, then the three NeuronLayerWeights, as LongTermMemory::WriteToDisk stores them
//   out_prefix.short: top_, mid_, bot_, probs_, then Lstm::WriteToDisk -- the stretch LstmModel::WriteToDisk writes
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <valarray>
#include <vector>

#include "models/lstm.h"

int main(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: %s cells horizon lr clip seed n_bytes in.bin out_prefix\n", argv[0]);
    return 2;
  }
  const unsigned cells = (unsigned)atoi(argv[1]);
  const int horizon = atoi(argv[2]);
  const float lr = strtof(argv[3], nullptr), clip = strtof(argv[4], nullptr);
  const unsigned seed = (unsigned)strtoul(argv[5], nullptr, 0);
  const size_t n = (size_t)strtoull(argv[6], nullptr, 0);
  const std::string prefix = argv[8];

  std::vector<float> ppm(n * 256);
  std::vector<uint8_t> bytes(n);
  {
    std::ifstream in(argv[7], std::ios::binary);
    in.read((char*)ppm.data(), (std::streamsize)(ppm.size() * 4));
    in.read((char*)bytes.data(), (std::streamsize)n);
    if (!in) {
      fprintf(stderr, "short input\n");
      return 2;
    }
  }

  srand(seed);
  LongTermMemory ltm;
  Lstm lstm(256, 256, cells, 1, horizon, lr, clip, ltm);

  int top = 255, mid = 127, bot = 0;
  std::valarray<float> probs(1.0 / 256, 256);
  unsigned last_byte = 0;
  std::ofstream po(prefix + ".probs", std::ios::binary);
  std::valarray<float> x(256);
  for (size_t i = 0; i < n; ++i) {
    for (int j = 0; j < 256; ++j) x[j] = ppm[i * 256 + j];
    lstm.SetInput(x);
    probs = lstm.Predict(last_byte, ltm);
    po.write((const char*)&probs[0], 256 * 4);
    top = 255;
    bot = 0;
    for (int k = 0; k < 8; ++k) {  // LstmModel::Predict's walk (lstm-model.cpp:34-41)
      if (k > 0) {
        if ((bytes[i] >> (8 - k)) & 1) bot = mid + 1;
        else top = mid;
      }
      mid = bot + ((top - bot) / 2);
    }
    lstm.Perceive(bytes[i], ltm);
    last_byte = bytes[i];
  }
  {
    std::ofstream lf(prefix + ".long", std::ios::binary);
    for (auto& e : ltm.lstm_output_layer)
      for (auto& y : e) lf.write((const char*)&y[0], (std::streamsize)(y.size() * 4));
    for (auto& g : ltm.neuron_layer_weights)
      for (auto& y : g.weights) lf.write((const char*)&y[0], (std::streamsize)(y.size() * 4));
  }
  {
    std::ofstream sf(prefix + ".short", std::ios::binary);
    sf.write((const char*)&top, 4);
    sf.write((const char*)&mid, 4);
    sf.write((const char*)&bot, 4);
    sf.write((const char*)&probs[0], 256 * 4);
    lstm.WriteToDisk(&sf);
  }
  return 0;
}
