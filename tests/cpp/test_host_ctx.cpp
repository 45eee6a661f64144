// test_host_ctx.cpp -- gmx::CtxBank (gmix_amd/host/gmx_models.h), the C++ owner of a context bank: one stream through
// files (ReadFromDisk / WriteToDisk), the group checkpoint (ExportGroup / ImportGroup) and the boards (Boards /
// SetBoards) against the per-stream calls.  Needs an MI355X.  Built and run by tests/test_gpu_host_ctx_cpp.py, which
// passes a directory holding descs.bin (the gmx_ctx_desc records of the variables, which this program hands to the
// owner's Add... calls one by one) and sec<i>.bin / board<i>.bin of four streams -- written by the Python CtxGroup,
// since the owner has no run surface.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../gmix_amd/host/gmx_models.h"

static void Fail(const char* what, long t = -1) {
  fprintf(stderr, "Test failed: %s (stream %ld)\n", what, t);
  fflush(stderr);
  abort();  // the reference's convention (tester.cpp:318-321)
}
static std::vector<char> Slurp(const std::string& path) {
  std::ifstream s(path, std::ios::binary);
  if (!s) Fail(path.c_str());
  return std::vector<char>((std::istreambuf_iterator<char>(s)), std::istreambuf_iterator<char>());
}

static const int kS = 4;
static std::vector<gmx_ctx_desc> g_descs;

static void Build(gmx::CtxBank* b, int streams) {
  size_t hashes = 0;
  for (size_t i = 0; i < g_descs.size(); ++i) {
    const gmx_ctx_desc& d = g_descs[i];
    int at = -1;
    switch (d.kind) {
      case GMX_CTX_ZERO: at = b->AddZero(); break;
      case GMX_CTX_BIT_CONTEXT: at = b->AddBitContext(); break;
      case GMX_CTX_RECENT_BYTE: at = b->AddRecentByte(d.index); break;
      case GMX_CTX_BYTE_PLUS_RECENT: at = b->AddBytePlusRecent(d.index); break;
      case GMX_CTX_INTERVAL: at = b->AddIntervalContext(d.map, d.num_bits); break;
      case GMX_CTX_SKIP:
        at = b->AddSkipContext(std::vector<int>(d.bytes_to_use, d.bytes_to_use + d.n_bytes));
        break;
      case GMX_CTX_INDIRECT_HASH:
        at = b->AddIndirectHash(d.outer_order, d.table_size, d.inner_order);
        ++hashes;
        break;
      default: Fail("descs.bin: kind");
    }
    if (at != (int)i) Fail("Add");
  }
  if (b->Finalize(streams) != GMX_OK || !b->ready() || b->status() != GMX_OK) Fail("Finalize");
  if (b->size() != g_descs.size() || b->hashes() != hashes || b->streams() != streams || !b->handle())
    Fail("size / hashes / streams / handle");
}

static std::vector<char> PerStream(gmx::CtxBank* b, int s) {
  size_t n = 0;
  if (gmx_ctx_export(b->handle(), s, nullptr, &n, nullptr) != GMX_OK) Fail("gmx_ctx_export(size)", s);
  std::vector<char> p(n ? n : 1);
  if (gmx_ctx_export(b->handle(), s, p.data(), &n, nullptr) != GMX_OK) Fail("gmx_ctx_export", s);
  p.resize(n);
  return p;
}
static bool SameBoards(const std::vector<gmx_ctx_blackboard>& a, const std::vector<gmx_ctx_blackboard>& b) {
  return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(gmx_ctx_blackboard)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) Fail("usage: test_host_ctx <directory>");
  const std::string dir = argv[1];
  {
    std::vector<char> raw = Slurp(dir + "/descs.bin");
    if (raw.empty() || raw.size() % sizeof(gmx_ctx_desc)) Fail("descs.bin");
    g_descs.resize(raw.size() / sizeof(gmx_ctx_desc));
    memcpy(g_descs.data(), raw.data(), raw.size());
  }
  std::vector<std::vector<char>> secs;
  std::vector<gmx_ctx_blackboard> boards(kS);
  std::vector<char> all;
  std::vector<size_t> off(1, 0);
  for (int s = 0; s < kS; ++s) {
    secs.push_back(Slurp(dir + "/sec" + std::to_string(s) + ".bin"));
    std::vector<char> bb = Slurp(dir + "/board" + std::to_string(s) + ".bin");
    if (bb.size() != sizeof(gmx_ctx_blackboard)) Fail("board file", s);
    memcpy(&boards[s], bb.data(), bb.size());
    all.insert(all.end(), secs[s].begin(), secs[s].end());
    off.push_back(all.size());
  }
  std::vector<char> xb;
  std::vector<size_t> xo;
  std::vector<gmx_ctx_blackboard> got;
  if (gmx::CtxBank().ExportGroup(&xb, &xo) != GMX_ERR_STATE) Fail("ExportGroup before Finalize");
  // ---- ReadFromDisk per stream, then ExportGroup: the files' bytes
  gmx::CtxBank a;
  Build(&a, kS);
  for (int s = 0; s < kS; ++s) {
    std::ifstream f(dir + "/sec" + std::to_string(s) + ".bin", std::ios::binary);
    a.ReadFromDisk(&f, s);
    if (a.status() != GMX_OK) Fail("ReadFromDisk", s);
    if (PerStream(&a, s) != secs[s]) Fail("ReadFromDisk != gmx_ctx_export", s);
  }
  if (a.ExportGroup(&xb, &xo) != GMX_OK) Fail("ExportGroup");
  if (xo != off || xb != all) Fail("ExportGroup != the files");
  if (a.ExportGroup(&xb, &xo, 1, 2) != GMX_OK || xo.size() != 3 || xo[2] != off[3] - off[1] ||
      memcmp(xb.data(), all.data() + off[1], xo[2]) != 0)
    Fail("ExportGroup of a window");
  if (a.ExportGroup(&xb, &xo, 3, 2) != GMX_ERR_INVALID) Fail("a window beyond the bank");
  // ---- ImportGroup + SetBoards into a second bank, then WriteToDisk per stream
  gmx::CtxBank b;
  Build(&b, kS);
  if (b.ImportGroup(all, off) != GMX_OK) Fail("ImportGroup");
  if (b.SetBoards(boards) != GMX_OK) Fail("SetBoards");
  if (b.Boards(&got) != GMX_OK || !SameBoards(got, boards)) Fail("Boards != SetBoards");
  for (int s = 0; s < kS; ++s) {
    const std::string path = dir + "/out" + std::to_string(s) + ".bin";
    {
      std::ofstream f(path, std::ios::binary);
      b.WriteToDisk(&f, s);
    }
    if (b.status() != GMX_OK || Slurp(path) != secs[s]) Fail("WriteToDisk != the stream's file", s);
    gmx_ctx_blackboard one;
    if (gmx_ctx_blackboard_get(b.handle(), s, &one) != GMX_OK || memcmp(&one, &boards[s], sizeof one) != 0)
      Fail("board != gmx_ctx_blackboard_get", s);
  }
  // ---- damage: GMX_ERR_FORMAT, and the bank as it was
  {
    std::vector<char> bad = all;
    uint32_t count;
    memcpy(&count, bad.data() + off[3], 4);
    count += 1;  // the last stream's first table claims one entry more than its section holds
    memcpy(bad.data() + off[3], &count, 4);
    if (b.ImportGroup(bad, off) != GMX_ERR_FORMAT) Fail("damaged buffer accepted");
    std::vector<gmx_ctx_blackboard> badb = boards;
    badb[2].recent_bits = 0;
    if (b.SetBoards(badb) != GMX_ERR_INVALID) Fail("bad board accepted");
    if (b.ExportGroup(&xb, &xo) != GMX_OK || xo != off || xb != all) Fail("a refused import moved a bank");
    if (b.Boards(&got) != GMX_OK || !SameBoards(got, boards)) Fail("a refused set moved a board");
    // a damaged file through ReadFromDisk: status() turns GMX_ERR_FORMAT, the bank stays
    const std::string path = dir + "/bad.bin";
    {
      std::ofstream f(path, std::ios::binary);
      f.write(bad.data() + off[3], (std::streamsize)(off[4] - off[3]));
    }
    gmx::CtxBank c;
    Build(&c, 2);
    {
      std::ifstream f(dir + "/sec2.bin", std::ios::binary);
      c.ReadFromDisk(&f, 1);
    }
    if (c.status() != GMX_OK) Fail("ReadFromDisk into stream 1");
    {
      std::ifstream f(path, std::ios::binary);
      c.ReadFromDisk(&f, 1);
    }
    if (c.status() != GMX_ERR_FORMAT) Fail("a damaged file left status() alone");
    if (PerStream(&c, 1) != secs[2]) Fail("a damaged file moved the bank");
  }
  printf("Tests passed.\n");
  return 0;
}
