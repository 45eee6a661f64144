// test_host_match.cpp -- gmx::MatchBank (gmix_amd/host/gmx_models.h), the C++ owner of a Match bank: the group
// checkpoint (ExportAll / ImportAll) against the per-stream calls, and one stream through files.  Needs an MI355X.
// Built and run by tests/test_gpu_host_match_cpp.py, which passes a directory holding long<i>.bin / short<i>.bin of
// four streams -- written by the Python MatchGroup, since the owner has no Predict / Learn surface yet.
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

// the models of tests/test_gpu_host_match_cpp.py
static const unsigned kTables[] = {4096, 100, 40000};
static const int kLimit = 60, kK = 3, kS = 4;
static const uint64_t kHistory = 1024;

static void Build(gmx::MatchBank* b, int streams) {
  for (int i = 0; i < kK; ++i)
    if (b->Add(kTables[i], kLimit, 2 + 3 * i) != i) Fail("Add");
  if (b->Finalize(kHistory, streams) != GMX_OK || !b->ready() || b->status() != GMX_OK) Fail("Finalize");
  if (b->size() != (size_t)kK || b->streams() != streams || !b->handle()) Fail("size / streams / handle");
}

static void ExpectPerStream(gmx::MatchBank* b, int s, const std::vector<char>& l, const std::vector<char>& sh) {
  size_t nl = 0, ns = 0;
  if (gmx_match_export(b->handle(), s, nullptr, &nl, nullptr, &ns) != GMX_OK) Fail("gmx_match_export(size)", s);
  std::vector<char> pl(nl ? nl : 1), ps(ns ? ns : 1);
  if (gmx_match_export(b->handle(), s, pl.data(), &nl, ps.data(), &ns) != GMX_OK) Fail("gmx_match_export", s);
  if (nl != l.size() || memcmp(pl.data(), l.data(), nl) != 0) Fail("long section != gmx_match_export", s);
  if (ns != sh.size() || memcmp(ps.data(), sh.data(), ns) != 0) Fail("short section != gmx_match_export", s);
}

int main(int argc, char** argv) {
  if (argc < 2) Fail("usage: test_host_match <directory>");
  const std::string dir = argv[1];
  std::vector<char> lb, sb;
  std::vector<size_t> off(1, 0);
  std::vector<std::vector<char>> ls, ss;
  for (int s = 0; s < kS; ++s) {
    ls.push_back(Slurp(dir + "/long" + std::to_string(s) + ".bin"));
    ss.push_back(Slurp(dir + "/short" + std::to_string(s) + ".bin"));
    lb.insert(lb.end(), ls[s].begin(), ls[s].end());
    sb.insert(sb.end(), ss[s].begin(), ss[s].end());
    off.push_back(lb.size());
  }
  gmx::MatchBank a;
  Build(&a, kS);
  std::vector<char> xl, xs;
  std::vector<size_t> xo;
  if (gmx::MatchBank().ExportAll(&xl, &xo, &xs) != GMX_ERR_STATE) Fail("ExportAll before Finalize");
  if (a.ImportAll(lb, off, sb) != GMX_OK) Fail("ImportAll");
  // ExportAll against gmx_match_export per stream, and against what went in
  if (a.ExportAll(&xl, &xo, &xs) != GMX_OK) Fail("ExportAll");
  if (xo != off || xl != lb || xs != sb) Fail("ExportAll != the imported sections");
  for (int s = 0; s < kS; ++s)
    ExpectPerStream(&a, s, std::vector<char>(xl.begin() + xo[s], xl.begin() + xo[s + 1]),
                    std::vector<char>(xs.begin() + 11 * kK * s, xs.begin() + 11 * kK * (s + 1)));
  // the round trip into a second bank
  gmx::MatchBank b;
  Build(&b, kS);
  if (b.ImportAll(xl, xo, xs) != GMX_OK) Fail("ImportAll into a second bank");
  std::vector<char> yl, ys;
  std::vector<size_t> yo;
  if (b.ExportAll(&yl, &yo, &ys) != GMX_OK || yo != xo || yl != xl || ys != xs) Fail("round trip");
  // a damaged buffer: GMX_ERR_FORMAT, and the bank as it was
  {
    std::vector<char> bad = xl;
    uint64_t hs;
    memcpy(&hs, bad.data() + xo[2], 8);
    hs = kHistory + 1;  // a history above the capacity, in the third stream
    memcpy(bad.data() + xo[2], &hs, 8);
    if (b.ImportAll(bad, xo, xs) != GMX_ERR_FORMAT) Fail("damaged long buffer accepted");
    std::vector<char> bads = xs;
    bads[11 * kK * 3 + 9] = 3;  // bit_pos_ neither 0 nor a power of two, in the last stream
    if (b.ImportAll(xl, xo, bads) != GMX_ERR_FORMAT) Fail("damaged short buffer accepted");
    std::vector<size_t> short_off(xo.begin(), xo.end() - 1);
    if (b.ImportAll(xl, short_off, xs) != GMX_ERR_INVALID) Fail("offsets of another stream count accepted");
    if (b.ExportAll(&yl, &yo, &ys) != GMX_OK || yo != xo || yl != xl || ys != xs) Fail("a refused import moved a bank");
  }
  // one stream through files: stream 1 of `a` -> stream 0 of a one-stream bank
  {
    const std::string fl = dir + "/one.long", fs = dir + "/one.short";
    {
      std::ofstream l(fl, std::ios::binary), s(fs, std::ios::binary);
      a.WriteToDisk(&l, 1);
      a.WriteShortToDisk(&s, 1);
    }
    if (Slurp(fl) != ls[1] || Slurp(fs) != ss[1]) Fail("WriteToDisk != the stream's sections");
    gmx::MatchBank c;
    Build(&c, 1);
    {
      std::ifstream s(fs, std::ios::binary), l(fl, std::ios::binary);
      c.ReadShortFromDisk(&s);
      c.ReadFromDisk(&l);
    }
    if (c.status() != GMX_OK) Fail("ReadFromDisk");
    ExpectPerStream(&c, 0, ls[1], ss[1]);
    gmx::MatchBank e;
    Build(&e, 2);
    e.Copy(&a, 1, 3);  // Match::Copy: stream 3 of `a` -> stream 1 of `e`
    if (e.status() != GMX_OK) Fail("Copy");
    ExpectPerStream(&e, 1, ls[3], ss[3]);
  }
  printf("Tests passed.\n");
  return 0;
}
