// fold_items_selftest.cpp -- CPU check, under ASan/UBSan, of what hpf_fold_in_items decides on the host
// (tests/test_fold_items_plan.py builds and runs it; nothing links it).
// 1. hpf_plan::fold_items_plan over K = 1..HPF_MAX_COLUMNS with and without bias:
//      R * 64 >= ld, an instance of fold_in_long_kernel for (R, WAVES)
//      the workgroup's LDS (WAVES partial rows of R * 64 doubles + the shared stop word) within what a launch may ask for
//      hpf_plan::fold_part: the parts of the WAVES waves cover [0, len) exactly once, in order, in whole 64-blocks, for a
//        seeded list of lengths with 0, 1 and WAVES * 64 +- 1 among them
//      grid_long(n_long) >= 1 for n_long >= 1, never more workgroups than long rows or than FOLD_LONG_BLOCKS_MAX
//    stdout: for a fixed list of cases a line
//      fip K bias ld R waves lds_long_bytes long_min grid_long(1) grid_long(5000) | the parts of a row of waves * 64 + 1
//    which the test compares with tests/data/fold_items_plan_table.txt.
// 2. Ratings::read_fold_in_items on the cases of host_selftest.cpp's fold-in block, transposed.
// Then `fold_items_selftest ok: <points> points`.
#include "../hpf_plan.hpp"
#include "hgaprec_host.hpp"

#include <unistd.h>

#include <string>

using namespace hpf_plan;
using hgaprec::Ratings;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                     \
  do { if (!(cond)) { if (++g_fail <= 20) { fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } } while (0)

static void check_parts(uint32_t len, uint32_t waves)
{
  uint32_t at = 0;
  for (uint32_t w = 0; w < waves; ++w) {
    const FoldPart p = fold_part(len, waves, w);
    CHECK(p.begin == at && p.end >= p.begin && p.end <= len, "len=%u waves=%u w=%u [%u, %u) after %u", len, waves, w, p.begin, p.end, at);
    CHECK(p.begin % 64 == 0 || p.begin == len, "len=%u w=%u: begin %u inside a block", len, w, p.begin);
    CHECK(p.end % 64 == 0 || p.end == len, "len=%u w=%u: end %u inside a block", len, w, p.end);
    at = p.end;
  }
  CHECK(at == len, "len=%u waves=%u: covered up to %u", len, waves, at);
}

static void check_plan(uint32_t K, bool bias, uint64_t &rng)
{
  const uint32_t C = K + (bias ? 2u : 0u);
  const FoldItemsPlan p = fold_items_plan(K, bias);
  if (C > HPF_MAX_COLUMNS) { CHECK(!p.ok, "K=%u bias=%d: a plan beyond HPF_MAX_COLUMNS", K, (int)bias); return; }
  CHECK(p.ok && p.wave.ok, "K=%u bias=%d: no plan", K, (int)bias);
  CHECK(p.wave.R * 64 >= p.wave.ld && p.wave.ld >= C, "K=%u bias=%d ld=%u R=%u", K, (int)bias, p.wave.ld, p.wave.R);
  CHECK((p.waves == 8 || p.waves == 4) && has_fold_long((int)p.wave.R, (int)p.waves), "K=%u R=%u waves=%u: no instance", K, p.wave.R, p.waves);
  CHECK(p.lds_long_bytes() >= (uint64_t)p.waves * p.wave.R * 64 * 8 + 4 && p.lds_long_bytes() <= FOLD_LDS_LIMIT, "K=%u lds=%u", K, p.lds_long_bytes());
  CHECK(p.long_min == FOLD_LONG_MIN && p.long_min >= 1, "K=%u long_min=%u", K, p.long_min);
  const uint32_t W = p.waves;
  const uint32_t fixed[] = {0, 1, 63, 64, 65, W * 64 - 1, W * 64, W * 64 + 1, 2 * W * 64 + 1, FOLD_LONG_MIN, 0xffffffffu, 0xffffffc0u};
  for (uint32_t len : fixed) check_parts(len, W);
  for (int i = 0; i < 8; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    check_parts((uint32_t)(rng >> 32) >> ((rng >> 8) % 31), W);
    const uint32_t nl = i == 0 ? 1u : i == 1 ? 0xffffffffu : (uint32_t)(rng >> 32) >> ((rng >> 16) % 31);
    const uint32_t g = p.grid_long(nl);
    CHECK((nl == 0) == (g == 0) && g <= nl && g <= FOLD_LONG_BLOCKS_MAX, "K=%u n_long=%u grid=%u", K, nl, g);
    CHECK(g == nl || g == FOLD_LONG_BLOCKS_MAX, "K=%u n_long=%u grid=%u: a long row without a workgroup while the grid has room", K, nl, g);
  }
}

// ---- -fold-in-items FILE: new items against the users of a data set that has been read ----
static std::string g_dir;
static std::string path(const char *name) { return g_dir + "/" + name; }
static void write_text(const std::string &p, const std::string &s)
{
  FILE *f = fopen(p.c_str(), "w");
  if (!f) { perror(p.c_str()); exit(2); }
  fwrite(s.data(), 1, s.size(), f);
  fclose(f);
}

static void check_reader()
{
  write_text(path("fi_train.tsv"), "70\t1\t5\n30\t1\t4\n90\t2\t3\n");
  Ratings r; r.cap_n = 10; r.cap_m = 10;
  CHECK(r.read_train(path("fi_train.tsv")) == 0 && r.n == 3 && r.m == 2, "train: n=%u m=%u", r.n, r.m);
  // first appearance, a duplicated pair (last wins, both copies stay), rating 0, an unknown user, an item with nothing
  // but unknown users, 300 wraps to 44, no trailing newline; item 1 is known to train.tsv and still a new item here
  write_text(path("fi.tsv"), "30\t50\t2\n70\t40\t1\n555\t50\t5\n30\t50\t4\n556\t60\t1\n90\t40\t0\n90\t50\t300\n70\t1\t3");
  Ratings f; uint64_t skipped = 99;
  CHECK(r.read_fold_in_items(path("fi.tsv"), &f, &skipped) == 0, "fi.tsv");
  CHECK(skipped == 2 && f.m == 3 && f.n == 3 && f.seq2user == r.seq2user, "skipped=%llu m=%u n=%u", (unsigned long long)skipped, f.m, f.n);
  CHECK(f.seq2item.size() == 3 && f.seq2item[0] == 50 && f.seq2item[1] == 40 && f.seq2item[2] == 1, "seq2item");
  // users 70, 30, 90 are rows 0, 1, 2: 70 rated 40 and 1; 30 rated 50 twice; 90 rated 50
  CHECK(f.rowptr.size() == 4 && f.rowptr[1] == 2 && f.rowptr[2] == 4 && f.rowptr[3] == 5 && f.col.size() == 5 && f.val.size() == 5, "rowptr");
  if (f.col.size() == 5) {
    CHECK(f.col[0] == 1 && f.col[1] == 2 && f.col[2] == 0 && f.col[3] == 0 && f.col[4] == 0, "col");
    CHECK(f.val[0] == 1 && f.val[1] == 3 && f.val[2] == 4 && f.val[3] == 4 && f.val[4] == 44, "val");
  }
  write_text(path("fi_empty.tsv"), "");
  Ratings e; skipped = 99;
  CHECK(r.read_fold_in_items(path("fi_empty.tsv"), &e, &skipped) == 0 && e.m == 0 && e.n == 3 && skipped == 0 && e.rowptr.size() == 4 && e.col.empty(), "empty file");
  write_text(path("fi_junk.tsv"), "30\t1\t3\nabc\t2\n");
  Ratings j;
  CHECK(r.read_fold_in_items(path("fi_junk.tsv"), &j, &skipped) == -2, "junk token");
  write_text(path("fi_short.tsv"), "30\t1\t3\n70\t2");
  CHECK(r.read_fold_in_items(path("fi_short.tsv"), &j, &skipped) != -1, "a last record cut short is read by the train reader's rules");
  CHECK(r.read_fold_in_items(path("fi-does-not-exist.tsv"), &j, &skipped) == -1, "missing file");
  std::string big = "30\t4294967295\t4294967295\n70\t99999999999999999999\t1\n90\t" + std::string(100000, '7') + "\t1\n";
  write_text(path("fi_big.tsv"), big);
  Ratings b;
  CHECK(r.read_fold_in_items(path("fi_big.tsv"), &b, &skipped) == 0 && b.m >= 1 && b.n == 3 && (uint64_t)b.rowptr[b.n] == b.col.size(), "overlong tokens");
  for (uint32_t c : b.col) CHECK(c < b.m, "column %u of %u items", c, b.m);
}

int main()
{
  uint64_t rng = 20261020u;
  unsigned points = 0;
  for (uint32_t K = 1; K <= HPF_MAX_COLUMNS; ++K)
    for (int bias = 0; bias < 2; ++bias) { check_plan(K, bias != 0, rng); ++points; }
  CHECK(!fold_items_plan(0, false).ok, "K=0 has a plan");
  const uint32_t cases[] = {1, 3, 7, 14, 16, 17, 20, 50, 62, 64, 65, 100, 126, 128, 129, 190, 192, 256, 300, 510, 512, 513, 576, 760, 768, 1000, 1022, 1024};
  for (uint32_t K : cases)
    for (int bias = 0; bias < 2; ++bias) {
      const FoldItemsPlan p = fold_items_plan(K, bias != 0);
      if (!p.ok) { printf("fip %u %d none\n", K, bias); continue; }
      printf("fip %u %d %u %u %u %u %u %u %u |", K, bias, p.wave.ld, p.wave.R, p.waves, p.lds_long_bytes(), p.long_min, p.grid_long(1), p.grid_long(5000));
      for (uint32_t w = 0; w < p.waves; ++w) { const FoldPart q = fold_part(p.waves * 64 + 1, p.waves, w); printf(" %u-%u", q.begin, q.end); }
      printf("\n");
    }

  char tmpl[] = "/tmp/fold_items_selftest.XXXXXX";
  if (!mkdtemp(tmpl)) { perror("mkdtemp"); return 2; }
  g_dir = tmpl;
  check_reader();
  const char *files[] = {"fi_train.tsv", "fi.tsv", "fi_empty.tsv", "fi_junk.tsv", "fi_short.tsv", "fi_big.tsv"};
  for (const char *f : files) unlink(path(f).c_str());
  rmdir(tmpl);

  if (g_fail) { fprintf(stderr, "fold_items_selftest: %d checks failed\n", g_fail); return 1; }
  printf("fold_items_selftest ok: %u points\n", points);
  return 0;
}
