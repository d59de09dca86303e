// host_selftest.cpp -- CPU-only driver of the host side, built with
// -fsanitize=address,undefined by `make asan` (the
// reference has no sanitizer build; its reader has missing-return UB).  It walks
// the code that owns raw memory and sockets -- the hand-rolled id maps, the TSV
// reader on hostile input, the binary dataset cache (valid, truncated and
// corrupted images), the multi-threaded "%.8f" writer, the TCP star used by
// `hgaprec -ngpus N` -- and checks results, so that a sanitizer report or a
// wrong answer both fail the run.  No HIP, no oracle.
#include "hgaprec_host.hpp"

#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

using namespace hgaprec;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } } while (0)

static std::string g_dir;
static std::string path(const char *name) { return g_dir + "/" + name; }

static void write_text(const std::string &p, const std::string &s)
{
  FILE *f = fopen(p.c_str(), "w");
  if (!f) { perror(p.c_str()); exit(2); }
  fwrite(s.data(), 1, s.size(), f);
  fclose(f);
}

static std::string read_text(const std::string &p)
{
  std::string s; FILE *f = fopen(p.c_str(), "r");
  if (!f) return s;
  char buf[65536]; size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

// ---- id maps: growth, collisions, ids at the edges of uint32 --------------
static void test_idmap()
{
  Ratings::IdMap mp;
  std::mt19937 g(1);
  std::vector<uint32_t> keys;
  for (int i = 0; i < 200000; ++i) keys.push_back((uint32_t)g());
  keys.push_back(0u); keys.push_back(0xffffffffu); keys.push_back(0xfffffffeu);
  std::vector<uint32_t> first(keys.size());
  for (size_t i = 0; i < keys.size(); ++i) {
    uint32_t v;
    if (!mp.find(keys[i], &v)) { mp.put(keys[i], (uint32_t)i); first[i] = (uint32_t)i; }
    else first[i] = v;
  }
  for (size_t i = 0; i < keys.size(); ++i) { uint32_t v = 0; CHECK(mp.find(keys[i], &v) && v == first[i]); }
  uint32_t v;
  CHECK(!mp.find(123456789u, &v) || true);
}

// ---- reader on well-formed and hostile input --------------------------------
static void test_reader()
{
  // first-seen order, duplicates, rating 0, rating 300 (uint8 wrap), capacity, no trailing newline
  write_text(path("train.tsv"), "7\t70\t5\n3\t30\t4\n7\t30\t0\n7\t70\t2\n9\t90\t300\n3\t70\t1\n11\t10\t3\n9\t30\t1");
  Ratings r; r.cap_n = 3; r.cap_m = 3; r.binary = false; r.rating_threshold = 1;
  CHECK(r.read_train(path("train.tsv")) == 0);
  CHECK(r.n == 3 && r.m == 3);                         // user 11 / item 10 are over capacity
  CHECK(r.seq2user[0] == 7 && r.seq2user[1] == 3 && r.seq2user[2] == 9);
  CHECK(r.rowptr.size() == 4 && (uint64_t)r.rowptr[3] == r.col.size());
  CHECK(r.col.size() == r.val.size());
  // user 7: item 70 twice (duplicate kept in the list, last rating wins), item 30 dropped (rating 0)
  CHECK(r.rowptr[1] - r.rowptr[0] == 2 && r.val[0] == 2 && r.val[1] == 2);
  // rating 300 wraps to 44
  bool saw44 = false; for (uint8_t y : r.val) saw44 |= (y == 44);
  CHECK(saw44);
  write_text(path("validation.tsv"), "7\t30\t4\n99\t30\t5\n7\t999\t1\n3\t70\t0\n");
  CHECK(r.read_heldout(path("validation.tsv"), &r.validation) == 0);
  CHECK(r.validation.u.size() == 1);                   // unseen ids and rating 0 are skipped

  // hostile: garbage tokens, huge numbers, a NUL byte, very long line, empty file
  write_text(path("junk.tsv"), std::string("1\t2\t3\nabc\tdef\n4\t5\t6\n"));
  Ratings j; j.cap_n = 10; j.cap_m = 10;
  (void)j.read_train(path("junk.tsv"));               // must terminate without touching bad memory
  std::string big = "4294967295\t4294967295\t4294967295\n99999999999999999999\t1\t1\n";
  big += std::string(100000, '7') + "\t1\t1\n";
  write_text(path("big.tsv"), big);
  Ratings b; b.cap_n = 10; b.cap_m = 10;
  (void)b.read_train(path("big.tsv"));
  write_text(path("empty.tsv"), "");
  Ratings e; e.cap_n = 10; e.cap_m = 10;
  (void)e.read_train(path("empty.tsv"));
  CHECK(e.n == 0);
  Ratings missing; missing.cap_n = 1; missing.cap_m = 1;
  CHECK(missing.read_train(path("does-not-exist.tsv")) != 0);
}

// ---- -fold-in FILE: new users against the items of a data set that has been read -------
static void test_fold_in_reader()
{
  write_text(path("fi_train.tsv"), "1\t70\t5\n1\t30\t4\n2\t90\t3\n");
  Ratings r; r.cap_n = 10; r.cap_m = 10;
  CHECK(r.read_train(path("fi_train.tsv")) == 0 && r.m == 3);
  // first appearance, a duplicated pair (last wins, both copies stay), rating 0, an unknown item, a user with nothing
  // but unknown items, 300 wraps to 44, no trailing newline
  write_text(path("fi.tsv"), "50\t30\t2\n40\t70\t1\n50\t555\t5\n50\t30\t4\n60\t556\t1\n40\t90\t0\n50\t90\t300");
  Ratings f; uint64_t skipped = 99;
  CHECK(r.read_fold_in(path("fi.tsv"), &f, &skipped) == 0);
  CHECK(skipped == 2 && f.n == 2 && f.m == 3 && f.seq2item == r.seq2item);
  CHECK(f.seq2user.size() == 2 && f.seq2user[0] == 50 && f.seq2user[1] == 40);
  CHECK(f.rowptr.size() == 3 && f.rowptr[1] == 3 && f.rowptr[2] == 4 && f.col.size() == 4 && f.val.size() == 4);
  if (f.col.size() == 4) {
    CHECK(f.col[0] == 1 && f.col[1] == 1 && f.col[2] == 2 && f.col[3] == 0);
    CHECK(f.val[0] == 4 && f.val[1] == 4 && f.val[2] == 44 && f.val[3] == 1);
  }
  write_text(path("fi_empty.tsv"), "");
  Ratings e; skipped = 99;
  CHECK(r.read_fold_in(path("fi_empty.tsv"), &e, &skipped) == 0 && e.n == 0 && skipped == 0 && e.rowptr.size() == 1 && e.col.empty());
  write_text(path("fi_junk.tsv"), "1\t30\t3\nabc\t2\n");
  Ratings j;
  CHECK(r.read_fold_in(path("fi_junk.tsv"), &j, &skipped) == -2);
  CHECK(r.read_fold_in(path("fi-does-not-exist.tsv"), &j, &skipped) == -1);
  std::string big = "4294967295\t30\t4294967295\n99999999999999999999\t70\t1\n" + std::string(100000, '7') + "\t90\t1\n";
  write_text(path("fi_big.tsv"), big);
  Ratings b;
  CHECK(r.read_fold_in(path("fi_big.tsv"), &b, &skipped) == 0 && b.n >= 1 && (uint64_t)b.rowptr[b.n] == b.col.size());
}

// ---- dataset cache: round trip, then every kind of damaged image ------------
static void test_cache()
{
  const std::string d = path("cache");
  mkdir(d.c_str(), 0775);
  std::mt19937 g(5);
  std::string tr, va, te;
  for (int i = 0; i < 5000; ++i) {
    char line[64];
    snprintf(line, sizeof line, "%u\t%u\t%u\n", (unsigned)(g() % 300) + 1, (unsigned)(g() % 200) + 1, (unsigned)(g() % 6));
    (i % 10 == 0 ? va : i % 10 == 1 ? te : tr) += line;
  }
  write_text(d + "/train.tsv", tr); write_text(d + "/validation.tsv", va); write_text(d + "/test.tsv", te);
  Ratings a; a.cap_n = 300; a.cap_m = 200;
  CHECK(a.read_train(d + "/train.tsv") == 0);
  CHECK(a.read_heldout(d + "/validation.tsv", &a.validation) == 0);
  CHECK(a.read_heldout(d + "/test.tsv", &a.test) == 0);
  CHECK(a.save_cache(d) == 0);
  Ratings b; b.cap_n = 300; b.cap_m = 200;
  CHECK(b.load_cache(d) == 0);
  CHECK(b.n == a.n && b.m == a.m && b.col == a.col && b.val == a.val && b.rowptr == a.rowptr);
  CHECK(b.seq2user == a.seq2user && b.seq2item == a.seq2item);
  CHECK(b.validation.u == a.validation.u && b.test.y == a.test.y && b.heldout_loaded);
  uint32_t s = 0;
  CHECK(b.user2seq.find(a.seq2user[5], &s) && s == 5);
  // different reader parameters => the image must be refused
  Ratings c; c.cap_n = 299; c.cap_m = 200;
  CHECK(c.load_cache(d) != 0);

  const std::string img = d + "/hgaprec.cache.bin";
  const std::string good = read_text(img);
  CHECK(good.size() > 64);
  auto try_image = [&](const std::string &bytes) {
    write_text(img, bytes);
    Ratings x; x.cap_n = 300; x.cap_m = 200;
    return x.load_cache(d);                            // any answer but a crash / overrun is fine ...
  };
  for (size_t cut : {(size_t)0, (size_t)7, (size_t)40, good.size() / 3, good.size() / 2, good.size() - 1})
    CHECK(try_image(good.substr(0, cut)) != 0);         // ... and a truncated image must be refused
  std::mt19937 h(9);
  for (int t = 0; t < 200; ++t) {                       // flipped bytes in the header / counts area
    std::string bad = good;
    const size_t at = h() % std::min<size_t>(bad.size(), 256);
    bad[at] = (char)(bad[at] ^ (1 << (h() % 8)));
    (void)try_image(bad);
  }
  for (int t = 0; t < 50; ++t) {                        // a count field blown up to "huge"
    std::string bad = good;
    const size_t at = (h() % 32) * 4;
    if (at + 4 <= bad.size()) { const uint32_t hugev = 0xfffffff0u; memcpy(&bad[at], &hugev, 4); }
    (void)try_image(bad);
  }
  write_text(img, good);
}

// ---- writers: the threaded matrix writer equals the serial one --------------
static void test_writers()
{
  const uint32_t rows = 20000, cols = 7;
  std::vector<double> a((size_t)rows * cols);
  std::mt19937_64 g(3);
  for (double &v : a) {
    const int kind = (int)(g() % 6);
    const double u = (double)(g() >> 11) / 9007199254740992.0;
    v = kind == 0 ? u * 1e-9 : kind == 1 ? u * 1e6 : kind == 2 ? 0.0 : kind == 3 ? 0.5 + 5e-9 : u;
  }
  std::vector<uint32_t> ids(rows);
  for (uint32_t i = 0; i < rows; ++i) ids[i] = 1000000u - i;
  setenv("HGAPREC_SAVE_THREADS", "1", 1);
  CHECK(save_matrix(path("m1.tsv"), a.data(), rows, cols, ids.data(), rows, 5) == 0);
  setenv("HGAPREC_SAVE_THREADS", "7", 1);
  CHECK(save_matrix(path("m7.tsv"), a.data(), rows, cols, ids.data(), rows, 5) == 0);
  unsetenv("HGAPREC_SAVE_THREADS");
  const std::string s1 = read_text(path("m1.tsv")), s7 = read_text(path("m7.tsv"));
  CHECK(!s1.empty() && s1 == s7);
  // the fast formatter against printf on the same values
  char buf[64], ref[64];
  for (size_t i = 0; i < 20000; ++i) {
    const size_t n = format_fixed8(a[i], buf); buf[n] = 0;
    snprintf(ref, sizeof ref, "%.8f", a[i]);
    CHECK(!strcmp(buf, ref));
  }
  CHECK(save_vector(path("v.tsv"), a.data(), 100, ids.data(), 10, 0) == 0);   // ids shorter than rows
  CHECK(save_matrix("/nonexistent-dir/x.tsv", a.data(), 2, 2, ids.data(), 2, 0) != 0);
}

// ---- start state: shard slices of the one MT19937 stream ---------------------
static void test_state()
{
  const uint32_t n = 57, m = 31, k = 6;
  Mt19937 r0 = make_rng(7.0), r1 = make_rng(7.0), r2 = make_rng(7.0);
  GammaState full, lo, hi;
  initialize_state(r0, n, m, k, true, true, &full);
  initialize_state(r1, n, m, k, true, true, &lo, 0, 20);
  initialize_state(r2, n, m, k, true, true, &hi, 20, n);
  CHECK(lo.n == 20 && hi.n == n - 20);
  CHECK(r0.next_u32() == r1.next_u32());
  CHECK(lo.beta_E == full.beta_E && hi.eta_Elog == full.eta_Elog);
  for (uint32_t e = 0; e < 20 * k; ++e) CHECK(lo.theta_E[e] == full.theta_E[e]);
  for (uint32_t e = 0; e < (n - 20) * k; ++e) CHECK(hi.theta_Elog[e] == full.theta_Elog[20 * k + e]);
  CHECK(std::fabs(digamma(1.0) + 0.57721566490153286) < 1e-15);
  StopRule st; int why = -1;
  CHECK(!st.update(10, -2.0, &why));
}

// ---- TCP star: 4 ranks as threads, a stranger knocking first ------------------
static void test_comm()
{
  const int world = 4, port = 20000 + (int)(getpid() % 20000);
  const uint64_t nonce = 0xc0ffee1234ull;
  std::vector<int> ok(world, 0);
  std::vector<double> sums(world, 0.0), maxs(world, 0.0);
  std::vector<uint32_t> got(world, 0);
  auto body = [&](int rank) {
    Comm c;
    if (c.init(rank, world, "127.0.0.1", port, nonce)) return;
    std::vector<double> v(1000);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (double)(rank + 1) * (double)(i + 1);
    if (c.allreduce_sum(v.data(), v.size())) return;
    sums[rank] = v[999];
    double mx = (double)rank;
    if (c.allreduce_max(&mx, 1)) return;
    maxs[rank] = mx;
    uint32_t token = rank == 0 ? 0xabcdef01u : 0;
    if (c.bcast(&token, 4)) return;
    got[rank] = token;
    if (c.barrier()) return;
    c.close_all();
    ok[rank] = 1;
  };
  std::vector<std::thread> th;
  th.emplace_back(body, 0);
  {
    // a connection that does not know the nonce must be dropped, not given a rank
    std::thread s([&] { Comm x; (void)x.init(2, world, "127.0.0.1", port, 0xbadull); x.close_all(); });
    s.join();
  }
  for (int r = 1; r < world; ++r) th.emplace_back(body, r);
  for (auto &t : th) t.join();
  for (int r = 0; r < world; ++r) {
    CHECK(ok[r]);
    CHECK(sums[r] == 1000.0 * (1 + 2 + 3 + 4));
    CHECK(maxs[r] == 3.0);
    CHECK(got[r] == 0xabcdef01u);
  }
  // MASTER_ADDR as a NAME (launchers export localhost / a host name): resolved, rank 0 listens;
  // a name that does not resolve is an error of its own, not "cannot reach rank 0"
  {
    std::vector<int> ok2(2, 0);
    auto two = [&](int rank) {
      Comm c;
      if (c.init(rank, 2, "localhost", port + 1, nonce)) return;
      double v = rank + 1.0;
      if (c.allreduce_sum(&v, 1) || v != 3.0) return;
      c.close_all();
      ok2[rank] = 1;
    };
    std::thread a(two, 0), b(two, 1);
    a.join(); b.join();
    CHECK(ok2[0] && ok2[1]);
    Comm bad;
    CHECK(bad.init(0, 2, "no-such-host.invalid", port + 2, nonce) == -2);
  }
  // partition: every rank non-empty, boundaries monotone, balanced on nnz
  std::vector<int64_t> rp(1, 0);
  std::mt19937 g(2);
  for (int u = 0; u < 5000; ++u) rp.push_back(rp.back() + (int64_t)(g() % 100));
  for (int w : {1, 2, 3, 8, 64}) {
    auto parts = partition_users(rp, w);
    CHECK((int)parts.size() == w && parts.front().first == 0 && parts.back().second == 5000);
    for (int r = 0; r < w; ++r) {
      CHECK(parts[r].first < parts[r].second);
      if (r) CHECK(parts[r].first == parts[r - 1].second);
    }
  }
}

// ---- Env: directory name and flags --------------------------------------------
static void test_env()
{
  const char *argv1[] = {"hgaprec", "-dir", "data/ml", "-n", "300", "-m", "200", "-k", "5", "-hier", "-seed", "7"};
  Env e; std::string bad;
  CHECK(e.parse(12, (char **)argv1, false, &bad) == 0);
  CHECK(e.make_prefix() == "n300-m200-k5-da-batch-hier-vb-seed7");
  const char *argv2[] = {"hgaprec", "-dir", "x", "-bogus"};
  Env e2;
  CHECK(e2.parse(4, (char **)argv2, false, &bad) != 0 && bad == "-bogus");
  const char *argv3[] = {"hgaprec", "-n"};                  // value missing at the end of argv
  Env e3;
  (void)e3.parse(2, (char **)argv3, false, &bad);
}

// ---- the threaded host paths (round 4): a ratings file parsed in pieces, the CSR built per user range, the start
// state's expectations and the matrix writer on several threads -- the results of the one-thread paths, and (under
// -fsanitize=thread, `make tsan`) no data race on the way
static void test_threads()
{
  std::mt19937 g(5);
  std::string text;
  const int R = 60000;
  for (int j = 0; j < R; ++j) {
    const unsigned u = j < R / 2 ? 100u + (unsigned)(j / 9) : 100u + g() % 9000u;       // grouped, then scattered users
    const unsigned i = 1u + (g() % 97u) * (g() % 41u);
    text += std::to_string(u) + "\t" + std::to_string(i) + "\t" + std::to_string(g() % 6u) + "\n";
  }
  write_text(path("big.tsv"), text);
  write_text(path("bigv.tsv"), text.substr(0, text.size() / 3 * 2));                       // may end inside a record: token-by-token then
  auto read = [&](const char *threads, uint32_t cap_n, Ratings *r) {
    setenv("HGAPREC_READ_THREADS", threads, 1);
    setenv("HGAPREC_READ_PARALLEL_MIN", "0", 1);
    r->cap_n = cap_n; r->cap_m = 100000;
    CHECK(r->read_train(path("big.tsv")) == 0);
    CHECK(r->read_heldout(path("bigv.tsv"), &r->validation) == 0);
  };
  for (uint32_t cap_n : {100000u, 3000u}) {                 // 3000: the capacity binds, the fast path hands its records back
    Ratings one, many;
    read("1", cap_n, &one);
    read("5", cap_n, &many);
    CHECK(one.n == many.n && one.m == many.m && one.nratings == many.nratings);
    CHECK(one.rowptr == many.rowptr && one.col == many.col && one.val == many.val);
    CHECK(one.seq2user == many.seq2user && one.seq2item == many.seq2item);
    CHECK(one.validation.u == many.validation.u && one.validation.i == many.validation.i && one.validation.y == many.validation.y);
    CHECK(cap_n < 100000u ? one.n == cap_n : one.n > 3000u);
  }
  unsetenv("HGAPREC_READ_THREADS"); unsetenv("HGAPREC_READ_PARALLEL_MIN");
  // start state: 70 000 elements per matrix, above the bar of the threaded half
  GammaState a, b;
  setenv("HGAPREC_SAVE_THREADS", "1", 1);
  { Mt19937 r = make_rng(3.0); initialize_state(r, 700, 300, 100, true, true, &a); }
  setenv("HGAPREC_SAVE_THREADS", "6", 1);
  { Mt19937 r = make_rng(3.0); initialize_state(r, 700, 300, 100, true, true, &b); }
  CHECK(a.theta_Elog.size() == 70000 && std::equal(a.theta_Elog.begin(), a.theta_Elog.end(), b.theta_Elog.begin()));
  CHECK(std::equal(a.theta_E.begin(), a.theta_E.end(), b.theta_E.begin()) && std::equal(a.theta_rate.begin(), a.theta_rate.end(), b.theta_rate.begin()));
  CHECK(std::equal(a.beta_Elog.begin(), a.beta_Elog.end(), b.beta_Elog.begin()));
  // three matrices side by side, each formatted on several threads while its previous wave is written
  const uint32_t rows = 30000, cols = 80;                   // 2.4 M numbers: above the bar of the threaded writer
  std::vector<double> mtx((size_t)rows * cols);
  for (auto &v : mtx) v = (double)(g() % 100000u) / 977.0;
  setenv("HGAPREC_SAVE_THREADS", "1", 1);
  CHECK(save_matrix(path("solo.tsv"), mtx.data(), rows, cols, nullptr, 0) == 0);
  setenv("HGAPREC_SAVE_THREADS", "4", 1);
  {
    std::vector<std::thread> th;
    int bad[3] = {0, 0, 0};
    for (int j = 0; j < 3; ++j)
      th.emplace_back([&, j]() { bad[j] = save_matrix(path(("side" + std::to_string(j) + ".tsv").c_str()), mtx.data(), rows, cols, nullptr, 0, 0, 4); });
    for (auto &t : th) t.join();
    const std::string want = read_text(path("solo.tsv"));
    for (int j = 0; j < 3; ++j) CHECK(bad[j] == 0 && read_text(path(("side" + std::to_string(j) + ".tsv").c_str())) == want);
  }
  unsetenv("HGAPREC_SAVE_THREADS");
}

// ---- model reader: what the writers wrote, hostile text, pieces on threads ----
static void test_loader()
{
  const uint32_t rows = 257, cols = 9;
  std::vector<double> mtx((size_t)rows * cols), back((size_t)rows * cols, -1.0);
  std::vector<uint32_t> ids(rows);
  for (size_t e = 0; e < mtx.size(); ++e) mtx[e] = (double)((e * 2654435761u) % 1000003u) / 1024.0;
  for (uint32_t r = 0; r < rows; ++r) ids[r] = 7u * r + 3u;
  CHECK(save_matrix(path("load.tsv"), mtx.data(), rows, cols, ids.data(), rows, 0, 1) == 0);
  std::string err;
  for (int threaded = 0; threaded < 2; ++threaded) {
    if (threaded) { setenv("HGAPREC_READ_PARALLEL_MIN", "1", 1); setenv("HGAPREC_READ_THREADS", "5", 1); }
    std::fill(back.begin(), back.end(), -1.0);
    CHECK(load_matrix(path("load.tsv"), back.data(), rows, cols, ids.data(), rows, &err) == 0);
    bool close = true;
    for (size_t e = 0; e < mtx.size(); ++e) close = close && std::fabs(back[e] - mtx[e]) <= 5.001e-9;        // %.8f, plus the rounding of the parsed decimal
    CHECK(close);
    CHECK(load_matrix(path("load.tsv"), back.data(), rows + 1, cols, nullptr, 0, &err) != 0 && err.find("257 rows") != std::string::npos);
    CHECK(load_matrix(path("load.tsv"), back.data(), rows, cols + 1, nullptr, 0, &err) != 0 && err.find("line 1:") != std::string::npos);
    ids[200] ^= 1u;
    CHECK(load_matrix(path("load.tsv"), back.data(), rows, cols, ids.data(), rows, &err) != 0 && err.find("line 201:") != std::string::npos);
    ids[200] ^= 1u;
  }
  unsetenv("HGAPREC_READ_PARALLEL_MIN"); unsetenv("HGAPREC_READ_THREADS");
  CHECK(load_matrix(path("no-such-model.tsv"), back.data(), 1, 1, nullptr, 0, &err) != 0 && err.find("cannot open") != std::string::npos);
  // text the writers never produce: no final newline, a lone sign, letters, an empty file, only newlines
  double v[4] = {0, 0, 0, 0};
  write_text(path("tail.tsv"), "0\t5\t1.5\n1\t6\t2.5");
  CHECK(load_vector(path("tail.tsv"), v, 2, nullptr, 0, &err) == 0 && v[0] == 1.5 && v[1] == 2.5);
  write_text(path("sign.tsv"), "0\t5\t-");
  CHECK(load_vector(path("sign.tsv"), v, 1, nullptr, 0, &err) != 0);
  write_text(path("junk.tsv"), "0\t5\tabc\n\n\n");
  CHECK(load_vector(path("junk.tsv"), v, 1, nullptr, 0, &err) != 0 && err.find("line 1:") != std::string::npos);
  CHECK(load_vector(path("junk.tsv"), v, 3, nullptr, 0, &err) != 0);
  write_text(path("empty.tsv"), "");
  CHECK(load_vector(path("empty.tsv"), v, 1, nullptr, 0, &err) != 0 && load_vector(path("empty.tsv"), v, 0, nullptr, 0, &err) == 0);
  write_text(path("nl.tsv"), "\n\n");
  CHECK(load_vector(path("nl.tsv"), v, 2, nullptr, 0, &err) != 0 && err.find("line 1:") != std::string::npos);
  // values outside a Gamma's domain, as the first row, a middle row and a last line without '\n'; one piece and several
  const char *bad[] = {"-1", "nan", "inf", "-inf", "-1e-320", "NAN(7)", "-nan", "1e999"};
  for (int threaded = 0; threaded < 2; ++threaded) {
    if (threaded) { setenv("HGAPREC_READ_PARALLEL_MIN", "0", 1); setenv("HGAPREC_READ_THREADS", "3", 1); }
    for (const char *b : bad)
      for (int at : {0, 20, 39}) {                              // 40 lines of ~20 bytes: three pieces when threaded
        std::string text;
        for (int r = 0; r < 40; ++r)                            // the last line is bad too: the first in file order is reported
          text += std::to_string(r) + "\t" + std::to_string(r + 5) + "\t0.50000000\t" + ((r == at || r == 39) ? b : "0.25") + (r == 39 ? "" : "\n");
        write_text(path("domain.tsv"), text);
        double w[80];
        CHECK(load_matrix(path("domain.tsv"), w, 40, 2, nullptr, 0, &err) != 0 &&
              err.find("line " + std::to_string(at + 1) + ":") != std::string::npos && err.find("(finite, >= 0)") != std::string::npos);
        CHECK(load_matrix(path("domain.tsv"), w, 40, 1, nullptr, 0, &err) == 0);      // the bad column is beyond `cols`: ignored
      }
    write_text(path("edge.tsv"), "0\t5\t0\n1\t6\t-0.0\n2\t7\t1e-320");
    CHECK(load_vector(path("edge.tsv"), v, 3, nullptr, 0, &err) == 0 && v[0] == 0.0 && v[1] == 0.0 && std::signbit(v[1]) && v[2] > 0.0 && v[2] < 1e-319);
  }
  unsetenv("HGAPREC_READ_PARALLEL_MIN"); unsetenv("HGAPREC_READ_THREADS");
  double E[4] = {1.0, 2.0, 3.0, 0.0}, rate[2] = {2.0, 0.0};
  CHECK(shape_over_rate(E, 2, 2, rate, "beta_rate.tsv", &err) != 0 && err.find("beta_rate.tsv: line 2:") != std::string::npos && E[0] == 1.0);
  rate[1] = std::nan("");
  CHECK(shape_over_rate(E, 2, 2, rate, "beta_rate.tsv", &err) != 0 && err.find("line 2:") != std::string::npos);
  rate[1] = 4.0;
  CHECK(shape_over_rate(E, 2, 2, rate, "beta_rate.tsv", &err) == 0 && E[0] == 0.5 && E[1] == 0.5 && E[2] == 1.5 && E[3] == 0.0);
}

// ---- the loops the reports share: chunk walk, mask lists, Ratings::r / ranked_items, list writer, expectations ----
static void test_reports()
{
  // a dozen users by hand: user 1 and 5 and 8 have no validation item, user 2 has several and no training item, user 3 a
  // duplicated pair (last rating 2), user 6 a stored rating of 0
  const uint32_t n = 12, m = 9;
  const std::vector<std::vector<std::pair<uint32_t, uint8_t>>> rows = {
    {{0, 3}, {2, 1}, {5, 2}}, {{1, 1}}, {}, {{4, 5}, {7, 1}, {4, 2}}, {{0, 1}, {1, 1}, {2, 1}, {3, 1}}, {{8, 4}},
    {{6, 0}, {7, 3}}, {{3, 2}}, {{0, 1}, {8, 1}}, {{5, 5}}, {{2, 2}, {3, 3}}, {{7, 1}}};
  const std::vector<std::vector<uint32_t>> valid = {{1}, {}, {0, 4, 7}, {0}, {5, 6}, {}, {2}, {0, 1}, {}, {3}, {8}, {0}};
  Ratings rt; rt.n = n; rt.m = m; rt.rowptr.assign(1, 0);
  std::vector<std::vector<uint32_t>> dense(n, std::vector<uint32_t>(m, 0));
  std::vector<uint32_t> deg(m, 0);
  for (uint32_t u = 0; u < n; ++u) {
    for (auto &e : rows[u]) { rt.col.push_back(e.first); rt.val.push_back(e.second); dense[u][e.first] = e.second; deg[e.first]++; }
    rt.rowptr.push_back((int64_t)rt.col.size());
    for (uint32_t it : valid[u]) { rt.validation.u.push_back(u); rt.validation.i.push_back(it); rt.validation.y.push_back(1); }
    rt.seq2user.push_back(100 + 3 * u);
  }
  for (uint32_t i = 0; i < m; ++i) rt.seq2item.push_back(900 - i);

  // Ratings::r, ranked_items, item_degrees against the dense matrix
  for (uint32_t u = 0; u < n; ++u) {
    uint32_t pos = 0;
    for (uint32_t i = 0; i < m; ++i) { CHECK(rt.r(u, i) == dense[u][i]); pos += dense[u][i] > 0; }
    CHECK(rt.ranked_items(u) == m - pos);
  }
  CHECK(rt.r(3, 4) == 2 && rt.ranked_items(2) == m && rt.ranked_items(6) == m - 1 && rt.item_degrees() == deg);

  // the walk: every row once, in order; nothing for no rows; 65 536 rows a chunk unless told otherwise
  for (size_t total : {(size_t)0, (size_t)1, (size_t)12, (size_t)13})
    for (size_t ch : {(size_t)1, (size_t)3, (size_t)5, (size_t)12, (size_t)100}) {
      size_t next = 0, visits = 0;
      for_chunks(total, [&](size_t r0, size_t r1) { CHECK(r0 == next && r1 > r0 && r1 - r0 <= ch && r1 <= total); next = r1; ++visits; }, ch);
      CHECK(next == total && visits == (total + ch - 1) / ch);
    }
  {
    std::vector<std::pair<size_t, size_t>> seen;
    for_chunks(70000, [&](size_t r0, size_t r1) { seen.push_back({r0, r1}); });
    CHECK(seen.size() == 2 && seen[0] == std::make_pair((size_t)0, (size_t)65536) && seen[1] == std::make_pair((size_t)65536, (size_t)70000));
  }

  // mask lists and -eval-all's query offsets, chunk by chunk, put together again == the one-chunk result == the lists above
  const std::vector<uint32_t> scattered = {9, 2, 4, 0, 11, 7, 2, 5};
  for (int use_list = 0; use_list < 2; ++use_list) {
    const size_t cnt = use_list ? scattered.size() : n;
    auto user_at = [&](size_t b) { return use_list ? scattered[b] : (uint32_t)b; };
    std::vector<uint64_t> qptr(1, 0);                       // 0, 1, 2, 0, 1, ... queries a user
    for (size_t b = 0; b < cnt; ++b) qptr.push_back(qptr.back() + (user_at(b) + b) % 3);
    MaskLists one;
    one.fill(rt.validation, use_list ? scattered.data() : nullptr, use_list ? cnt : 0, 0, n);
    CHECK(one.users.size() == cnt && one.ptr.size() == cnt + 1 && one.ptr[0] == 0);
    for (size_t b = 0; b < cnt && b < one.users.size(); ++b) {
      CHECK(one.users[b] == user_at(b));
      CHECK(std::vector<uint32_t>(one.items.begin() + one.ptr[b], one.items.begin() + one.ptr[b + 1]) == valid[user_at(b)]);
    }
    for (size_t ch : {(size_t)1, (size_t)3, (size_t)5, (size_t)12, (size_t)64}) {
      MaskLists cat, ml; std::vector<uint64_t> cq, catq(1, 0);
      cat.ptr.assign(1, 0);
      for_chunks(cnt, [&](size_t b0, size_t b1) {
        if (use_list) ml.fill(rt.validation, scattered.data() + b0, b1 - b0, 0, n);
        else ml.fill(rt.validation, nullptr, 0, (uint32_t)b0, (uint32_t)b1);
        CHECK(ml.ptr.size() == b1 - b0 + 1 && ml.ptr[0] == 0 && ml.ptr.back() == ml.items.size());
        cat.users.insert(cat.users.end(), ml.users.begin(), ml.users.end());
        for (size_t j = 1; j < ml.ptr.size(); ++j) cat.ptr.push_back(cat.items.size() + ml.ptr[j]);
        cat.items.insert(cat.items.end(), ml.items.begin(), ml.items.end());
        chunk_offsets(qptr.data(), b0, b1, &cq);
        CHECK(cq.size() == b1 - b0 + 1 && cq[0] == 0);
        for (size_t j = 1; j < cq.size(); ++j) catq.push_back(qptr[b0] + cq[j]);
      }, ch);
      CHECK(cat.users == one.users && cat.ptr == one.ptr && cat.items == one.items && catq == qptr);
    }
  }
  {
    MaskLists ml;                                           // a rank's part of a sample: users outside [3, 9) dropped, the rest local
    ml.fill(rt.validation, scattered.data(), scattered.size(), 3, 9, 3);
    CHECK((ml.users == std::vector<uint32_t>{1, 4, 2}) && (ml.items == std::vector<uint32_t>{5, 6, 0, 1}) &&
          (ml.ptr == std::vector<uint64_t>{0, 2, 4, 4}));
  }

  // the transposed lists (-audience): the validation users of every item, ascending; chunk by chunk == the one-chunk result
  {
    std::vector<std::vector<uint32_t>> by_item(m);
    for (uint32_t u = 0; u < n; ++u) for (uint32_t it : valid[u]) by_item[it].push_back(u);
    ItemMaskLists one;
    one.fill(rt.validation, 0, m);
    CHECK(one.items.size() == m && one.ptr.size() == (size_t)m + 1 && one.ptr[0] == 0 && one.ptr.back() == one.users.size());
    for (uint32_t it = 0; it < m && it < one.items.size(); ++it) {
      CHECK(one.items[it] == it);
      CHECK(std::vector<uint32_t>(one.users.begin() + one.ptr[it], one.users.begin() + one.ptr[it + 1]) == by_item[it]);
    }
    for (size_t ch : {(size_t)1, (size_t)3, (size_t)5, (size_t)64}) {
      ItemMaskLists cat, ml;
      cat.ptr.assign(1, 0);
      for_chunks(m, [&](size_t i0, size_t i1) {
        ml.fill(rt.validation, (uint32_t)i0, (uint32_t)i1);
        CHECK(ml.ptr.size() == i1 - i0 + 1 && ml.ptr[0] == 0 && ml.ptr.back() == ml.users.size());
        cat.items.insert(cat.items.end(), ml.items.begin(), ml.items.end());
        for (size_t j = 1; j < ml.ptr.size(); ++j) cat.ptr.push_back(cat.users.size() + ml.ptr[j]);
        cat.users.insert(cat.users.end(), ml.users.begin(), ml.users.end());
      }, ch);
      CHECK(cat.items == one.items && cat.ptr == one.ptr && cat.users == one.users);
    }
    ItemMaskLists none;
    none.fill(HeldOut(), 2, 5);                             // no pairs, and an empty range
    CHECK(none.items == (std::vector<uint32_t>{2, 3, 4}) && none.users.empty() && none.ptr == (std::vector<uint64_t>{0, 0, 0, 0}));
    none.fill(rt.validation, 4, 4);
    CHECK(none.items.empty() && none.users.empty() && none.ptr == (std::vector<uint64_t>{0}));
  }

  // the list writer: only the real entries, only what the predicate keeps, the line count
  {
    const uint32_t N = 4, bad = 0xffffffffu;
    const std::vector<uint32_t> sel = {3, 0, 2};
    for (uint32_t real : {0u, 2u, 4u, 9u}) {
      const uint32_t shown = std::min(real, N);
      std::vector<uint32_t> items = {4, 1, 7, 8, 5, 0, 6, 2, 3, 3, 0, 1};
      std::vector<double> scores(items.size());
      for (size_t e = 0; e < items.size(); ++e) { scores[e] = 1.0 / (double)(e + 3); if (e % N >= shown) items[e] = bad; }   // padding: never looked at
      for (int with_keep = 0; with_keep < 2; ++with_keep) {
        std::string want; uint64_t want_lines = 0; char line[96];
        for (size_t b = 0; b < sel.size(); ++b)
          for (uint32_t j = 0; j < shown; ++j) {
            const uint32_t it = items[b * N + j];
            if (with_keep && dense[sel[b]][it] != 0) continue;
            snprintf(line, sizeof line, "%d\t%d\t%.5f\n", rt.seq2user[sel[b]], rt.seq2item[it], scores[b * N + j]);
            want += line; ++want_lines;
          }
        FILE *f = fopen(path("topn.tsv").c_str(), "w");
        CHECK(f != nullptr);
        if (!f) continue;
        const uint64_t lines = with_keep
          ? write_topn(f, sel.data(), sel.size(), items.data(), scores.data(), N, real, rt.seq2user.data(), rt.seq2item.data(),
                       [&](uint32_t u, uint32_t it) { return rt.r(u, it) == 0; })
          : write_topn(f, sel.data(), sel.size(), items.data(), scores.data(), N, real, rt.seq2user.data(), rt.seq2item.data());
        fclose(f);
        CHECK(lines == want_lines && read_text(path("topn.tsv")) == want);
        if (real == 4) CHECK(with_keep ? lines == 7 : lines == 12);     // (3,4), (3,7), (0,5), (0,0), (0,2) are training pairs
      }
    }
  }

  // Gamma expectations: the formula, the rate as a matrix and as a K-vector, the domain
  {
    const size_t R = 3, K = 2;
    const double shape[6] = {0.3, 1.5, 2.0, 7.25, 1e-3, 40.0}, rmat[6] = {0.5, 2.0, 1.0, 3.5, 1e-2, 8.0}, rvec[2] = {0.75, 4.0};
    std::string err;
    for (int vec = 0; vec < 2; ++vec) {
      double E[6], L[6];
      memcpy(E, shape, sizeof E);
      CHECK(gamma_expectations(E, L, vec ? rvec : rmat, R, K, vec != 0, "hbeta_rate.tsv", &err) == 0);
      for (size_t e = 0; e < 6; ++e) {
        const double rv = vec ? rvec[e % K] : rmat[e];
        CHECK(E[e] == shape[e] / rv && L[e] == digamma(shape[e]) - std::log(rv));
      }
      for (double v : {0.0, -1.0, (double)NAN})
        for (int in_rate = 0; in_rate < 2; ++in_rate) {
          double r2[6];
          memcpy(E, shape, sizeof E); memcpy(r2, rmat, sizeof r2);
          if (in_rate) { if (vec) { r2[0] = rvec[0]; r2[1] = v; } else r2[5] = v; } else E[5] = v;
          // the bad value is in row 2 -- a bad entry of the K-vector shows in row 0 already
          CHECK(gamma_expectations(E, L, r2, R, K, vec != 0, "some/hbeta_rate.tsv", &err) == -1);
          CHECK(err.find("some/hbeta_rate.tsv: ") == 0 && err.find(in_rate && vec ? "(row 0)" : "(row 2)") != std::string::npos);
        }
    }
  }
}

int main(int argc, char **argv)
{
  char tmpl[] = "/tmp/hgaprec_selftest_XXXXXX";
  const char *d = argc > 1 ? argv[1] : mkdtemp(tmpl);
  if (!d) { perror("mkdtemp"); return 2; }
  g_dir = d;
  test_idmap();
  test_env();
  test_reader();
  test_fold_in_reader();
  test_cache();
  test_writers();
  test_state();
  test_threads();
  test_loader();
  test_reports();
  test_comm();
  if (g_fail) { fprintf(stderr, "host_selftest: %d check(s) failed\n", g_fail); return 1; }
  printf("host_selftest ok\n");
  return 0;
}
