// hgaprec_main.cpp -- the `hgaprec` command line on MI355X.
//
// Same flags, input files and output files as the reference's src/main.cc +
// HGAPRec::vb_hier / vb / vb_bias (hgaprec.cc:1321-1436, 919-980, 1219-1319);
// the CAVI sweeps, the held-out likelihood, the ELBO and the ranking
// evaluation run on the GPU through include/hpf.h.  What stays on the host is
// what the reference also does outside the hot loop: parsing, TSV I/O, the
// MT19937 start state, the report series and their stop rule.
//
// Extension: `-ngpus N` shards the users over N GPUs of the node, one process
// per GPU (the parent re-executes itself N times); per iteration the item-side
// sums go through one RCCL all-reduce (`-comm rccl`, default) or a host-staged
// stand-in (`-comm host`, for tests on a single GPU).  The output files are
// the same as in a single-GPU run.
//
// Scoring a saved model (-gen-ranking / -rmse / -msr / -eval-all / -recommend [-explain] [-because] [-ucb] [-thompson] [-diverse] / -fold-in / -fold-in-items / -similar-items /
// -similar-users / -topic-items / -topic-users / -audience [-explain]) sets the run up the same way and then writes ONE report instead of training: score(), score_modes.cpp.
// What both halves share -- flags, ratings, handle, the ways to fail -- is struct Cli (hgaprec_cli.hpp).
//
// Out of scope: competitor bridges, MLE/Canny ablations, -test; their
// flags are recognised and refused.
#include "hgaprec_cli.hpp"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <chrono>
#include <csignal>
#include <ctime>
#include <mutex>
#include <set>
#include <fcntl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <thread>
#include <unistd.h>
#include <vector>

using namespace hgaprec;

static volatile sig_atomic_t g_save_state_now = 0;
static void term_handler(int) { g_save_state_now = 1; }   // main.cc:19-30

namespace {

// HPF_CLI_TIMING=1: wall seconds of each phase of the run on stderr (tools/cli_walltime.py reads them)
struct PhaseClock {
  bool on = getenv("HPF_CLI_TIMING") != nullptr;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double acc_get = 0, acc_join = 0;     // inside save_model: hpf_get_state, waiting for the file writers after the last fetch
  double acc_iter = 0, acc_report = 0, acc_part[5] = {0, 0, 0, 0, 0};   // parts: likelihood, save_model, precision, itemrank, on stop
  std::chrono::steady_clock::time_point p0;
  void part_begin() { p0 = std::chrono::steady_clock::now(); }
  void part_end(int j) { acc_part[j] += std::chrono::duration<double>(std::chrono::steady_clock::now() - p0).count(); }
  double lap() {
    const auto t1 = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
    return s;
  }
  static double epoch() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }
  void stamp(const char *what) { if (on) fprintf(stderr, "[timing-epoch] %s %.6f\n", what, epoch()); }   // for the caller's own clock (tools/cli_walltime.py)
  double acc_other = 0;                 // time between the named phases (logging, small files, frees)
  void other() { acc_other += lap(); }
  void mark(const char *what) { const double s = lap(); if (on) fprintf(stderr, "[timing] %-28s %9.3f s\n", what, s); }
  void totals(uint32_t iterations) {
    if (!on) return;
    fprintf(stderr, "[timing] %-28s %9.3f s\n[timing] %-28s %9.3f s\n[timing] %-28s %9u\n", "iterations (hpf_iterate)", acc_iter,
            "report steps + saves", acc_report, "iterations run", iterations);
    const char *nm[5] = {"  held-out likelihood", "  save_model", "  compute_precision", "  compute_itemrank", "  on stop (save + ranking)"};
    for (int j = 0; j < 5; ++j) fprintf(stderr, "[timing] %-28s %9.3f s\n", nm[j], acc_part[j]);
    fprintf(stderr, "[timing] %-28s %9.3f s\n[timing] %-28s %9.3f s\n", "  saves: hpf_get_state", acc_get, "  saves: waiting for writers", acc_join);
    fprintf(stderr, "[timing] %-28s %9.3f s\n", "between the phases", acc_other);
  }
};
PhaseClock g_clock;

// A host buffer that is used again and again as the target of hpf_get_state: page-locked when the library can give
// that (the DMA then writes it directly, hpf.h hpf_host_alloc), ordinary memory otherwise.  Never shrinks.
struct SaveBuf {
  double *p = nullptr; size_t cap = 0; bool pinned = false;
  double *data() const { return p; }
  void reserve(size_t cnt) {
    if (cnt <= cap) return;
    release();
    void *q = nullptr;
    if (hpf_host_alloc(&q, cnt * sizeof(double)) == HPF_OK) { p = (double *)q; pinned = true; }
    else { p = (double *)malloc(cnt * sizeof(double)); pinned = false; }
    if (!p) { fprintf(stderr, "error: out of host memory (%zu doubles)\n", cnt); exit(1); }
    cap = cnt;
  }
  void release() {
    if (p) { if (pinned) hpf_host_free(p); else free(p); }
    p = nullptr; cap = 0;
  }
  ~SaveBuf() { release(); }
  SaveBuf() = default;
  SaveBuf(const SaveBuf &) = delete;
  SaveBuf &operator=(const SaveBuf &) = delete;
};

// part files of this rank, unlinked by an atexit hook (and, after a good run, by rank 0 behind the last barrier)
static std::mutex g_parts_mu;
static std::set<std::string> *g_own_parts = nullptr;
static void unlink_own_parts() {
  std::lock_guard<std::mutex> lk(g_parts_mu);
  if (!g_own_parts) return;
  for (const std::string &p : *g_own_parts) { unlink(p.c_str()); unlink(rewrite_marker(p).c_str()); }
  g_own_parts->clear();
}
static void own_part(const std::string &p) {
  std::lock_guard<std::mutex> lk(g_parts_mu);
  if (!g_own_parts) { g_own_parts = new std::set<std::string>(); atexit(unlink_own_parts); }
  g_own_parts->insert(p);
}

struct Driver : Cli {
  Comm &comm;
  uint32_t n, m, k, iter = 0;          // n: ALL users; lo..hi: this rank's range
  uint32_t lo = 0, hi = 0;
  bool use_rccl = false;
  bool fallback_logged = false;
  time_t start;
  FILE *vf = nullptr, *tf = nullptr, *af = nullptr, *pf = nullptr;
  StopRule stop;
  Mt19937 rng;                         // gsl_rng *_r: keeps running after initialize()
  std::vector<uint32_t> sampled;       // _sampled_users (std::map keys: sorted, unique), GLOBAL seq ids
  HeldOut lvalid, ltest;               // this rank's held-out pairs, LOCAL user indices
  std::vector<double> xbuf;            // host staging of the exchange buffer (-comm host)
  SaveBuf save_u[3], save_i[3];        // host copies of an object's shape / rate / expectation while they are written
  std::set<std::string> part_files;    // (rank 0, several ranks) files whose per-rank parts are lying beside them until the run ends
  std::thread save_prealloc;           // page-locking them (0.2 s per GB) runs beside the start state, not inside the first save

  Driver(Env &e, Ratings &r, Comm &c) : Cli(e, r, c.rank), comm(c), n(r.n), m(r.m), k(e.k), start(time(0)) {}

  bool root() const { return comm.rank == 0; }
  uint32_t duration() const { return (uint32_t)(time(0) - start); }      // hgaprec.hh:164-169

  void comm_check(int rc, const char *what) {
    if (rc) { fprintf(stderr, "error: [rank %d] %s: peer lost\n", comm.rank, what); exit(-1); }
  }

  static void slice(const HeldOut &src, uint32_t a, uint32_t b, HeldOut *dst) {
    dst->u.clear(); dst->i.clear(); dst->y.clear();
    for (size_t p = 0; p < src.u.size(); ++p)
      if (src.u[p] >= a && src.u[p] < b) { dst->u.push_back(src.u[p] - a); dst->i.push_back(src.i[p]); dst->y.push_back(src.y[p]); }
  }

  // HGAPRec::HGAPRec (hgaprec.cc:8-98): output files, held-out sets, prior log
  void construct() {
    if (root()) {
      env.plog("infer n:", n);
      const char *names[] = {"/heldout.txt", "/validation.txt", "/test.txt", "/logl.txt",
                             "/precision.txt", "/ndcg.txt", "/rmse.txt"};
      for (const char *nm : names) {
        FILE *f = fopen(env.file_str(nm).c_str(), env.resume ? "a" : "w");
        if (!f) { printf("cannot open heldout file:%s\n", strerror(errno)); exit(-1); }
        if (!strcmp(nm, "/validation.txt")) vf = f;
        else if (!strcmp(nm, "/test.txt")) tf = f;
        else if (!strcmp(nm, "/logl.txt")) af = f;
        else if (!strcmp(nm, "/precision.txt")) pf = f;
        else fclose(f);
      }
    }
    // load_validation_and_test_sets (hgaprec.cc:110-151): both must open
    g_clock.other();
    if (!rt.heldout_loaded) {                     // else: came with the -cache image
      int rc = rt.read_heldout(env.datfname + "/validation.tsv", &rt.validation);
      assert(rc != -1);
      if (rc) exit(-1);
      rc = rt.read_heldout(env.datfname + "/test.tsv", &rt.test);
      assert(rc != -1);
      if (rc) exit(-1);
      if (env.data_cache && root()) {
        if (rt.save_cache(env.datfname)) env.lerr("-cache: cannot write %s/hgaprec.cache.bin", env.datfname.c_str());
        else env.lerr("-cache: wrote %s/hgaprec.cache.bin", env.datfname.c_str());
      }
    }
    if (root()) {
      printf("+ loaded validation and test sets from %s\n", env.datfname.c_str());
      fflush(stdout);
      env.plog("test ratings", (uint64_t)rt.test.u.size());
      env.plog("validation ratings", (uint64_t)rt.validation.u.size());
      if (!env.hier) {
        env.plog("theta shape:", 0.3); env.plog("theta rate:", 0.3);
        env.plog("beta shape:", 0.3); env.plog("beta rate:", 0.3);
      } else {
        env.plog("htheta shape:", 0.3); env.plog("htheta rate:", 0.3);
        env.plog("hbeta shape:", 0.3); env.plog("hbeta rate:", 0.3);
        env.plog("thetarate shape:", 0.3); env.plog("thetarate rate:", 0.3);
        env.plog("betarate shape:", 0.3); env.plog("betarate rate:", 0.3);
      }
    }

    g_clock.mark("validation.tsv + test.tsv");
    // this rank's contiguous user range, balanced on the nnz prefix sum
    const auto parts = partition_users(rt.rowptr, comm.world);
    lo = parts[comm.rank].first; hi = parts[comm.rank].second;
    if (comm.world > 1)
      fprintf(stderr, "[rank %d] users [%u, %u) of %u: %lld of %lld ratings\n", comm.rank, lo, hi, n,
              (long long)(rt.rowptr[hi] - rt.rowptr[lo]), (long long)rt.rowptr[n]);
    slice(rt.validation, lo, hi, &lvalid);
    slice(rt.test, lo, hi, &ltest);

    const hpf_config cfg = config(hi - lo, n, (uint32_t)comm.world, (uint32_t)comm.rank);
    int rc = hpf_create(&cfg, &h);
    if (rc) die("hpf_create (is an MI355X visible? there is no CPU fallback)", rc);
    std::vector<int64_t> rp(rt.rowptr.begin() + lo, rt.rowptr.begin() + hi + 1);
    const int64_t base = rp[0];
    for (auto &v : rp) v -= base;
    g_clock.mark("hpf_create (HIP start-up)");
    rc = hpf_upload_csr(h, rp.data(), rt.col.data() + base, env.binary_data ? nullptr : rt.val.data() + base);
    if (rc) die("hpf_upload_csr", rc);
    g_clock.mark("hpf_upload_csr");
    {
      hpf_work_info wi;
      if (root() && hpf_get_work_info(h, &wi) == HPF_OK)      // infer.log: how the device side laid the work out
        env.lerr("device: rows of W %s, %u columns; phi passes: user %s (%u tiles), item %s (%u tiles)",
                 wi.w_layout == 3 ? "packed 59-bit (lossless)" : wi.w_layout == 2 ? "48-bit (opt-in)" :
                 wi.w_layout == 4 ? "plain fp64 in 16-byte pieces" : "plain fp64", wi.ld,
                 wi.tiles_user ? "tiled" : "row-major", wi.tiles_user, wi.tiles_item ? "tiled" : "row-major", wi.tiles_item);
    }

    if (!env.score_mode()) save_prealloc = std::thread([this]() {     // (a score mode never saves the model)
      for (int j = 0; j < 3; ++j) {
        save_u[j].reserve((size_t)(hi - lo) * k);
        if (root()) save_i[j].reserve((size_t)m * k);
      }
    });
    if (comm.world > 1 && use_rccl) {                      // bootstrap the RCCL communicator
      char id[HPF_COMM_ID_BYTES]; memset(id, 0, sizeof id);
      if (root() && (rc = hpf_comm_unique_id(id))) die("hpf_comm_unique_id (librccl.so missing?)", rc);
      comm_check(comm.bcast(id, sizeof id), "bcast of the RCCL id");
      if ((rc = hpf_comm_init(h, id))) die("hpf_comm_init", rc);
    }
  }

  // HGAPRec::initialize (hgaprec.cc:153-204): MT19937 on the host, state to the device.
  // Every rank consumes the whole stream (same generator state everywhere afterwards).
  void initialize() {
    rng = make_rng(env.seed);
    GammaState s;
    g_clock.other();
    initialize_state(rng, n, m, k, env.hier, env.bias, &s, lo, hi);
    g_clock.mark("start state (MT19937, host)");
    put(HPF_THETA_SHAPE, s.theta_shape); put(HPF_THETA_RATE, s.theta_rate);
    put(HPF_THETA_E, s.theta_E); put(HPF_THETA_ELOG, s.theta_Elog);
    put(HPF_BETA_SHAPE, s.beta_shape); put(HPF_BETA_RATE, s.beta_rate);
    put(HPF_BETA_E, s.beta_E); put(HPF_BETA_ELOG, s.beta_Elog);
    if (env.hier) {
      put(HPF_XI_SHAPE, s.xi_shape); put(HPF_XI_RATE, s.xi_rate); put(HPF_XI_E, s.xi_E); put(HPF_XI_ELOG, s.xi_Elog);
      put(HPF_ETA_SHAPE, s.eta_shape); put(HPF_ETA_RATE, s.eta_rate); put(HPF_ETA_E, s.eta_E); put(HPF_ETA_ELOG, s.eta_Elog);
    }
    if (env.bias) {
      put(HPF_UBIAS_SHAPE, s.ubias_shape); put(HPF_UBIAS_E, s.ubias_E); put(HPF_UBIAS_ELOG, s.ubias_Elog);
      put(HPF_IBIAS_SHAPE, s.ibias_shape); put(HPF_IBIAS_E, s.ibias_E); put(HPF_IBIAS_ELOG, s.ibias_Elog);
    }
    g_clock.mark("hpf_set_state");
  }

  // -bias -novb without -hier on several ranks (vb_bias()'s else-branch, hgaprec.cc:1276-1297): the first
  // item rate takes sum_u E[theta] of the START state (_theta.sum_rows() before _theta.swap()), summed
  // over the ranks once -- hpf_start_sums leaves this rank's part in the tail of the exchange buffer
  void start_sums() {
    if (comm.world == 1 || env.vb || !env.bias || env.hier) return;
    // after -resume the tail came with the snapshot, already summed over the ranks: start_sums_pending reads 0 and the
    // tail must not be reduced a second time (it would come out world x too large -- ADVICE r4)
    hpf_work_info wi;
    int rc = hpf_get_work_info(h, &wi);
    if (rc) die("hpf_get_work_info", rc);
    const bool pending = wi.start_sums_pending != 0;
    if ((rc = hpf_start_sums(h))) die("hpf_start_sums", rc);   // with RCCL the library reduces the tail itself
    if (use_rccl || !pending) return;
    void *p; size_t cnt;
    hpf_exchange_buffer(h, &p, &cnt);
    xbuf.resize(cnt);
    if ((rc = hpf_exchange_read(h, xbuf.data(), cnt))) die("hpf_exchange_read", rc);
    comm_check(comm.allreduce_sum(xbuf.data() + (cnt - wi.ld), wi.ld), "start-state all-reduce of sum_u E[theta]");
    if ((rc = hpf_exchange_write(h, xbuf.data(), cnt))) die("hpf_exchange_write", rc);
  }

  // one CAVI iteration (steps A-F); with several ranks the item-side sums are
  // all-reduced between the local and the replicated half
  void iterate() {
    int rc;
    if (comm.world == 1) { if ((rc = hpf_iterate(h, 1))) die("hpf_iterate", rc); return; }
    if (use_rccl && env.single_allreduce) {
      // ONE fused all-reduce of [m x ld | ld] after the whole local half (BASELINE.json's wording): nothing overlaps it
      if ((rc = hpf_iterate_local_items(h))) die("hpf_iterate_local_items", rc);
      if ((rc = hpf_iterate_local_users(h))) die("hpf_iterate_local_users", rc);
      if ((rc = hpf_allreduce_exchange(h))) die("hpf_allreduce_exchange", rc);
    } else if (use_rccl) {
      // item pass, all-reduce of the item sums (m*ld doubles) on a second stream
      // underneath the user pass and the user sweep, [ld] tail, item sweep
      if ((rc = hpf_iterate(h, 1))) die("hpf_iterate", rc);
      return;
    } else {
      if ((rc = hpf_iterate_local(h))) die("hpf_iterate_local", rc);
      void *p; size_t cnt;
      hpf_exchange_buffer(h, &p, &cnt);
      xbuf.resize(cnt);
      if ((rc = hpf_exchange_read(h, xbuf.data(), cnt))) die("hpf_exchange_read", rc);
      comm_check(comm.allreduce_sum(xbuf.data(), cnt), "host-staged all-reduce");
      if ((rc = hpf_exchange_write(h, xbuf.data(), cnt))) die("hpf_exchange_write", rc);
    }
    if ((rc = hpf_iterate_global(h))) die("hpf_iterate_global", rc);
  }

  // ---- output of sharded objects: every rank writes its rows to a part
  // file, rank 0 concatenates them in rank (= row) order
  std::string part_name(const std::string &path, int r) const { return path + ".part" + std::to_string(r); }
  // The files of one object at once: one barrier in front, one behind; rank 0 copies the parts of each file
  // into it on a thread of its own, inside the kernel (copy_file_range) and over the file's old contents --
  // like the parts themselves, which are kept and rewritten in place until the run ends (finish()): with two ranks
  // on C2 the copy through a user-space buffer into a truncated file was 7.9 of the run's 17.6 seconds.
  // errno-style result: 0, or -1 with *bad naming the file that failed.
  static int concat_parts(const std::string &path, const std::vector<std::string> &parts, std::string *bad) {
    const int out = ::open(path.c_str(), O_WRONLY | O_CREAT | O_CLOEXEC, 0666);
    if (out < 0) { *bad = path; return -1; }
    // "<path>.writing" until the file is whole (hgaprec_host.cpp open_rewrite) -- after the open has succeeded (a target
    // that cannot be opened is an old file nobody touched) and only beside a regular file
    struct stat ost;
    const bool regular = fstat(out, &ost) == 0 && S_ISREG(ost.st_mode);
    if (regular) rewrite_begin(path);
    off_t total = 0;
    bool in_kernel = true;
    std::vector<char> buf;
    for (const std::string &pn : parts) {
      const int in = ::open(pn.c_str(), O_RDONLY | O_CLOEXEC);
      struct stat st;
      if (in < 0 || fstat(in, &st) != 0) { if (in >= 0) ::close(in); ::close(out); *bad = pn; return -1; }   // every rank writes one, even if empty
      off_t left = st.st_size;
      while (left > 0 && in_kernel) {
        const ssize_t got = copy_file_range(in, nullptr, out, nullptr, (size_t)std::min<off_t>(left, (off_t)1 << 30), 0);
        if (got > 0) { left -= got; total += got; continue; }
        if (got == 0) { ::close(in); ::close(out); *bad = pn; errno = EIO; return -1; }                 // the part is shorter than it was a moment ago
        if (errno == EINTR) continue;
        if (left == st.st_size && (errno == EXDEV || errno == EINVAL || errno == ENOSYS || errno == EOPNOTSUPP)) in_kernel = false;   // this file system cannot: copy by hand
        else { ::close(in); ::close(out); *bad = path; return -1; }
      }
      if (left > 0) {
        if (buf.empty()) buf.resize((size_t)8 << 20);
        while (left > 0) {
          const ssize_t got = ::read(in, buf.data(), (size_t)std::min<off_t>(left, (off_t)buf.size()));
          if (got < 0 && errno == EINTR) continue;
          if (got <= 0) { ::close(in); ::close(out); *bad = pn; if (!got) errno = EIO; return -1; }
          for (ssize_t w = 0; w < got;) {
            const ssize_t put = ::write(out, buf.data() + w, (size_t)(got - w));
            if (put < 0 && errno == EINTR) continue;
            if (put <= 0) { ::close(in); ::close(out); *bad = path; return -1; }
            w += put;
          }
          left -= got; total += got;
        }
      }
      ::close(in);
    }
    const bool ok = !regular || ftruncate(out, total) == 0;
    if (::close(out) != 0 || !ok) { *bad = path; return -1; }
    if (regular) rewrite_end(path);
    return 0;
  }
  void finish_parts(const std::vector<std::string> &paths) {
    if (comm.world == 1 || paths.empty()) return;
    comm_check(comm.barrier(), "barrier");
    if (root()) {
      std::vector<std::thread> th;
      std::vector<int> rc(paths.size(), 0), err(paths.size(), 0);
      std::vector<std::string> bad(paths.size());
      for (size_t j = 0; j < paths.size(); ++j) {
        part_files.insert(paths[j]);
        th.emplace_back([&, j]() {
          std::vector<std::string> parts;
          for (int r = 0; r < comm.world; ++r) parts.push_back(part_name(paths[j], r));
          rc[j] = concat_parts(paths[j], parts, &bad[j]);
          err[j] = errno;
        });
      }
      for (auto &t : th) t.join();
      for (size_t j = 0; j < paths.size(); ++j) if (rc[j]) { errno = err[j]; io_die("cannot put the part files together:", bad[j]); }
    }
    comm_check(comm.barrier(), "barrier");
  }
  void finish_parts(const std::string &path) { finish_parts(std::vector<std::string>{path}); }
  void remove_part_files() {                    // end of the run, every rank behind the barrier of finish()
    for (const std::string &p : part_files)
      for (int r = 0; r < comm.world; ++r) unlink(part_name(p, r).c_str());
    part_files.clear();
  }
  // a part file this rank has written is removed when the process exits, however it exits (die / io_die / a lost peer
  // all go through exit()): a failed run of several ranks used to leave every part lying in the output directory --
  // at C2 three times 1.1 GB of text per object.  While the run lasts the parts double the disk space of
  // the user-side objects (README).
  std::string my_path(const std::string &path) const {
    if (comm.world == 1) return path;
    const std::string p = part_name(path, comm.rank);
    own_part(p);
    return p;
  }

  // GP*::save_state (gpbase.hh:389-398,743-752,971-980).  The three matrices of an object (shape, rate,
  // expectation) are fetched one after the other and written SIDE BY SIDE, a thread per file: one file's
  // buffered writes are serial in the kernel, three files' are not, and at C2 a save is 3.3 GB of text
  // whose formatting already runs on all threads (hgaprec_host.cpp save_matrix).
  void save_object(const char *name, hpf_state shape, bool user_side, uint32_t cols, bool vec_rate) {
    const uint32_t rows = user_side ? hi - lo : m, row0 = user_side ? lo : 0;
    const std::vector<uint32_t> &ids = user_side ? rt.seq2user : rt.seq2item;
    const bool mine = user_side || root();       // item-side state is replicated: rank 0 writes it
    const std::string base = env.file_str(std::string("/") + name);
    if (save_prealloc.joinable()) save_prealloc.join();
    SaveBuf *buf = user_side ? save_u : save_i;   // kept between saves: 2.9 GB of fresh pages per report otherwise
    auto get = [&](SaveBuf &b, hpf_state w, size_t cnt) {
      const auto t0 = std::chrono::steady_clock::now();
      b.reserve(cnt);
      int rc = hpf_get_state(h, w, b.data(), cnt);
      if (rc) die("hpf_get_state", rc);
      g_clock.acc_get += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    };
    const char *suf[3] = {"_shape.tsv", "_rate.tsv", ".tsv"};
    std::string dst[3];
    int failed[3] = {0, 0, 0};
    std::vector<std::thread> writers;
    const unsigned per_file = std::max(1u, std::thread::hardware_concurrency() / 3);
    for (int j = 0; j < 3; ++j) {
      const std::string path = base + suf[j];
      const bool vec = j == 1 && vec_rate;       // GPMatrixGR rate: K-vector, ids looked up by k
      if (vec) {
        if (root()) {
          get(buf[j], (hpf_state)(shape + 1), cols);
          if (save_vector(path, buf[j].data(), cols, ids.data(), (uint32_t)ids.size())) io_die("cannot write", path);
        }
        continue;
      }
      if (!mine) continue;
      get(buf[j], (hpf_state)(shape + j), (size_t)rows * cols);
      dst[j] = user_side ? my_path(path) : path;
      const double *a = buf[j].data();
      const std::string *d = &dst[j];
      int *bad = &failed[j];
      const std::vector<uint32_t> *idv = &ids;
      writers.emplace_back([=]() { *bad = save_matrix(*d, a, rows, cols, idv->data(), (uint32_t)idv->size(), row0, per_file); });
    }
    const auto tw = std::chrono::steady_clock::now();
    for (auto &w : writers) w.join();
    g_clock.acc_join += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    for (int j = 0; j < 3; ++j) if (failed[j]) io_die("cannot write", dst[j]);
    if (user_side) {
      std::vector<std::string> whole;
      for (int j = 0; j < 3; ++j) if (!(j == 1 && vec_rate)) whole.push_back(base + suf[j]);
      finish_parts(whole);
    }
  }
  void save_array(const char *name, hpf_state shape, bool user_side) {
    const uint32_t rows = user_side ? hi - lo : m, row0 = user_side ? lo : 0;
    const std::vector<uint32_t> &ids = user_side ? rt.seq2user : rt.seq2item;
    std::vector<double> buf(rows);
    const std::string base = env.file_str(std::string("/") + name);
    const char *suf[3] = {"_shape.tsv", "_rate.tsv", ".tsv"};
    for (int j = 0; j < 3; ++j) {
      const std::string path = base + suf[j];
      if (user_side || root()) {
        int rc = hpf_get_state(h, (hpf_state)(shape + j), buf.data(), rows);
        if (rc) die("hpf_get_state", rc);
        const std::string dst = user_side ? my_path(path) : path;
        if (save_vector(dst, buf.data(), rows, ids.data(), (uint32_t)ids.size(), row0)) io_die("cannot write", dst);
      }
    }
    if (user_side) finish_parts({base + suf[0], base + suf[1], base + suf[2]});
  }

  void save_model() {                           // hgaprec.cc:2137-2158
    if (env.hier) {
      save_object("hbeta", HPF_BETA_SHAPE, false, k, false);
      save_array("betarate", HPF_ETA_SHAPE, false);
      save_object("htheta", HPF_THETA_SHAPE, true, k, false);
      save_array("thetarate", HPF_XI_SHAPE, true);
    } else {
      save_object("beta", HPF_BETA_SHAPE, false, k, true);
      save_object("theta", HPF_THETA_SHAPE, true, k, true);
    }
    if (env.bias) {     // n x 1 GPMatrix objects: one value column
      save_object("betabias", HPF_IBIAS_SHAPE, false, 1, false);
      save_object("thetabias", HPF_UBIAS_SHAPE, true, 1, false);
    }
  }

  // ---- ranking evaluation: compute_precision / compute_itemrank --------
  // this rank's part of the sampled users (local indices) + their validation items (is_validation())
  MaskLists local_sample() const { MaskLists ml; ml.fill(rt.validation, sampled.data(), sampled.size(), lo, hi, lo); return ml; }

  void compute_precision(bool save_ranking_file) {          // hgaprec.cc:1703-1848
    if (iter % 100 == 0 && iter > 0) save_ranking_file = true;
    const std::string rpath = env.file_str("/ranking.tsv");
    FILE *f = save_ranking_file ? open_or_die(my_path(rpath), "w") : nullptr;
    if (!save_ranking_file) {                    // hgaprec.cc:1714-1721 (same draws on every rank)
      sampled.clear();
      do {
        const uint32_t u = (uint32_t)rng.uniform_int(n);
        auto it = std::lower_bound(sampled.begin(), sampled.end(), u);
        if (it == sampled.end() || *it != u) sampled.insert(it, u);
      } while (sampled.size() < 1000 && sampled.size() < n / 2);
    }
    const uint32_t N = 100;                      // _topN_by_user
    const MaskLists ml = local_sample();
    const std::vector<uint32_t> &lus = ml.users;
    std::vector<uint32_t> items(lus.size() * N); std::vector<double> scores(lus.size() * N);
    int rc = hpf_rank_topn(h, lus.data(), (uint32_t)lus.size(), ml.ptr.data(), ml.items.data(), N,
                           items.data(), scores.data());
    if (rc) die("hpf_rank_topn", rc);
    double acc[3] = {0, 0, 0};                   // mhits10, mhits100, total_users
    for (size_t b = 0; b < lus.size(); ++b) {
      const uint32_t u = lus[b] + lo;
      uint32_t hits10 = 0, hits100 = 0;
      for (uint32_t j = 0; j < m && j < N; ++j) {
        const uint32_t it = items[b * N + j]; const double pred = scores[b * N + j];
        int v = 0;
        const size_t a = rt.test.lower(u, it);
        if (a < rt.test.u.size() && rt.test.u[a] == u && rt.test.i[a] == it) {
          v = test_hit(rt.test.y[a]) ? 1 : 0;
          if (j < 10) { if (v > 0) { hits10++; hits100++; } }
          else if (j < 100) { if (v > 0) hits100++; }
        }
        if (f && rt.r(u, it) == 0) fprintf(f, "%d\t%d\t%.5f\t%d\n", rt.seq2user[u], rt.seq2item[it], pred, v);
      }
      acc[0] += (double)hits10 / 10; acc[1] += (double)hits100 / 100; acc[2] += 1;
    }
    if (f) close_or_die(f, my_path(rpath));
    if (save_ranking_file) finish_parts(rpath);
    comm_check(comm.allreduce_sum(acc, 3), "precision all-reduce");
    if (root()) {
      const uint32_t total_users = (uint32_t)acc[2];
      fprintf(pf, "%d\t%.5f\t%.5f\n", total_users, (double)acc[0] / total_users, (double)acc[1] / total_users);
      fflush(pf);
    }
  }

  void compute_itemrank(bool final) {                       // hgaprec.cc:1606-1701
    if (iter % 100 == 0 && iter > 0) final = true;
    if (!final) return;
    const std::string ipath = env.file_str("/itemrank.tsv");
    FILE *f = open_or_die(my_path(ipath), "w");
    const std::vector<uint32_t> &item_deg = rt.item_degrees();
    const MaskLists ml = local_sample();
    const std::vector<uint32_t> &lus = ml.users;
    std::vector<uint32_t> qs, qi;                 // one query per test item that is a hit
    for (size_t b = 0; b < lus.size(); ++b) {
      const uint32_t u = lus[b] + lo;
      for (size_t a = rt.test.lower(u, 0); a < rt.test.u.size() && rt.test.u[a] == u; ++a)
        if (test_hit(rt.test.y[a])) { qs.push_back((uint32_t)b); qi.push_back(rt.test.i[a]); }
    }
    std::vector<uint32_t> rank(qs.size()); std::vector<double> pred(qs.size());
    int rc = hpf_item_ranks(h, lus.data(), (uint32_t)lus.size(), ml.ptr.data(), ml.items.data(),
                            qs.data(), qi.data(), (uint32_t)qs.size(), rank.data(), pred.data());
    if (rc) die("hpf_item_ranks", rc);
    double acc[3] = {0, 0, 0};                   // sum_rank, sum_reciprocal_rank, total_users
    std::vector<uint32_t> ord;
    for (size_t b = 0, q0 = 0; b < lus.size(); ++b) {
      size_t q1 = q0; while (q1 < qs.size() && qs[q1] == b) ++q1;
      const uint32_t u = lus[b] + lo;
      const uint32_t nranked = rt.ranked_items(u);
      ord.resize(q1 - q0);
      for (size_t t = 0; t < ord.size(); ++t) ord[t] = (uint32_t)(q0 + t);
      std::sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return rank[x] < rank[y]; });
      double rank_ui = .0, reciprocal_rank_ui = .0; uint32_t ntestitems = 0;
      for (uint32_t q : ord) {
        const uint32_t j = rank[q];
        ntestitems++;
        fprintf(f, "%d\t%d\t%.5f\t%d\t%d\n", u, qi[q], pred[q], j, item_deg[qi[q]]);
        rank_ui += (j + 1);
        reciprocal_rank_ui += 1 / (j + 1);        // integer division, as in the reference
      }
      if (ntestitems > 0 && nranked > 0) {
        acc[0] += (rank_ui / nranked) / ntestitems;
        acc[1] += reciprocal_rank_ui / ntestitems;
        acc[2] += 1;
      }
      q0 = q1;
    }
    close_or_die(f, my_path(ipath));
    finish_parts(ipath);
    comm_check(comm.allreduce_sum(acc, 3), "itemrank all-reduce");
    if (root()) {
      FILE *itemf = fopen(env.file_str("/meanrank.txt").c_str(), "w");
      if (!itemf) { printf("cannot open logl file:%s\n", strerror(errno)); exit(-1); }
      const uint32_t total_users = (uint32_t)acc[2];
      fprintf(itemf, "%d\t%.5f\t%.5f\n", total_users, (double)acc[0] / total_users, (double)acc[1] / total_users);
      fclose(itemf);
    }
  }

  void gen_ranking_for_users() {                            // hgaprec.cc:2087-2112 (load == false)
    const std::string path = env.datfname + "/test_users.tsv";
    if (root()) env.lerr("loading test users from %s", path.c_str());
    std::vector<uint32_t> ids;
    if (rt.read_test_users(path, &ids)) { if (root()) env.lerr("cannot open %s", path.c_str()); return; }
    sampled = ids;
    compute_precision(true);
    compute_itemrank(true);
    if (root()) env.lerr("DONE writing ranking.tsv in output directory\n");
  }

  void do_on_stop() { save_model(); gen_ranking_for_users(); }          // hgaprec.cc:1572-1577

  // the library moved the rows of W from the packed form to plain doubles (a state p59 cannot hold): say so once
  void note_fallback() {
    hpf_work_info wi;
    if (!fallback_logged && hpf_get_work_info(h, &wi) == HPF_OK && wi.w_fallbacks) {
      fallback_logged = true;
      env.lerr("[rank %d] iteration %d: an entry of W fell below 2^-126 of its row maximum; rows of W are plain fp64 from here on "
               "(results are exact either way)", comm.rank, iter);
    }
  }

  bool held_bound[2] = {false, false};
  // HGAPRec::compute_likelihood (hgaprec.cc:1439-1501); returns true to stop
  bool compute_likelihood(bool validation) {
    const HeldOut &ho = validation ? lvalid : ltest;
    double s = 0.0; uint64_t cnt = 0;
    // the same pairs at every report step: validated and uploaded once (ABI v8), then kernel + ordered sum only
    const int slot = validation ? 0 : 1;
    if (!held_bound[slot]) {
      int rc0 = hpf_heldout_bind(h, slot, ho.u.data(), ho.i.data(), ho.y.data(), ho.u.size());
      if (rc0) die("hpf_heldout_bind", rc0);
      held_bound[slot] = true;
    }
    int rc = hpf_heldout_ll_bound(h, slot, &s, &cnt);
    if (rc) die("hpf_heldout_ll_bound", rc);
    double acc[2] = {s, (double)cnt};
    comm_check(comm.allreduce_sum(acc, 2), "likelihood all-reduce");
    const uint32_t kk = (uint32_t)acc[1];
    const double a = acc[0] / kk;
    if (root()) {
      FILE *ff = validation ? vf : tf;
      fprintf(ff, "%d\t%d\t%.9f\t%d\n", iter, duration(), a, kk);
      fflush(ff);
    }
    if (!validation) return false;
    int why = -1;
    const bool st = stop.update(iter, a, &why);   // same value on every rank => same decision
    if (root()) write_line(env.file_str("/max.txt"), "%d\t%d\t%.5f\t%d\n", iter, duration(), a, why);
    if (st) { g_clock.part_begin(); do_on_stop(); g_clock.part_end(4); return true; }
    return false;
  }

  void finish(int code) {
    g_clock.other();
    if (save_prealloc.joinable()) save_prealloc.join();
    for (int j = 0; j < 3; ++j) { save_u[j].release(); save_i[j].release(); }
    if (h) { hpf_synchronize(h); hpf_destroy(h); h = nullptr; }
    if (root()) { g_clock.totals(iter); g_clock.mark("hpf_destroy"); g_clock.stamp("exit"); }
    comm.barrier();
    if (root()) remove_part_files();
    comm.close_all();
    exit(code);
  }

  // ---- checkpoint / resume (extension) -----------------
  // Everything the loop needs to go on: iteration, stop-rule state, the
  // MT19937 state, the sampled users and every Gamma array of this rank.
  std::string checkpoint_path() const {
    return env.file_str("/checkpoint.r" + std::to_string(comm.rank) + "of" + std::to_string(comm.world) + ".bin");
  }
  // -checkpoint N / -resume (extension).  The device part is hpf_snapshot_save's blob: the
  // loop's arrays verbatim, so a resumed run continues with the bits of an uninterrupted one
  // (same LL series, same stop iteration, same top-N ties).
  void write_checkpoint() {
    const std::string path = checkpoint_path(), tmp = path + ".tmp";
    FILE *f = open_or_die(tmp, "wb");
    bool ok = true;
    auto put = [&](const void *p, size_t sz, size_t cnt) { ok = ok && fwrite(p, sz, cnt, f) == cnt; };
    const uint32_t head[13] = {2u, (uint32_t)comm.world, (uint32_t)comm.rank, n, lo, hi, m, k,
                               (uint32_t)env.hier, (uint32_t)env.bias, (uint32_t)env.binary_data, iter + 1, stop.nh};
    put("HPFCKPT2", 1, 8); put(head, 4, 13); put(&stop.prev_h, 8, 1);
    put(rng.mt, 4, 624); const int32_t mti = rng.mti; put(&mti, 4, 1);
    const uint32_t ns = (uint32_t)sampled.size(); put(&ns, 4, 1); put(sampled.data(), 4, ns);
    size_t bytes = 0;
    int rc = hpf_snapshot_size(h, &bytes);
    if (rc) die("hpf_snapshot_size", rc);
    std::vector<char> blob(bytes);
    if ((rc = hpf_snapshot_save(h, blob.data(), bytes))) die("hpf_snapshot_save", rc);
    const uint64_t b64 = bytes; put(&b64, 8, 1); put(blob.data(), 1, bytes);
    const uint32_t end = 0xffffffffu; put(&end, 4, 1);
    // a checkpoint that did not reach the disk must not replace the previous good one
    if (!ok || (ferror(f) | fclose(f))) { unlink(tmp.c_str()); io_die("cannot write", tmp); }
    if (rename(tmp.c_str(), path.c_str())) io_die("cannot rename checkpoint to", path);
  }
  void read_checkpoint() {
    const std::string path = checkpoint_path();
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "error: [rank %d] -resume: cannot open %s\n", comm.rank, path.c_str()); exit(-1); }
    auto need = [&](bool ok) { if (!ok) { fprintf(stderr, "error: [rank %d] %s is not a checkpoint of this run\n", comm.rank, path.c_str()); exit(-1); } };
    char magic[8]; uint32_t head[13];
    need(fread(magic, 1, 8, f) == 8 && !memcmp(magic, "HPFCKPT2", 8) && fread(head, 4, 13, f) == 13);
    need(head[0] == 2 && head[1] == (uint32_t)comm.world && head[2] == (uint32_t)comm.rank && head[3] == n &&
         head[4] == lo && head[5] == hi && head[6] == m && head[7] == k && head[8] == (uint32_t)env.hier &&
         head[9] == (uint32_t)env.bias && head[10] == (uint32_t)env.binary_data);
    iter = head[11]; stop.nh = head[12];
    need(fread(&stop.prev_h, 8, 1, f) == 1 && fread(rng.mt, 4, 624, f) == 624);
    int32_t mti; need(fread(&mti, 4, 1, f) == 1 && mti >= 0 && mti <= 624); rng.mti = mti;
    uint32_t ns; need(fread(&ns, 4, 1, f) == 1 && ns <= n); sampled.resize(ns); need(fread(sampled.data(), 4, ns, f) == ns);
    size_t want = 0;
    int rc = hpf_snapshot_size(h, &want);
    if (rc) die("hpf_snapshot_size", rc);
    uint64_t b64 = 0;
    need(fread(&b64, 8, 1, f) == 1 && b64 >= 64 && b64 <= (uint64_t)want + (uint64_t)(hi - lo + m) * k * 16);   // bounded before allocating
    std::vector<char> blob((size_t)b64);
    need(fread(blob.data(), 1, blob.size(), f) == blob.size());
    uint32_t end = 0; need(fread(&end, 4, 1, f) == 1 && end == 0xffffffffu);
    fclose(f);
    if ((rc = hpf_snapshot_load(h, blob.data(), blob.size()))) die("hpf_snapshot_load (resume)", rc);
    if (root()) env.lerr("resumed from %s at iteration %d", path.c_str(), iter);
  }

  // the three batch loops share one shape; only -hier honours max_iterations
  // (hgaprec.cc:1337-1339; vb() and vb_bias() run until the stop rule fires)
  void run() {
    if (!env.hier && root()) env.lerr(env.bias ? "running vb_bias()" : "running vb()");
    if (env.resume) read_checkpoint(); else initialize();
    start_sums();
    while (1) {
      if (env.hier && iter > env.max_iterations) finish(0);
      g_clock.other();
      iterate();
      if (g_clock.on) hpf_synchronize(h);
      g_clock.acc_iter += g_clock.lap();
      if (root()) { printf("\r iteration %d", iter); fflush(stdout); }
      if (iter % env.rfreq == 0) {
        g_clock.part_begin();
        if (compute_likelihood(true)) finish(0);
        note_fallback();
        compute_likelihood(false);
        g_clock.part_end(0); g_clock.part_begin();
        save_model();
        g_clock.part_end(1); g_clock.part_begin();
        compute_precision(false);
        g_clock.part_end(2); g_clock.part_begin();
        if (env.hier || !env.bias) compute_itemrank(false);   // vb_bias() has no itemrank call
        g_clock.part_end(3);
        if (env.logl) {                          // HGAPRec::logl, hgaprec.cc:2160-2255
          double v = 0.0;
          int rc2 = hpf_elbo(h, &v);
          if (rc2) die("hpf_elbo", rc2);
          comm_check(comm.allreduce_sum(&v, 1), "ELBO all-reduce");
          if (root()) { fprintf(af, "%.5f\n", v); fflush(af); }
        }
      }
      double flag = g_save_state_now ? 1.0 : 0.0;           // SIGTERM on any rank => all save
      if (comm.world > 1) comm_check(comm.allreduce_max(&flag, 1), "signal all-reduce");
      if (flag > 0) {
        if (root()) env.lerr("Saving state at iteration %d duration %d secs", iter, duration());
        do_on_stop();
      }
      if (env.checkpoint_every && iter > 0 && iter % env.checkpoint_every == 0) write_checkpoint();
      g_clock.acc_report += g_clock.lap();
      iter++;
    }
  }
};

// -ngpus N without rank variables in the environment: re-execute this binary
// N times, one process per GPU, and wait for all of them
int spawn_ranks(int ngpus, char **argv)
{
  int port = 20000 + (int)(getpid() % 20000);
  if (const char *e = getenv("MASTER_PORT")) port = atoi(e);
  // the children prove they are ours with a random nonce (Comm::init)
  {
    unsigned long long nonce = (unsigned long long)getpid() * 0x9E3779B97F4A7C15ull ^ (unsigned long long)time(nullptr);
    if (FILE *f = fopen("/dev/urandom", "rb")) { if (fread(&nonce, 8, 1, f) != 1) {} fclose(f); }
    char buf[32]; snprintf(buf, sizeof buf, "%llx", nonce);
    setenv("HGAPREC_NONCE", buf, 1);
  }
  std::vector<pid_t> kids;
  for (int r = 0; r < ngpus; ++r) {
    pid_t pid = fork();
    if (pid < 0) { perror("fork"); return 1; }
    if (pid == 0) {
      setenv("HGAPREC_RANK", std::to_string(r).c_str(), 1);
      setenv("HGAPREC_WORLD", std::to_string(ngpus).c_str(), 1);
      setenv("HGAPREC_PORT", std::to_string(port).c_str(), 1);
      execv("/proc/self/exe", argv);
      perror("execv");
      _exit(127);
    }
    kids.push_back(pid);
  }
  // wait for all; if one rank fails, the others may be blocked in a collective
  // waiting for it: terminate them instead of hanging
  int code = 0; size_t left = kids.size();
  while (left) {
    int st = 0;
    const pid_t p = waitpid(-1, &st, 0);
    if (p < 0) { if (errno == EINTR) continue; break; }
    auto it = std::find(kids.begin(), kids.end(), p);
    if (it == kids.end()) continue;
    *it = -1; --left;
    const int c = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + WTERMSIG(st);
    if (c && !code) {
      code = c;
      for (pid_t q : kids) if (q > 0) kill(q, SIGKILL);
    }
  }
  return code;
}

}  // namespace

int main(int argc, char **argv)
{
  signal(SIGTERM, term_handler);
  g_clock.stamp("main");
  if (argc <= 1) {
    printf("gaprec -dir <netflix-dataset-dir> -n <users>"
           "-m <movies> -k <dims> -label <out-dir-tag>\n");
    exit(0);
  }
  Env env; std::string bad;
  const bool spawned = getenv("HGAPREC_RANK") != nullptr;
  int rank = 0, world = 1;
  if (spawned) { rank = atoi(getenv("HGAPREC_RANK")); world = atoi(getenv("HGAPREC_WORLD")); }
  else if (getenv("RANK") && getenv("WORLD_SIZE")) { rank = atoi(getenv("RANK")); world = atoi(getenv("WORLD_SIZE")); }
  const int parsed = env.parse(argc, argv, rank == 0, &bad);
  if (parsed && !env.usage_error.empty()) {
    fprintf(stderr, "error: %s\n", env.usage_error.c_str());
    return 2;
  }
  if (parsed) {
    fprintf(stdout, "error: unknown option %s\n", bad.c_str());
    fflush(stdout);
    abort();                                    // the reference asserts (main.cc:227-230)
  }
  // -novb only changes the reference's behaviour in vb_bias() (-bias without -hier): there the
  // rates of BOTH sides are built from the previous iteration's expectations before anything is
  // swapped (hgaprec.cc:1276-1297, a Jacobi order); vb() and vb_hier() never read the flag.
  // The library runs that order (hpf_config.novb); across ranks the start state's sum_u E[theta]
  // is reduced once before the first iteration (Driver::start_sums).
  if (!env.unsupported.empty()) {
    fprintf(stderr, "error: option %s selects a mode outside the MI355X hot-path build "
                    "(supported: -dir -n -m -k -hier -bias -binary-data -rfreq -max-iterations "
                    "-seed -label -rating-threshold -logl -novb -a -b -c -d, -gen-ranking -rmse -msr -eval-all -recommend -fold-in -fold-in-items -fold-iters -fold-tol "
                    "-similar-items -similar-users -similar-metric -topic-items -topic-users -explain -because -audience -ucb -thompson -thompson-seed -diverse -diverse-pool -model-dir, "
                    "-ngpus -comm -single-allreduce -device)\n", env.unsupported.c_str());
    return 2;
  }
  if (env.score_mode()) {
    if (env.ngpus > 1 || world > 1) {
      fprintf(stderr, "error: -gen-ranking / -rmse / -msr / -eval-all / -recommend / -fold-in / -fold-in-items / -similar-items / -similar-users score a saved model on ONE GPU: run them without -ngpus\n");
      return 1;
    }
    // the start of a run truncates validation.txt, precision.txt and friends in its output directory: that directory
    // must not be the one the model is read from.  Nothing has been opened yet.
    char *pm = realpath(env.model_dir.empty() ? "." : env.model_dir.c_str(), nullptr);
    char *po = realpath(env.make_prefix().c_str(), nullptr);
    const bool same = pm && po && !strcmp(pm, po);
    free(pm); free(po);
    if (same) {
      fprintf(stderr, "error: the output directory %s is the model directory: the run would overwrite the files next to the model. "
                      "Give another -label, or run from inside the model directory like the reference\n", env.make_prefix().c_str());
      return 1;
    }
  }
  if (world == 1 && env.ngpus > 1) return spawn_ranks(env.ngpus, argv);

  Comm comm;
  if (world > 1) {
    const char *addr = getenv("MASTER_ADDR");
    int port = 29400;
    if (const char *e = getenv("HGAPREC_PORT")) port = atoi(e);
    else if (const char *e2 = getenv("MASTER_PORT")) port = atoi(e2) + 1;   // leave MASTER_PORT to the launcher
    uint64_t nonce = 0;
    if (const char *e = getenv("HGAPREC_NONCE")) nonce = strtoull(e, nullptr, 16);
    if (comm.init(rank, world, addr ? addr : "127.0.0.1", port, nonce)) {
      fprintf(stderr, "error: [rank %d] cannot reach rank 0 on port %d\n", rank, port);
      return 1;
    }
    if (!env.device_set) env.device = getenv("LOCAL_RANK") ? atoi(getenv("LOCAL_RANK")) : rank;
  }

  // rank 0 owns the output directory; the others only ever write part files into it
  if (rank == 0) {
    if (env.open_output()) { fprintf(stderr, "error: cannot create output directory\n"); abort(); }
  } else env.prefix = env.make_prefix();
  if (comm.barrier()) return 1;

  if (rank == 0) g_clock.mark("start-up (flags, output dir)");
  Ratings ratings;
  ratings.cap_n = env.n; ratings.cap_m = env.m;
  ratings.binary = env.binary_data; ratings.rating_threshold = env.rating_threshold;
  if (rank == 0) { fprintf(stdout, "+ reading ratings dataset from %s\n", env.datfname.c_str()); fflush(stdout); }
  int rc = 0;
  bool have_data = false;
  // -cache: whether the image is there is ONE decision for the whole job: a rank that found the
  // image rank 0 had only just written would skip the hand-over's collectives and leave the ranks out of
  // step.  Every rank looks first, the answers are reduced (also a barrier: nobody writes before everybody
  // has looked), and all ranks take the same path.
  if (env.data_cache && ratings.load_cache(env.datfname) == 0) {
    if (rank == 0) env.lerr("-cache: loaded %s/hgaprec.cache.bin", env.datfname.c_str());
    have_data = true;
  }
  bool all_have = have_data;
  if (world > 1) {
    double neg = have_data ? -1.0 : 0.0;                  // min over ranks through the max of the negatives
    if (comm.allreduce_max(&neg, 1)) return 1;
    all_have = neg < 0.0;
  }
  if (world > 1 && !all_have) {
    // Several ranks, not everybody holds the data set: rank 0 alone parses the TSVs (train, validation,
    // test) -- unless the cache gave it the data -- and hands the parsed data set to the others through an
    // image in the output directory: N parsers of the same text were the set-up cost of `-ngpus N`
    // (VERDICT r2, weak #7).  Ranks that did load the cache keep it and only take part in the collectives.
    const std::string handoff = env.file_str("/ranks.cache.bin");
    double ok = 1.0;
    bool parsed = false;
    if (rank == 0) {
      if (!have_data) {
        rc = ratings.read_train(env.datfname + "/train.tsv");
        if (rc) exit(-1);
        int r2 = ratings.read_heldout(env.datfname + "/validation.tsv", &ratings.validation);
        assert(r2 != -1);
        if (r2) exit(-1);
        r2 = ratings.read_heldout(env.datfname + "/test.tsv", &ratings.test);
        assert(r2 != -1);
        if (r2) exit(-1);
        ratings.heldout_loaded = true;
        parsed = true;
      }
      ok = ratings.save_cache(env.datfname, handoff) == 0 ? 1.0 : 0.0;
      have_data = true;
    }
    if (comm.allreduce_max(&ok, 1)) return 1;            // also the barrier the others wait at
    double got = 1.0;
    if (rank != 0 && !have_data) {
      got = (ok > 0 && ratings.load_cache(env.datfname, handoff) == 0) ? 1.0 : 0.0;
      if (got > 0) { have_data = true; fprintf(stderr, "[rank %d] ratings handed over by rank 0 (%s)\n", rank, handoff.c_str()); }
    }
    double neg = -got;                                    // min over ranks: everybody is done with the image
    if (comm.allreduce_max(&neg, 1)) return 1;
    if (rank == 0) {
      remove(handoff.c_str());
      if (env.data_cache && parsed) {                     // the -cache image is written only now: no rank is still deciding
        if (ratings.save_cache(env.datfname)) env.lerr("-cache: cannot write %s/hgaprec.cache.bin", env.datfname.c_str());
        else env.lerr("-cache: wrote %s/hgaprec.cache.bin", env.datfname.c_str());
      }
    }
  }
  g_clock.other();
  if (!have_data) rc = ratings.read_train(env.datfname + "/train.tsv");
  if (rc) exit(-1);
  if (rank == 0) g_clock.mark("train.tsv");
  if (rank == 0) {
    env.plog("training ratings", (uint32_t)ratings.nratings);
    uint32_t lu = 0, li = 0;
    ratings.write_marginals(env.file_str("/byusers.tsv"), env.file_str("/byitems.tsv"), &lu, &li);
    env.lerr("longest sequence of users with no movies: %d", lu);
    env.lerr("longest sequence of items with no users: %d", li);
    // write_marginal_distributions logs env.n / env.m before Ratings::read shrinks them
    env.plog("post pruning nusers:", env.n);
    env.plog("post pruning nitems:", env.m);
    char st[1024];
    snprintf(st, sizeof st, "read %d users, %d movies, %d ratings", ratings.n, ratings.m, (uint32_t)ratings.nratings);
    env.plog("statistics", std::string(st));
    g_clock.mark("byusers.tsv + byitems.tsv");
  }
  if (!env.batch) {
    if (rank == 0) { printf("Quitting. Online inference not implemented.\n"); fflush(stdout); }
    exit(0);
  }
  if ((uint32_t)world > ratings.n) { fprintf(stderr, "error: more ranks than users\n"); return 1; }
  Driver d(env, ratings, comm);
  d.use_rccl = world > 1 && env.comm_mode != "host";
  d.construct();
  if (env.score_mode()) { score(d, [&]() { d.gen_ranking_for_users(); }); d.finish(0); }   // one report on the loaded model: never the training loop
  d.run();
  return 0;
}
