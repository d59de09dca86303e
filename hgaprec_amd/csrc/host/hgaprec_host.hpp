// hgaprec_host.hpp -- host side of the reference interface (no HIP here).
//
// Mirrors, for the hot path only, what the reference keeps on the host:
//   Env        CLI flags, output-directory name, param.txt   (src/main.cc:99-243, src/env.hh:216-408)
//   Ratings    train/validation/test.tsv -> CSR + held-out lists (src/ratings.cc:63-119,217-271)
//   Mt19937    the gsl_rng_default stream                    (hgaprec.cc:34-38)
//   GammaInit  HGAPRec::initialize draw order                (hgaprec.cc:153-204, gpbase.hh:292-340,939-949)
//   save_*     factor TSV writers                            (matrix.hh:725-744,1140-1166)
//   reports    the loops the CLI's reports on a saved model share (chunk walk, mask lists, list writer)
// The device side is reached only through include/hpf.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <memory>
#include <utility>
#include <vector>

namespace hgaprec {

// ---------------------------------------------------------------- Env -----
struct Env {
  // values as main.cc:41-97 initialises them
  std::string datfname, label;
  uint32_t n = 0, m = 0, k = 0;
  uint32_t rfreq = 10, max_iterations = 1000, rating_threshold = 1;
  double seed = 0, a = 0.3, b = 0.3, c = 0.3, d = 0.3;
  bool logl = false, batch = true, binary_data = false, bias = false, hier = false, vb = true;
  // flags that are parsed (they are part of the CLI) but select code that is
  // outside the hot path; `unsupported` names the first one seen
  std::string unsupported;
  // not part of the reference CLI: device ordinal for the HIP side, number of
  // GPUs (one process each) and how the per-iteration all-reduce is carried
  int device = 0; bool device_set = false;
  bool no_tiles = false;                // -no-tiles: never tile the phi passes (hpf_config.tiling = 1)
  bool w48 = false;                     // -w48: OPT-IN, lossy -- W kept as the top 48 bits of its fp64 value (hpf_config.w_storage = 2): both phi passes ~17 % faster at
                                        // K = 100; arithmetic and every exported number stay fp64.  Never the default: measured drift vs the exact path 1e-6 after 150 sweeps
                                        // (contract 1e-4); tests/test_gpu_cli.py runs C1 to its stop rule both ways
  bool plain_rows = false;              // -plain-rows: W as plain doubles from the start (hpf_config.w_storage = 3; a packed handle moves there by itself when a state does not fit)
  int ngpus = 1;
  std::string comm_mode = "rccl";      // "rccl" | "host" (host-staged, for tests)
  bool single_allreduce = false;        // -single-allreduce: ONE all-reduce of [m x ld | ld] per iteration after the user half, as
                                        // BASELINE.json words it, instead of the overlapped pair (item sums underneath the user half + tail)
  // extension (the reference has no training resume: its -load is inert,
  // main.cc:137-140): -checkpoint N writes <outdir>/checkpoint.r<rank>of<world>.bin
  // every N iterations, -resume continues from it
  uint32_t checkpoint_every = 0; bool resume = false;
  // extension (the reference reads TSV only): -cache keeps a
  // binary image of the parsed dataset (CSR + id maps + held-out sets) in
  // <dir>/hgaprec.cache.bin and loads it instead of the three TSVs while their
  // sizes / mtimes and -n -m -binary-data -rating-threshold are unchanged
  bool data_cache = false;
  // score a saved model instead of training one (main.cc:233-257; hgaprec.cc:2087-2112, 1579-1604, 1993-2085): read the
  // data, load the factor files the writers left, run ONE report, exit.  -model-dir DIR (extension): where those files
  // are; default the current directory, like the reference (name() + ".tsv")
  bool gen_ranking = false, rmse = false, msr = false;
  std::string model_dir;
  // extension: -eval-all ranks EVERY hit test item of EVERY user of a saved model (compute_itemrank judges a sample of at
  // most 1000 users) and writes itemrank_all.tsv, eval_users.tsv and eval_all.txt; a score mode like the three above
  bool eval_all = false;
  // extension: -recommend N writes the N best items of EVERY user of a saved model (recommend.tsv: the first three columns
  // of ranking.tsv, which lists a sample of at most 1000 users; recommend.txt) through hpf_recommend; a score mode too.
  // N outside 1 .. 1024 or no N: parse() returns 2 and says why in usage_error
  uint32_t recommend = 0;
  // extension: -fold-in FILE [-fold-iters T] [-fold-tol X] folds the users of FILE -- who need not be in -dir -- into a
  // saved model through hpf_fold_in (HGAPRec::test(), hgaprec.cc:2257-2346: T = 10 iterations from the prior against the
  // frozen item side; X > 0 stops a user once its E[theta] moves by no more than X of its largest entry) and writes the
  // user-side files of save_model under the prefix foldin_, foldin.txt and, with -recommend N, foldin_recommend.tsv / .txt.
  // A score mode too.  No FILE, T outside 1 .. 10^6 or X outside 0 .. 1: parse() returns 2 and says why in usage_error
  std::string fold_in;
  // extension: -fold-in-items FILE [-fold-iters T] [-fold-tol X] is the mirror for a catalogue that grows: the ITEMS of FILE --
  // which need not be in -dir -- rated by users of -dir, folded in through hpf_fold_in_items against the frozen user side;
  // writes the item-side files of save_model under the prefix foldin_ and foldin_items.txt.  A score mode that runs alone:
  // with -fold-in or any other score mode parse() returns 2 and says why in usage_error
  std::string fold_in_items;
  uint32_t fold_iters = 10;
  double fold_tol = 0.0;
  // extension: -similar-items N / -similar-users N [-similar-metric cosine|dot] write the N nearest other items of every
  // item (users of every user) of a saved model in factor space through hpf_similar: similar_items.tsv / .txt,
  // similar_users.tsv / .txt.  Score modes too; both may be given in one run.  N outside 1 .. 256, no N or another metric:
  // parse() returns 2 and says why in usage_error
  uint32_t similar_items = 0, similar_users = 0;
  std::string similar_metric = "cosine";
  // extension: -topic-items N / -topic-users N write the N heaviest items (users) of every factor of a saved model through
  // hpf_factor_top: topic_items.tsv / .txt, topic_users.tsv / .txt.  Score modes too; both may be given in one run.
  // -explain T goes with -recommend N (also behind -fold-in) or with -audience N: the T largest terms of every listed
  // pair's score through hpf_explain, recommend_explain.tsv / .txt beside recommend.tsv.  N outside 1 .. 1024, T outside
  // 1 .. 32, no number, or -explain without -recommend and without -audience: parse() returns 2 and says why in usage_error
  uint32_t topic_items = 0, topic_users = 0, explain = 0;
  // extension: -because T goes with -recommend N only (also behind -fold-in, also beside -explain): the T items of the
  // user's own ratings that contribute most to every recommended item's score through hpf_because,
  // recommend_because.tsv / .txt beside recommend.tsv.  T outside 1 .. 32, no number, or -because without -recommend:
  // parse() returns 2 and says why in usage_error
  uint32_t because = 0;
  // extension: -audience N writes the N best users of EVERY item of a saved model (audience.tsv: item id, user id, score;
  // audience.txt) through hpf_audience: -recommend transposed, the item's training users with a rating > 0 and its
  // validation users zeroed.  A score mode that runs alone or behind -fold-in-items FILE (foldin_audience.tsv / .txt: the
  // audience of the new items); -explain T may go with it (audience_explain.tsv / .txt); -because is not offered: tracing
  // an audience to histories is another question.  N outside 1 .. 256, no N, or -audience with -fold-in or another score
  // mode: parse() returns 2 and says why in usage_error
  uint32_t audience = 0;
  // extension: -ucb Z goes with -recommend N, N <= 256 (also behind -fold-in): beside recommend.tsv, which is written byte
  // for byte as without the flag, the N best items of every user by the optimistic score mean + Z sd of the Gamma
  // posterior through hpf_recommend_ucb -- recommend_ucb.tsv (user id, item id, ucb, mean, sd) / .txt (users, lines, N, Z).
  // The run reads the shape files of both sides (with -bias of the biases) from -model-dir.  Z negative or no number,
  // -ucb without -recommend, with N > 256 or with -audience: parse() returns 2 and says why in usage_error
  bool ucb_set = false;
  double ucb = 0.0;
  // extension: -thompson D (D = 1 .. 64 draws) goes with -recommend N, N <= 256 (also behind -fold-in); -thompson-seed S (a
  // uint64, 0 unless given) goes with it.  Beside recommend.tsv, which is written byte for byte as without the flag, the N
  // best items of every user in D draws of the model from its Gamma posterior through hpf_recommend_thompson(seed = S,
  // draw = t), t < D -- recommend_thompson.tsv (user id, item id, draw, score) / .txt (users, lines, N, D, S).  The run reads
  // the shape files as -ucb does.  D outside 1 .. 64 or no number, S no uint64, -thompson-seed without -thompson, -thompson
  // without -recommend, with N > 256 or with -audience: parse() returns 2 and says why in usage_error
  uint32_t thompson = 0;
  bool thompson_seed_set = false;
  uint64_t thompson_seed = 0;
  // extension: -diverse L (L in [0, 1]) goes with -recommend N, N <= 256 (also behind -fold-in); -diverse-pool P (N <= P <=
  // 256, min(256, 4 N) unless given) goes with it.  Beside recommend.tsv, which is written byte for byte as without the flag,
  // every user's list re-ranked by greedy MMR from a pool of P candidates through hpf_recommend_diverse(topn = N, pool = P,
  // lambda = L) -- recommend_diverse.tsv (user id, item id, score, maxsim) / .txt (users, lines, N, P, L, mean maxsim).
  // L no number or outside [0, 1], P outside N .. 256, -diverse-pool without -diverse, -diverse without -recommend, with
  // N > 256, with -audience or with -ngpus: parse() returns 2 and says why in usage_error.  After parse() diverse_pool is
  // the pool of the run
  bool diverse_set = false;
  double diverse = 0.0;
  uint32_t diverse_pool = 0;
  std::string usage_error;
  bool score_mode() const {
    return gen_ranking || rmse || msr || eval_all || recommend > 0 || !fold_in.empty() || !fold_in_items.empty() || similar_items > 0 || similar_users > 0 ||
           topic_items > 0 || topic_users > 0 || audience > 0;
  }

  std::string prefix;          // output directory (Env::prefix)
  FILE *plogf = nullptr;       // param.txt
  FILE *logf = nullptr;        // infer.log

  // main.cc:99-232.  Returns 0, or 1 for "unknown option" (the reference
  // asserts there); echo = print the "+ n = ..." lines like the reference.
  int parse(int argc, char **argv, bool echo, std::string *bad_option);
  // env.hh:283-369: the directory name
  std::string make_prefix() const;
  // env.hh:371-402: mkdir (log.cc:97-118), infer.log, param.txt head.
  // Returns 0 or -1.
  int open_output();
  void close_output();
  std::string file_str(const std::string &f) const { return prefix + f; }
  void plog(const std::string &key, double v);
  void plog(const std::string &key, bool v);
  void plog(const std::string &key, uint32_t v);
  void plog(const std::string &key, uint64_t v);
  void plog(const std::string &key, const std::string &v);
  void lerr(const char *fmt, ...);      // log.hh:49 (the only live log level)
};

// ------------------------------------------------------------ Ratings -----
struct HeldOut {          // std::map<Rating,int> flattened in key order
  std::vector<uint32_t> u, i;
  std::vector<int32_t> y;
  size_t lower(uint32_t user, uint32_t item) const;   // the first pair that is not before (user, item)
};

struct Ratings {
  uint32_t cap_n = 0, cap_m = 0;      // env.n / env.m at read time
  bool binary = false;
  uint32_t rating_threshold = 1;
  uint32_t n = 0, m = 0;              // registered users / items
  uint64_t nratings = 0;
  std::vector<uint32_t> seq2user, seq2item;
  // CSR in visiting order: users by seq id, items in file order
  std::vector<int64_t> rowptr;
  std::vector<uint32_t> col;
  std::vector<uint8_t> val;           // last-duplicate-wins, uint8 wrap
  HeldOut validation, test;

  // ratings.cc:42-61 + 63-119.  0 / -1 (cannot open) / -2 (the reference's
  // "unexpected lines" exit(-1))
  int read_train(const std::string &path);
  int read_heldout(const std::string &path, HeldOut *out);
  // -fold-in FILE (extension): "user id, item id, rating" lines of users who need not be in this data set, read by the
  // token rules of train.tsv against THIS data set's items.  out: the new users -- n, seq2user in order of first
  // appearance, CSR (every copy of a duplicated pair with the last rating); m and seq2item are this object's.  Lines whose
  // item is unknown are skipped and counted; ratings the train reader drops are dropped; a user none of whose lines is
  // accepted does not exist; an empty file is zero users.  0 / -1 (cannot open) / -2 (malformed)
  int read_fold_in(const std::string &path, Ratings *out, uint64_t *skipped_unknown) const;
  // -fold-in-items FILE (extension): the mirror -- lines of ITEMS that need not be in this data set, against THIS data
  // set's users.  out: the new items -- m, seq2item in order of first appearance (the item id taken as given) -- and a CSR
  // over this object's n users whose columns are new-item numbers; n and seq2user are this object's.  Lines whose user is
  // unknown are skipped and counted; the rest as read_fold_in.  0 / -1 / -2
  int read_fold_in_items(const std::string &path, Ratings *out, uint64_t *skipped_unknown) const;
  // ratings.cc:273-292: seq ids (sorted, unique) of the listed users that
  // appear in the training set.  -1 if the file cannot be opened
  int read_test_users(const std::string &path, std::vector<uint32_t> *out) const;
  // ratings.cc:217-271
  int write_marginals(const std::string &byusers, const std::string &byitems,
                      uint32_t *longest_users, uint32_t *longest_items) const;
  // the rating stored for (user u, item) in the training set, 0 if absent; of a duplicated pair the last one
  uint32_t r(uint32_t u, uint32_t item) const;
  // the items the reference counts as "ranked" for user u (r(u, item) == 0): m minus the distinct training items with a
  // rating > 0 (compute_itemrank, hgaprec.cc:1628-1680)
  uint32_t ranked_items(uint32_t u) const;
  const std::vector<uint32_t> &item_degrees() const;   // _movies[item]->size(), counted at the first call

  // binary dataset image (extension): everything read_train + both
  // read_heldout calls produce.  dir = the -dir argument (source TSVs are
  // fingerprinted by size and mtime).  load: 0 = loaded, 1 = absent / stale /
  // other parameters / truncated (parse the TSVs instead).  save: 0 or -1.
  bool heldout_loaded = false;
  // `image`: where the image lives (default <dir>/hgaprec.cache.bin); the fingerprint is always
  // that of the TSV files in `dir`.  `-ngpus N` uses an image in the output directory to hand the
  // parsed data set from rank 0 to the other ranks.
  int save_cache(const std::string &dir, const std::string &image = "") const;
  int load_cache(const std::string &dir, const std::string &image = "");

 // open-addressing id -> seq maps (std::map in the reference; only lookups
  // and insertion order matter)
  struct IdMap {
    // one 8-byte slot per entry (key, seq + 1; 0 = empty): a probe touches one cache line
    std::vector<uint64_t> slots; uint32_t cnt = 0;
    IdMap() { rehash(1024); }
    void rehash(uint32_t cap);
    bool find(uint32_t key, uint32_t *val) const;
    void put(uint32_t key, uint32_t val);
  } user2seq, item2seq;

 private:
  int read_generic(FILE *f, HeldOut *out);
  int read_generic_parallel(FILE *f, HeldOut *out);   // 0 done, 1 not for this file (small, not well-formed, one thread)
  struct Consumer;
  uint32_t input_rating_class(uint32_t v) const;
  void build_csr();                            // tr_u_ / tr_i_ / tr_y_ -> rowptr, col, val (and frees the triples)
  std::vector<uint32_t> tr_u_, tr_i_, tr_y_;   // training triples in file order
  mutable std::vector<uint32_t> item_deg_;
};

// ------------------------------------------------------------ MT19937 -----
// gsl_rng_mt19937: 2002 init_genrand seeding, seed 0 -> 4357,
// gsl_rng_uniform = u32 / 2^32
struct Mt19937 {
  uint32_t mt[624]; int mti;
  explicit Mt19937(unsigned long seed = 0) { set(seed); }
  void set(unsigned long seed);
  uint32_t next_u32();
  void refill();
  // out[j] = base + scale * uniform() for the next cnt draws / cnt draws taken and dropped: the stream
  // position afterwards is that of cnt calls of next_u32()
  void fill_affine(double *out, size_t cnt, double base, double scale);
  void skip(size_t cnt);
  double uniform() { return next_u32() / 4294967296.0; }
  unsigned long uniform_int(unsigned long n);
};

double digamma(double x);      // x > 0, |err| ~ 1e-15 (stands for gsl_sf_psi)

// ---------------------------------------------------------- GammaInit -----
// Host arrays of the start state, in the layout of hpf_set_state.
// resize() of these arrays does not write zeros first: every element is assigned by initialize_state, and at
// C2 the four user-side matrices are 3.5 GB that would otherwise be touched twice
template <typename T> struct NoInitAlloc : std::allocator<T> {
  template <typename U> struct rebind { using other = NoInitAlloc<U>; };
  template <typename U> void construct(U *p) noexcept { ::new ((void *)p) U; }
  template <typename U, typename... A> void construct(U *p, A &&...a) { ::new ((void *)p) U(std::forward<A>(a)...); }
};
using StateArray = std::vector<double, NoInitAlloc<double>>;
struct GammaState {
  uint32_t n = 0, m = 0, k = 0; bool hier = false, bias = false;
  StateArray theta_shape, theta_rate, theta_E, theta_Elog;
  StateArray beta_shape, beta_rate, beta_E, beta_Elog;
  StateArray xi_shape, xi_rate, xi_E, xi_Elog;
  StateArray eta_shape, eta_rate, eta_E, eta_Elog;
  StateArray ubias_shape, ubias_rate, ubias_E, ubias_Elog;
  StateArray ibias_shape, ibias_rate, ibias_E, ibias_Elog;
};
// hgaprec.cc:153-204 with the RNG already seeded as hgaprec.cc:34-38.
// [user_lo, user_hi): keep only that range of the user-side arrays (a rank's
// shard); the whole MT19937 stream is still consumed in the reference's
// order, so every rank ends with the same generator state and the same
// item-side arrays.  out->n is the number of users kept.
void initialize_state(Mt19937 &rng, uint32_t n, uint32_t m, uint32_t k, bool hier,
                      bool bias, GammaState *out, uint32_t user_lo = 0,
                      uint32_t user_hi = 0xffffffffu);
// the seed rule of hgaprec.cc:34-38 (+ GSL_RNG_SEED like gsl_rng_env_setup)
Mt19937 make_rng(double env_seed);

// ------------------------------------------------------------ writers -----
// D2Array<double>::save / D1Array<double>::save: "seq\tid\tv...\n", %.8f;
// id = seq2id[row] when row < nids else the row index itself
// "%.8f" exactly as printf rounds it, ~10x faster; returns the length (no NUL)
size_t format_fixed8(double v, char *out);
// row0: sequence number of the first row (a rank writing its shard of a matrix)
// threads: how many host threads format the rows (0 = all of them)
// a model file is rewritten in place (save_matrix / save_vector, and the part files put together by rank 0): while that
// is going on "<path>.writing" lies beside it; a marker that outlives the run says the file is not whole
std::string rewrite_marker(const std::string &path);
void rewrite_begin(const std::string &path);
void rewrite_end(const std::string &path);
int save_matrix(const std::string &path, const double *a, uint32_t rows, uint32_t cols,
                const uint32_t *seq2id, uint32_t nids, uint32_t row0 = 0, unsigned threads = 0);
int save_vector(const std::string &path, const double *a, uint32_t rows,
                const uint32_t *seq2id, uint32_t nids, uint32_t row0 = 0);

// ------------------------------------------------------------ readers -----
// the inverse of save_matrix / save_vector with the reference's reading rules (matrix.hh:767-803,1198-1266): strtod per
// field, the first two columns (seq, id) skipped as values, rows in line order, lines beyond `rows` ignored.  Stricter
// than the reference (hgaprec_host.cpp): a missing file, fewer rows than `rows`, a row with fewer than `cols` values and
// -- when ids is given -- an id column that differs from ids[row] (row >= nids: the row index) return -1 with
// *err = "<path>: ..." naming the line.  out: rows x cols doubles, row-major.
int load_matrix(const std::string &path, double *out, uint32_t rows, uint32_t cols,
                const uint32_t *ids, uint32_t nids, std::string *err);
// A value field that is negative or not finite (strtod takes "-1", "nan", "inf") is an error of the same kind: the files
// hold Gamma parameters and expectations, and the ranking calls are defined for finite E >= +0.0 only (include/hpf.h).
int load_vector(const std::string &path, double *out, uint32_t rows,
                const uint32_t *ids, uint32_t nids, std::string *err);
// without -hier: E[r][c] = shape[r][c] / rate[c] in place (GPMatrixGR::compute_expectations, gpbase.hh:755-764).  A
// rate that is not finite and > 0, or a quotient that is not finite, returns -1 with *err = "<rate_path>: line c+1: ..."
int shape_over_rate(double *E, uint32_t rows, uint32_t cols, const double *rate, const std::string &rate_path, std::string *err);
// -fold-in: both Gamma expectations of a side read as shape and rate.  E holds the shapes on entry and shape / rate on
// return, Elog = digamma(shape) - log(rate); the rate is one value per element, or per column (a K-vector).  A shape or a
// rate that is not > 0 returns -1 with *err = "<rate_path>: a shape or a rate that is not > 0 (row r)"
int gamma_expectations(double *E, double *Elog, const double *rate, size_t rows, size_t cols, bool rate_per_column,
                       const std::string &rate_path, std::string *err);

// ------------------------------------------- held-out series / stopping ---
// HGAPRec::compute_likelihood bookkeeping (hgaprec.cc:1466-1500)
struct StopRule {
  double prev_h = 0.0; uint32_t nh = 0;
  // returns true when the run must stop; *why as written to max.txt
  bool update(uint32_t iter, double a, int *why);
};

// ------------------------------------------------- metrics from ranks -----
// -eval-all: what the ranks of a user's test items say about the user, and the means over the users.
// Integers per user (eval_users.tsv): hitsN = queries with rank < N, best_rank = the smallest rank, sum_rank = the sum
// of (rank + 1).
struct EvalUser { uint32_t ntest, hits10, hits100, best_rank; uint64_t sum_rank; };
// eval_all.txt: means over the users, each summed serially in the order given
struct EvalMeans { uint64_t users, pairs; double precision10, precision100, recall100, mrr, meanrank; };
// User b's ranks (0-based positions in its full item order) are rank[q_ptr[b] .. q_ptr[b+1]), in any order; every user
// given has at least one.  nranked[b]: the items the reference counts as ranked for the user (n_items minus the
// distinct training items with a rating > 0; compute_itemrank, hgaprec.cc:1628-1680).  Per user:
//   precision@N = hitsN / N, recall@100 = hits100 / ntest,
//   mrr = 1.0 / (best_rank + 1) -- REAL division: the reference's reciprocal_rank_ui divides integers (1 / (j + 1) is 0
//         for every j > 0; Driver::compute_itemrank keeps that for parity), this report is an extension and does not,
//   meanrank = (sum_rank / nranked) / ntest, the first figure of meanrank.txt (0 for a user with nranked = 0, whom
//         compute_itemrank leaves out).
// A user without a query (q_ptr[b] == q_ptr[b+1]) gets zeros and best_rank = 0 and adds 0 to every mean.
void eval_from_ranks(const uint64_t *q_ptr, const uint32_t *rank, const uint32_t *nranked, size_t n_users,
                     EvalUser *per_user, EvalMeans *means);

// ------------------------------------------- the loops of the reports -----
// What the ranking reports of the CLI share.  A report ranks its rows a chunk at a time (host memory is O(chunk), one
// library call per chunk): f(r0, r1) for the rows [r0, r1) of [0, rows), in order.
constexpr size_t REPORT_CHUNK = 1u << 16;
template <class F>
void for_chunks(size_t rows, F &&f, size_t chunk = REPORT_CHUNK)
{
  for (size_t r0 = 0; r0 < rows; r0 += chunk) f(r0, std::min(rows, r0 + chunk));
}
// the offsets ptr[b0 .. b1] of a chunk, counted from the chunk's first entry (b1 - b0 + 1 of them)
void chunk_offsets(const uint64_t *ptr, size_t b0, size_t b1, std::vector<uint64_t> *out);
// The held-out items of a run of users in the form the ranking calls take (mask_ptr, mask_items; is_validation()): of
// list[0 .. cnt) the users inside [lo, hi), in the list's order -- list == nullptr: every user of [lo, hi).  users holds
// them minus `rebase` (a rank's local indices).
struct MaskLists {
  std::vector<uint32_t> users, items;
  std::vector<uint64_t> ptr;
  void fill(const HeldOut &ho, const uint32_t *list, size_t cnt, uint32_t lo, uint32_t hi, uint32_t rebase = 0);
};
// The transpose of MaskLists::fill, for the calls that select ITEMS (hpf_audience): the held-out users of the items
// [lo, hi) as (mask_ptr, mask_users) -- items holds lo .. hi - 1, item b's users are users[ptr[b] .. ptr[b + 1]), ascending
// (the pairs of a HeldOut are in (user, item) order and are visited in that order).  One pass over the pairs per call.
struct ItemMaskLists {
  std::vector<uint32_t> items, users;
  std::vector<uint64_t> ptr;
  void fill(const HeldOut &ho, uint32_t lo, uint32_t hi);
};
// Top-N lists as lines "row id \t entry id \t %.5f" (`digits` decimals: 5 unless given): list b belongs to row sel[b] and has items[b * N + j], scores[b * N + j],
// j < N, of which the first `real` exist (the rest is padding and never printed); ids through row_ids / item_ids.  Only
// the entries keep(sel[b], item) accepts are written (no keep: all).  Returns the number of lines.
uint64_t write_topn(FILE *f, const uint32_t *sel, size_t n_sel, const uint32_t *items, const double *scores, uint32_t N,
                    uint32_t real, const uint32_t *row_ids, const uint32_t *item_ids,
                    const std::function<bool(uint32_t, uint32_t)> &keep = nullptr, int digits = 5);
// The lists of D draws (-thompson) as lines "row id \t entry id \t draw \t %.5f": items / scores hold draw t's lists of the
// n_sel rows at [t * n_sel * N ...), each as for write_topn.  Rows in the order of sel, within a row the draws ascending,
// each list best first, under write_topn's rule (no padding, only what keep accepts).  Returns the number of lines.
uint64_t write_thompson(FILE *f, const uint32_t *sel, size_t n_sel, const uint32_t *items, const double *scores, uint32_t D, uint32_t N,
                        uint32_t real, const uint32_t *row_ids, const uint32_t *item_ids,
                        const std::function<bool(uint32_t, uint32_t)> &keep = nullptr);
// The re-ranked lists (-diverse) as lines "row id \t entry id \t %.5f \t %.5f" (score, maxsim): items / scores / maxsim as
// hpf_recommend_diverse returns them, [n_sel x N].  Rows in the order of sel, each list in pick order up to its first
// padding entry (0xffffffff), only what keep accepts.  Returns the number of lines; maxsim_sum, where given, grows by the
// maxsim of every line written.
uint64_t write_diverse(FILE *f, const uint32_t *sel, size_t n_sel, const uint32_t *items, const double *scores, const double *maxsim,
                       uint32_t N, const uint32_t *row_ids, const uint32_t *item_ids,
                       const std::function<bool(uint32_t, uint32_t)> &keep = nullptr, double *maxsim_sum = nullptr);

// ------------------------------------------------------------- Comm --------
// Host-side collectives of a multi-process run (one process per GPU): a TCP
// star through rank 0 on MASTER_ADDR:MASTER_PORT.  Used for the bootstrap (the
// RCCL unique id), the few scalars per report step, and -- with `-comm host`
// -- a host-staged stand-in for the device all-reduce (tests on one GPU).
// Sums are formed on rank 0 in rank order, so every rank sees the same bits.
struct Comm {
  int rank = 0, world = 1;
  std::vector<int> fds;       // rank 0: one socket per peer (index = peer rank); others: fds[0]
  // nonce: shared secret of the job (0 when the launcher gave none); a peer that does not
  // present it is dropped.  0 / -1
  int init(int rank_, int world_, const std::string &addr, int port, uint64_t nonce = 0);
  void close_all();
  int allreduce_sum(double *v, size_t n);
  int allreduce_max(double *v, size_t n);
  int bcast(void *p, size_t bytes);          // from rank 0
  int barrier();
 private:
  int reduce_impl(double *v, size_t n, bool is_max);
};

// contiguous user ranges balanced on the nnz prefix sum
std::vector<std::pair<uint32_t, uint32_t>> partition_users(const std::vector<int64_t> &rowptr, int world);

}  // namespace hgaprec
