// score_modes.cpp -- the reports of `hgaprec` on a saved model: -rmse / -msr / -eval-all / -recommend [-explain] [-because] [-ucb] [-thompson] [-diverse] /
// -similar-items / -similar-users / -topic-items / -topic-users / -audience [-explain] / -fold-in / -fold-in-items (and -gen-ranking, which is the training run's own ranking on the loaded state).  Each
// reads the data like a training run, loads the factor files a run has written (from the current directory like the
// reference, or from -model-dir DIR), writes ONE report and returns.  One GPU; nothing of the training loop is seen here.
#include "hgaprec_cli.hpp"

#include <cmath>
#include <unistd.h>

namespace hgaprec {
namespace {

struct ScoreModes : Cli {
  const uint32_t n, m, k;
  explicit ScoreModes(const Cli &c) : Cli(c), n(c.rt.n), m(c.rt.m), k(c.env.k) {}

  std::string model_path(const std::string &name) const { return (env.model_dir.empty() ? std::string(".") : env.model_dir) + "/" + name; }
  // a factor file of the model, rows x cols, through the strict reader (hgaprec_host.cpp, load_matrix); returns its path.
  // ids: what its id column must hold -- nullptr for a K-vector, whose id column is seq2id[k] and is not compared
  std::string load(const std::string &name, std::vector<double> &out, uint32_t rows, uint32_t cols, const std::vector<uint32_t> *ids) const {
    const std::string path = model_path(name);
    std::string err;
    out.resize((size_t)rows * cols);
    if (load_matrix(path, out.data(), rows, cols, ids ? ids->data() : nullptr, ids ? (uint32_t)ids->size() : 0, &err)) model_die(err);
    return path;
  }

  // HGAPRec::load_beta_and_theta (hgaprec.cc:2114-2135): the expectations of the factor files into the handle's *_E.
  // -hier: htheta.tsv / hbeta.tsv hold E; without: E = shape / rate[k], as GPMatrixGR::load -> compute_expectations
  // does (gpbase.hh:755-764); -bias: the one value column of thetabias.tsv / betabias.tsv.  thetarate.tsv / betarate.tsv
  // are read when they are there (scoring never touches them).  Stricter than the reference (hgaprec_host.cpp,
  // load_matrix): a missing file, a short file, a short row, or ids that are not those of the ratings just read stop the run.
  void load_model() {
    std::string err;
    auto side = [&](bool user_side) {
      const uint32_t rows = user_side ? n : m;
      const std::vector<uint32_t> &ids = user_side ? rt.seq2user : rt.seq2item;
      const std::string base = env.hier ? (user_side ? "htheta" : "hbeta") : (user_side ? "theta" : "beta");
      std::vector<double> E, v;
      if (env.hier) load(base + ".tsv", E, rows, k, &ids);
      else {
        load(base + "_shape.tsv", E, rows, k, &ids);
        const std::string rate_path = load(base + "_rate.tsv", v, k, 1, nullptr);
        if (shape_over_rate(E.data(), rows, k, v.data(), rate_path, &err)) model_die(err);   // a zero rate would rank the item first
      }
      put(user_side ? HPF_THETA_E : HPF_BETA_E, E);
      if (env.hier && access(model_path(user_side ? "thetarate.tsv" : "betarate.tsv").c_str(), R_OK) == 0) {
        load(user_side ? "thetarate.tsv" : "betarate.tsv", v, rows, 1, &ids);
        put(user_side ? HPF_XI_E : HPF_ETA_E, v);
      }
      if (env.bias) {
        load(user_side ? "thetabias.tsv" : "betabias.tsv", v, rows, 1, &ids);
        put(user_side ? HPF_UBIAS_E : HPF_IBIAS_E, v);
      }
    };
    side(false);
    side(true);
    env.lerr("loaded the model from %s", env.model_dir.empty() ? "." : env.model_dir.c_str());
  }

  // -because T: hpf_because reads Elog beside E, and the E files do not give it.  Both sides' shape and rate files through
  // the strict readers -- htheta / hbeta or theta / beta, with -bias thetabias / betabias --, Elog = psi(shape) - log(rate)
  // (gamma_expectations) into the handle's *_ELOG.  E stays what load_model has put: the lists are those of a run without
  // the flag.  Only a run with the flag reads these files.
  void load_model_elog() {
    std::string err;
    for (int user_side = 0; user_side < 2; ++user_side) {
      const uint32_t rows = user_side ? n : m;
      const std::vector<uint32_t> &ids = user_side ? rt.seq2user : rt.seq2item;
      const std::string base = env.hier ? (user_side ? "htheta" : "hbeta") : (user_side ? "theta" : "beta");
      std::vector<double> E, L((size_t)rows * k), rate;
      load(base + "_shape.tsv", E, rows, k, &ids);
      const std::string rate_path = env.hier ? load(base + "_rate.tsv", rate, rows, k, &ids) : load(base + "_rate.tsv", rate, k, 1, nullptr);
      if (gamma_expectations(E.data(), L.data(), rate.data(), rows, k, !env.hier, rate_path, &err)) model_die(err);
      put(user_side ? HPF_THETA_ELOG : HPF_BETA_ELOG, L);
      if (env.bias) {
        const std::string bias = user_side ? "thetabias" : "betabias";
        L.resize(rows);
        load(bias + "_shape.tsv", E, rows, 1, &ids);
        const std::string bp = load(bias + "_rate.tsv", rate, rows, 1, &ids);
        if (gamma_expectations(E.data(), L.data(), rate.data(), rows, 1, false, bp, &err)) model_die(err);
        put(user_side ? HPF_UBIAS_ELOG : HPF_IBIAS_ELOG, L);
      }
    }
    env.lerr("-because: Elog of both sides formed from the shape and rate files");
  }

  // -ucb Z, -thompson D: hpf_recommend_ucb and hpf_recommend_thompson read the shapes beside E.  The shape files of both sides through the strict readers --
  // htheta / hbeta or theta / beta, with -bias thetabias / betabias -- into the handle's *_SHAPE.  E stays what load_model
  // has put: recommend.tsv is that of a run without the flag.  Only a run with the flag reads these files here.
  // only_items: the handle of a fold-in, whose user side the fold-in has left with its shapes.
  void load_model_shapes(bool only_items) {
    for (int user_side = 0; user_side < (only_items ? 1 : 2); ++user_side) {
      const uint32_t rows = user_side ? n : m;
      const std::vector<uint32_t> &ids = user_side ? rt.seq2user : rt.seq2item;
      const std::string base = env.hier ? (user_side ? "htheta" : "hbeta") : (user_side ? "theta" : "beta");
      std::vector<double> S;
      load(base + "_shape.tsv", S, rows, k, &ids);
      put(user_side ? HPF_THETA_SHAPE : HPF_BETA_SHAPE, S);
      if (env.bias) {
        load(std::string(user_side ? "thetabias" : "betabias") + "_shape.tsv", S, rows, 1, &ids);
        put(user_side ? HPF_UBIAS_SHAPE : HPF_IBIAS_SHAPE, S);
      }
    }
    env.lerr("%s: the shapes of %s from the shape files", env.ucb_set ? "-ucb" : "-thompson", only_items ? "the item side" : "both sides");
  }

  // HGAPRec::compute_rmse (hgaprec.cc:1579-1604).  DEVIATION: the reference's -rmse never loads the model (main.cc:254-257
  // constructs and calls compute_rmse; load_beta_and_theta() is commented out at hgaprec.cc:1587), so it scores the empty
  // start objects.  This build loads the model first.
  void compute_rmse() {
    const HeldOut &ho = rt.test;
    std::vector<double> pred(ho.u.size());
    int rc = hpf_predict(h, ho.u.data(), ho.i.data(), ho.u.size(), pred.data());
    if (rc) die("hpf_predict", rc);
    const std::string spath = env.file_str("/test_scores.tsv");
    FILE *f = open_or_die(spath, "w");
    double s = .0;
    for (size_t p = 0; p < pred.size(); ++p) {                // map order, summed serially
      const uint8_t v = (uint8_t)ho.y[p];                     // yval_t v = i->second
      const double u = pred[p];
      s += (u - v) * (u - v);
      fprintf(f, "%d\t%.5f\n", v, u);
    }
    close_or_die(f, spath);
    write_line(env.file_str("/rmse.txt"), "%.5f\n", sqrt(s / pred.size()));
  }

  // HGAPRec::gen_msr_csv (hgaprec.cc:1993-2085): per user, where the held-out item -- the LAST test pair of the user in
  // (user, item) order, hgaprec.cc:140-145 -- stands among the items [0, m - 1) (the reference's loop never scores item
  // m - 1).  The reference asserts on a user without a test pair; here the run stops before pred.csv exists.
  void gen_msr_csv() {
    std::vector<uint32_t> heldout(n, 0xffffffffu);
    for (size_t p = 0; p < rt.test.u.size(); ++p) heldout[rt.test.u[p]] = rt.test.i[p];     // sorted by (user, item): the last one stays
    for (uint32_t u = 0; u < n; ++u)
      if (heldout[u] == 0xffffffffu) {
        fprintf(stderr, "error: -msr: user %u (seq %u) has no pair in test.tsv\n", rt.seq2user[u], u);
        exit(1);
      }
    const std::vector<uint32_t> &item_deg = rt.item_degrees();
    std::vector<uint32_t> valid_users(m, 0);                 // _validation_users_of_movie
    for (uint32_t it : rt.validation.i) valid_users[it]++;
    std::vector<uint32_t> rank(n), masked(n);                // O(n) results; the scores of a chunk never leave the device
    std::vector<double> sc;
    const uint32_t limit = m - 1;
    MaskLists ml;
    // m == 1: the reference's loop over [0, m - 1) scores nothing and leaves rank 0 (a limit of 0 would mean "all items")
    for_chunks(limit > 0 ? n : 0, [&](size_t u0, size_t u1) {
      ml.fill(rt.validation, nullptr, 0, (uint32_t)u0, (uint32_t)u1);
      sc.resize(ml.users.size());
      int rc = hpf_loo_ranks(h, ml.users.data(), (uint32_t)ml.users.size(), ml.ptr.data(), ml.items.data(), heldout.data() + u0, limit,
                             rank.data() + u0, sc.data(), masked.data() + u0);
      if (rc) die("hpf_loo_ranks", rc);
    });
    const std::string path = env.file_str("/pred.csv");
    FILE *f = open_or_die(path, "w");
    fprintf(f, "User\tHeldOutItem\tHeldOutItemIndex\tUserNegatives\tUserCount\tItemCount\n");
    for (uint32_t u = 0; u < n; ++u) {
      const uint32_t t = heldout[u], training = masked[u], negatives = limit - masked[u];
      fprintf(f, "%d\t%d\t%d\t%d\t%d\t%d\n", rt.seq2user[u], rt.seq2item[t], rank[u], negatives, training,
              valid_users[t] + item_deg[t]);
    }
    close_or_die(f, path);
  }

  // -eval-all (extension): compute_itemrank's question -- where does each test item that is a hit stand in its user's
  // full item order, training items with a rating > 0 and validation items zeroed -- for EVERY user with such an item
  // instead of a sample, through hpf_rank_queries (the user's scores are computed once for all its items, and no score
  // reaches memory).  itemrank_all.tsv has itemrank.tsv's lines; eval_users.tsv the integers per user; eval_all.txt the
  // means (eval_from_ranks, hgaprec_host.hpp).
  void eval_all_report() {
    const std::vector<uint32_t> &item_deg = rt.item_degrees();
    std::vector<uint32_t> eu;                                 // evaluated users, seq order
    std::vector<uint64_t> qptr(1, 0); std::vector<uint32_t> qi;
    for (uint32_t u = 0; u < n; ++u) {
      for (size_t a = rt.test.lower(u, 0); a < rt.test.u.size() && rt.test.u[a] == u; ++a)
        if (test_hit(rt.test.y[a])) qi.push_back(rt.test.i[a]);
      if (qi.size() > qptr.back()) { eu.push_back(u); qptr.push_back(qi.size()); }
    }
    std::vector<uint32_t> rank(qi.size()); std::vector<double> pred(qi.size());
    MaskLists ml; std::vector<uint64_t> cq;
    for_chunks(eu.size(), [&](size_t b0, size_t b1) {
      ml.fill(rt.validation, eu.data() + b0, b1 - b0, 0, n);
      chunk_offsets(qptr.data(), b0, b1, &cq);
      int rc = hpf_rank_queries(h, ml.users.data(), (uint32_t)(b1 - b0), ml.ptr.data(), ml.items.data(), cq.data(),
                                qi.data() + qptr[b0], rank.data() + qptr[b0], pred.data() + qptr[b0]);
      if (rc) die("hpf_rank_queries", rc);
    });
    std::vector<uint32_t> nranked(eu.size());
    for (size_t b = 0; b < eu.size(); ++b) nranked[b] = rt.ranked_items(eu[b]);     // as in compute_itemrank
    std::vector<EvalUser> pu(eu.size()); EvalMeans mean;
    eval_from_ranks(qptr.data(), rank.data(), nranked.data(), eu.size(), pu.data(), &mean);

    const std::string ipath = env.file_str("/itemrank_all.tsv"), upath = env.file_str("/eval_users.tsv");
    FILE *f = open_or_die(ipath, "w"), *uf = open_or_die(upath, "w");
    std::vector<uint64_t> ord;
    for (size_t b = 0; b < eu.size(); ++b) {
      const uint32_t u = eu[b];
      ord.resize(qptr[b + 1] - qptr[b]);
      for (size_t t = 0; t < ord.size(); ++t) ord[t] = qptr[b] + t;
      std::stable_sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) { return rank[x] < rank[y]; });
      for (uint64_t q : ord) fprintf(f, "%d\t%d\t%.5f\t%d\t%d\n", u, qi[q], pred[q], rank[q], item_deg[qi[q]]);
      fprintf(uf, "%u\t%u\t%u\t%u\t%u\t%u\t%llu\n", u, rt.seq2user[u], pu[b].ntest, pu[b].hits10, pu[b].hits100,
              pu[b].best_rank, (unsigned long long)pu[b].sum_rank);
    }
    close_or_die(f, ipath);
    close_or_die(uf, upath);
    write_line(env.file_str("/eval_all.txt"), "%llu\t%llu\t%.5f\t%.5f\t%.5f\t%.5f\t%.5f\n", (unsigned long long)mean.users,
               (unsigned long long)mean.pairs, mean.precision10, mean.precision100, mean.recall100, mean.mrr, mean.meanrank);
    env.lerr("-eval-all: %llu users, %llu test items ranked", (unsigned long long)mean.users, (unsigned long long)mean.pairs);
  }

  // -recommend N (extension): what a recommender is for -- the N best items of EVERY user, training items with a
  // rating > 0 and the user's validation items zeroed exactly as compute_precision zeroes them for its sample -- through
  // hpf_recommend (no score reaches memory up to N = 256).  <stem>.tsv has the first three columns of ranking.tsv under
  // ranking.tsv's rule (given.r(u, it) == 0; the padding beyond m items is never printed), users in seq order; <stem>.txt
  // users, lines and N.  A chunk of users is written before the next is ranked: host memory is O(chunk x N).
  // -fold-in's tail is the same report for the new users: their own handle and ratings, and no list beyond the given
  // ratings, which the call masks itself (mask == nullptr).
  // -explain T (extension): behind each chunk's lists the same walk hands the (user, item) pairs of the lines it has just
  // written -- write_topn's rule, so no padding and no given item -- to hpf_explain and writes <stem>_explain.tsv: user id,
  // item id, factor, contribution (%.8f), pairs in <stem>.tsv's order, each pair's T largest terms best first; with -bias
  // the factors K and K + 1 are the user and the item bias.  <stem>_explain.txt: pairs, lines, T.  <stem>.tsv is written
  // by the same calls as without the flag.
  // -because T (extension): the same pairs, grouped by user as they are, go to hpf_because; <stem>_because.tsv: user id,
  // item id, rated item id, contribution (%.8f), pairs in <stem>.tsv's order, each pair's T rated items best first, the
  // padding of a history shorter than T never printed.  <stem>_because.txt: pairs, lines, T.
  // -ucb Z (extension): behind each chunk's lists the same users and mask lists go to hpf_recommend_ucb; <stem>_ucb.tsv:
  // user id, item id, ucb, mean, sd = sqrt(var) (%.5f each) under <stem>.tsv's rule, users in seq order, each list best
  // first by mean + Z sd.  <stem>_ucb.txt: users, lines, N, Z.  <stem>.tsv is written by the same calls as without the flag.
  // -thompson D (extension): behind each chunk's lists the same users and mask lists go to hpf_recommend_thompson once per
  // draw t < D with seed = -thompson-seed; <stem>_thompson.tsv: user id, item id, draw, score (%.5f) under <stem>.tsv's rule
  // (write_thompson: users in seq order, within a user the draws ascending, each list best first).  <stem>_thompson.txt:
  // users, lines, N, D, seed.
  // -diverse L (extension): behind each chunk's lists the same users and mask lists go to hpf_recommend_diverse(topn = N, pool
  // = -diverse-pool, lambda = L); <stem>_diverse.tsv: user id, item id, score, maxsim (%.5f each; write_diverse: users in seq
  // order, each list in pick order, no padding).  <stem>_diverse.txt: users, lines, N, P, L, the mean maxsim of the lines.
  unsigned long long recommend_lists(const Ratings &given, const HeldOut *mask, const std::string &stem) {
    const uint32_t N = env.recommend, T = env.explain, TB = env.because;
    const std::string rpath = env.file_str(stem + ".tsv"), epath = env.file_str(stem + "_explain.tsv"), bpath = env.file_str(stem + "_because.tsv");
    FILE *f = open_or_die(rpath, "w"), *ef = T ? open_or_die(epath, "w") : nullptr, *bf = TB ? open_or_die(bpath, "w") : nullptr;
    const std::string upath = env.file_str(stem + "_ucb.tsv");
    FILE *uf = env.ucb_set ? open_or_die(upath, "w") : nullptr;
    const uint32_t D = env.thompson;
    const std::string tpath = env.file_str(stem + "_thompson.tsv");
    FILE *tf = D ? open_or_die(tpath, "w") : nullptr;
    std::vector<uint32_t> titems; std::vector<double> tscores;
    unsigned long long tlines = 0;
    const std::string dpath = env.file_str(stem + "_diverse.tsv");
    FILE *df = env.diverse_set ? open_or_die(dpath, "w") : nullptr;
    std::vector<uint32_t> ditems; std::vector<double> dscores, dmaxsim;
    unsigned long long dlines = 0; double dsum = 0.0;
    MaskLists ml; std::vector<uint32_t> items, eu, ei, fac, rated, uitems; std::vector<double> scores, con, ucb, mean, var;
    std::vector<uint64_t> tptr;
    const HeldOut none;
    unsigned long long lines = 0, epairs = 0, elines = 0, bpairs = 0, blines = 0, ulines = 0;
    const std::function<bool(uint32_t, uint32_t)> keep = [&](uint32_t u, uint32_t it) { return given.r(u, it) == 0; };
    for_chunks(given.n, [&](size_t u0, size_t u1) {
      ml.fill(mask ? *mask : none, nullptr, 0, (uint32_t)u0, (uint32_t)u1);
      items.resize(ml.users.size() * (size_t)N); scores.resize(ml.users.size() * (size_t)N);
      int rc = hpf_recommend(h, ml.users.data(), (uint32_t)ml.users.size(), ml.ptr.data(), mask ? ml.items.data() : nullptr, N,
                             items.data(), scores.data());
      if (rc) die("hpf_recommend", rc);
      lines += write_topn(f, ml.users.data(), ml.users.size(), items.data(), scores.data(), N, m, given.seq2user.data(),
                          rt.seq2item.data(), keep);
      if (uf) {
        const size_t cnt = ml.users.size() * (size_t)N;
        uitems.resize(cnt); ucb.resize(cnt); mean.resize(cnt); var.resize(cnt);
        rc = hpf_recommend_ucb(h, ml.users.data(), (uint32_t)ml.users.size(), ml.ptr.data(), mask ? ml.items.data() : nullptr, N, env.ucb,
                               uitems.data(), ucb.data(), mean.data(), var.data());
        if (rc) die("hpf_recommend_ucb", rc);
        for (size_t b = 0; b < ml.users.size(); ++b)
          for (uint32_t j = 0; j < m && j < N; ++j) {               // write_topn's rule: no padding, no given item
            const size_t e = b * N + j;
            if (!keep(ml.users[b], uitems[e])) continue;
            fprintf(uf, "%d\t%d\t%.5f\t%.5f\t%.5f\n", given.seq2user[ml.users[b]], rt.seq2item[uitems[e]], ucb[e], mean[e], sqrt(var[e]));
            ++ulines;
          }
      }
      if (tf) {
        const size_t cnt = ml.users.size() * (size_t)N;
        titems.resize(cnt * D); tscores.resize(cnt * D);
        for (uint32_t t = 0; t < D; ++t) {
          rc = hpf_recommend_thompson(h, ml.users.data(), (uint32_t)ml.users.size(), ml.ptr.data(), mask ? ml.items.data() : nullptr, N,
                                      env.thompson_seed, t, titems.data() + cnt * t, tscores.data() + cnt * t);
          if (rc) die("hpf_recommend_thompson", rc);
        }
        tlines += write_thompson(tf, ml.users.data(), ml.users.size(), titems.data(), tscores.data(), D, N, m, given.seq2user.data(),
                                 rt.seq2item.data(), keep);
      }
      if (df) {
        const size_t cnt = ml.users.size() * (size_t)N;
        ditems.resize(cnt); dscores.resize(cnt); dmaxsim.resize(cnt);
        rc = hpf_recommend_diverse(h, ml.users.data(), (uint32_t)ml.users.size(), ml.ptr.data(), mask ? ml.items.data() : nullptr, N,
                                   env.diverse_pool, env.diverse, ditems.data(), dscores.data(), dmaxsim.data(), nullptr);
        if (rc) die("hpf_recommend_diverse", rc);
        dlines += write_diverse(df, ml.users.data(), ml.users.size(), ditems.data(), dscores.data(), dmaxsim.data(), N, given.seq2user.data(),
                                rt.seq2item.data(), keep, &dsum);
      }
      if (!ef && !bf) return;
      eu.clear(); ei.clear(); tptr.assign(1, 0);
      for (size_t b = 0; b < ml.users.size(); ++b) {
        for (uint32_t j = 0; j < m && j < N; ++j)                 // the entries write_topn has written
          if (keep(ml.users[b], items[b * N + j])) { eu.push_back(ml.users[b]); ei.push_back(items[b * N + j]); }
        tptr.push_back(ei.size());
      }
      if (bf) {
        rated.resize(eu.size() * (size_t)TB); con.resize(eu.size() * (size_t)TB);
        rc = hpf_because(h, ml.users.data(), (uint32_t)ml.users.size(), tptr.data(), ei.data(), TB, rated.data(), con.data(), nullptr, nullptr);
        if (rc) die("hpf_because", rc);
        for (size_t p = 0; p < eu.size(); ++p)
          for (uint32_t r = 0; r < TB && rated[p * TB + r] != 0xffffffffu; ++r, ++blines)
            fprintf(bf, "%d\t%d\t%d\t%.8f\n", given.seq2user[eu[p]], rt.seq2item[ei[p]], rt.seq2item[rated[p * TB + r]], con[p * TB + r]);
        bpairs += eu.size();
      }
      if (!ef) return;
      fac.resize(eu.size() * (size_t)T); con.resize(eu.size() * (size_t)T);
      rc = hpf_explain(h, eu.data(), ei.data(), eu.size(), T, fac.data(), con.data());
      if (rc) die("hpf_explain", rc);
      for (size_t p = 0; p < eu.size(); ++p)
        for (uint32_t r = 0; r < T && fac[p * T + r] != 0xffffffffu; ++r, ++elines)
          fprintf(ef, "%d\t%d\t%d\t%.8f\n", given.seq2user[eu[p]], rt.seq2item[ei[p]], fac[p * T + r], con[p * T + r]);
      epairs += eu.size();
    });
    close_or_die(f, rpath);
    write_line(env.file_str(stem + ".txt"), "%u\t%llu\t%u\n", given.n, lines, N);
    if (uf) {
      close_or_die(uf, upath);
      write_line(env.file_str(stem + "_ucb.txt"), "%u\t%llu\t%u\t%g\n", given.n, ulines, N, env.ucb);
      env.lerr("-ucb: %llu lines in %s_ucb.tsv, z = %g", ulines, stem.c_str() + 1, env.ucb);
    }
    if (df) {
      close_or_die(df, dpath);
      write_line(env.file_str(stem + "_diverse.txt"), "%u\t%llu\t%u\t%u\t%g\t%.5f\n", given.n, dlines, N, env.diverse_pool, env.diverse,
                 dlines ? dsum / (double)dlines : 0.0);
      env.lerr("-diverse: %llu lines in %s_diverse.tsv, pool %u, lambda %g, mean maxsim %.5f", dlines, stem.c_str() + 1, env.diverse_pool,
               env.diverse, dlines ? dsum / (double)dlines : 0.0);
    }
    if (tf) {
      close_or_die(tf, tpath);
      write_line(env.file_str(stem + "_thompson.txt"), "%u\t%llu\t%u\t%u\t%llu\n", given.n, tlines, N, D, (unsigned long long)env.thompson_seed);
      env.lerr("-thompson: %llu lines in %s_thompson.tsv, %u draws, seed %llu", tlines, stem.c_str() + 1, D, (unsigned long long)env.thompson_seed);
    }
    if (ef) {
      close_or_die(ef, epath);
      write_line(env.file_str(stem + "_explain.txt"), "%llu\t%llu\t%u\n", epairs, elines, T);
      env.lerr("-explain: %llu pairs, %llu lines in %s_explain.tsv", epairs, elines, stem.c_str() + 1);
    }
    if (bf) {
      close_or_die(bf, bpath);
      write_line(env.file_str(stem + "_because.txt"), "%llu\t%llu\t%u\n", bpairs, blines, TB);
      env.lerr("-because: %llu pairs, %llu lines in %s_because.tsv", bpairs, blines, stem.c_str() + 1);
    }
    return lines;
  }
  void recommend_report() {
    if (env.because) load_model_elog();
    if (env.ucb_set || env.thompson) load_model_shapes(false);
    const unsigned long long lines = recommend_lists(rt, &rt.validation, "/recommend");
    env.lerr("-recommend: %u users, %llu lines in recommend.tsv", n, lines);
  }

  // -audience N (extension): whom to show an item to -- the N best users of EVERY item, the item's training users with a
  // rating > 0 and its validation users zeroed: -recommend transposed, through hpf_audience.  <stem>.tsv: item id, user id,
  // score -- items in seq order, each list best first, printed by write_topn under the rule that mirrors recommend.tsv's
  // (given.r(user, item) == 0; the padding beyond n users is never printed); <stem>.txt items, lines and N.  The validation
  // pairs are regrouped per item for each chunk (ItemMaskLists); a chunk of items is written before the next is ranked.
  // -fold-in-items' tail is the same report for the new items: their own handle and ratings, and no list beyond the given
  // ratings, which the call masks itself (mask == nullptr).
  // -explain T: as behind -recommend, the (user, item) pairs of the lines just written go to hpf_explain;
  // <stem>_explain.tsv: item id, user id, factor, contribution (%.8f); <stem>_explain.txt: pairs, lines, T.
  unsigned long long audience_lists(const Ratings &given, const HeldOut *mask, const std::string &stem) {
    const uint32_t N = env.audience, T = env.explain, nu = given.n;
    const std::string rpath = env.file_str(stem + ".tsv"), epath = env.file_str(stem + "_explain.tsv");
    FILE *f = open_or_die(rpath, "w"), *ef = T ? open_or_die(epath, "w") : nullptr;
    ItemMaskLists ml; std::vector<uint32_t> users, eu, ei, fac; std::vector<double> scores, con;
    const HeldOut none;
    unsigned long long lines = 0, epairs = 0, elines = 0;
    const std::function<bool(uint32_t, uint32_t)> keep = [&](uint32_t it, uint32_t u) { return given.r(u, it) == 0; };
    for_chunks(given.m, [&](size_t i0, size_t i1) {
      ml.fill(mask ? *mask : none, (uint32_t)i0, (uint32_t)i1);
      users.resize(ml.items.size() * (size_t)N); scores.resize(ml.items.size() * (size_t)N);
      int rc = hpf_audience(h, ml.items.data(), (uint32_t)ml.items.size(), ml.ptr.data(), mask ? ml.users.data() : nullptr, N,
                            users.data(), scores.data());
      if (rc) die("hpf_audience", rc);
      lines += write_topn(f, ml.items.data(), ml.items.size(), users.data(), scores.data(), N, nu, given.seq2item.data(),
                          given.seq2user.data(), keep);
      if (!ef) return;
      eu.clear(); ei.clear();
      for (size_t b = 0; b < ml.items.size(); ++b)
        for (uint32_t j = 0; j < nu && j < N; ++j)                // the entries write_topn has written
          if (keep(ml.items[b], users[b * N + j])) { eu.push_back(users[b * N + j]); ei.push_back(ml.items[b]); }
      fac.resize(eu.size() * (size_t)T); con.resize(eu.size() * (size_t)T);
      rc = hpf_explain(h, eu.data(), ei.data(), eu.size(), T, fac.data(), con.data());
      if (rc) die("hpf_explain", rc);
      for (size_t p = 0; p < eu.size(); ++p)
        for (uint32_t r = 0; r < T && fac[p * T + r] != 0xffffffffu; ++r, ++elines)
          fprintf(ef, "%d\t%d\t%d\t%.8f\n", given.seq2item[ei[p]], given.seq2user[eu[p]], fac[p * T + r], con[p * T + r]);
      epairs += eu.size();
    });
    close_or_die(f, rpath);
    write_line(env.file_str(stem + ".txt"), "%u\t%llu\t%u\n", given.m, lines, N);
    if (ef) {
      close_or_die(ef, epath);
      write_line(env.file_str(stem + "_explain.txt"), "%llu\t%llu\t%u\n", epairs, elines, T);
      env.lerr("-explain: %llu pairs, %llu lines in %s_explain.tsv", epairs, elines, stem.c_str() + 1);
    }
    env.lerr("-audience: %u items, %llu lines in %s.tsv", given.m, lines, stem.c_str() + 1);
    return lines;
  }

  // -similar-items N / -similar-users N (extension): "more like this item" and "users like this one" -- the N nearest other
  // rows of E[beta] (E[theta]) to every row, by cosine or dot product over the K factor columns, through hpf_similar.
  // similar_items.tsv: item id, neighbour item id, score -- items in seq order, each list best first, ids and score printed
  // as recommend.tsv prints them, the padding of a list beyond rows - 1 never printed; similar_items.txt: rows, lines, N,
  // metric.  similar_users.* the same for users.  A chunk of rows is written before the next is ranked.
  void similar_report(bool items) {
    const uint32_t N = items ? env.similar_items : env.similar_users;
    const uint32_t rows = items ? m : n;
    const std::vector<uint32_t> &ids = items ? rt.seq2item : rt.seq2user;
    const int metric = env.similar_metric == "dot" ? HPF_SIM_DOT : HPF_SIM_COSINE;
    const std::string base = items ? "/similar_items" : "/similar_users";
    const std::string rpath = env.file_str(base + ".tsv");
    FILE *f = open_or_die(rpath, "w");
    std::vector<uint32_t> sel, nb; std::vector<double> scores;
    unsigned long long lines = 0;
    for_chunks(rows, [&](size_t r0, size_t r1) {
      sel.clear();
      for (size_t r = r0; r < r1; ++r) sel.push_back((uint32_t)r);
      nb.resize(sel.size() * (size_t)N); scores.resize(sel.size() * (size_t)N);
      int rc = hpf_similar(h, items ? 1 : 0, sel.data(), (uint32_t)sel.size(), N, metric, nb.data(), scores.data());
      if (rc) die("hpf_similar", rc);
      lines += write_topn(f, sel.data(), sel.size(), nb.data(), scores.data(), N, rows - 1, ids.data(), ids.data());
    });
    close_or_die(f, rpath);
    write_line(env.file_str(base + ".txt"), "%u\t%llu\t%u\t%s\n", rows, lines, N, env.similar_metric.c_str());
    env.lerr("-similar-%s: %u rows, %llu lines in %s.tsv", items ? "items" : "users", rows, lines, base.c_str() + 1);
  }

  // -topic-items N / -topic-users N (extension): what a factor is -- the N rows of E[beta] (E[theta]) that load most on each
  // of the K factors, through hpf_factor_top.  topic_items.tsv: factor, item id, value (%.8f) -- factors ascending, each
  // list best first, ids printed as recommend.tsv prints them, the padding of a list beyond the rows never printed;
  // topic_items.txt: factors, lines, N.  topic_users.* the same for users.  One call: K lists of N are O(K x N) on the host.
  void topic_report(bool items) {
    const uint32_t N = items ? env.topic_items : env.topic_users;
    const uint32_t rows = items ? m : n;
    const std::vector<uint32_t> &ids = items ? rt.seq2item : rt.seq2user;
    const std::string base = items ? "/topic_items" : "/topic_users";
    std::vector<uint32_t> top((size_t)k * N), factors(k);
    std::vector<double> vals((size_t)k * N);
    for (uint32_t c = 0; c < k; ++c) factors[c] = c;
    int rc = hpf_factor_top(h, items ? 1 : 0, N, top.data(), vals.data());
    if (rc) die("hpf_factor_top", rc);
    const std::string rpath = env.file_str(base + ".tsv");
    FILE *f = open_or_die(rpath, "w");
    const unsigned long long lines = write_topn(f, factors.data(), k, top.data(), vals.data(), N, rows, factors.data(), ids.data(), nullptr, 8);
    close_or_die(f, rpath);
    write_line(env.file_str(base + ".txt"), "%u\t%llu\t%u\n", k, lines, N);
    env.lerr("-topic-%s: %u factors, %llu lines in %s.tsv", items ? "items" : "users", k, lines, base.c_str() + 1);
  }

  // -fold-in FILE (extension; HGAPRec::test(), hgaprec.cc:2257-2346): the users of FILE, who need not be in -dir, folded
  // into the saved model.  The item side comes from -model-dir as SHAPE and RATE (E alone does not give Elog) through the
  // strict readers; the host forms E = shape / rate and Elog = psi(shape) - log(rate) and hands them to a second handle
  // that holds the new users; hpf_fold_in runs -fold-iters iterations from the prior (-fold-tol: a stopping time per
  // user).  Output: the user-side files of save_model under the prefix foldin_, through the same writers; foldin.txt
  // (users, nonzeros, lines skipped for an unknown item, T, X, iterations min / mean / max); with -recommend N also
  // foldin_recommend.tsv / .txt, recommend_report's lines for the new users with their given ratings masked (and with -explain T
  // foldin_recommend_explain.tsv / .txt, with -because T foldin_recommend_because.tsv / .txt: the second handle holds all the call reads;
  // with -ucb Z foldin_recommend_ucb.tsv / .txt: the item side's shapes are handed in too, the new users' the fold-in has left;
  // with -thompson D foldin_recommend_thompson.tsv / .txt from the same shapes; with -diverse L foldin_recommend_diverse.tsv /
  // .txt, which needs nothing beyond E).
  //
  // -fold-in-items FILE (extension) is the mirror, for a catalogue that grows: the ITEMS of FILE, which need not be in -dir,
  // rated by users of -dir (Ratings::read_fold_in_items).  The USER side comes from -model-dir as shape and rate
  // (htheta / theta, with -bias thetabias), the second handle holds the n users x the new items, hpf_fold_in_items runs
  // the iterations.  Output: the item-side files of save_model under foldin_ (foldin_hbeta*.tsv, foldin_betarate*.tsv,
  // foldin_betabias*.tsv) and foldin_items.txt (items, ratings, lines skipped for an unknown user, T, X, iterations
  // min / mean / max); with -audience N also foldin_audience.tsv / .txt, audience_lists' lines for the new items with their
  // given ratings masked (and with -explain T foldin_audience_explain.tsv / .txt).
  void fold_in_report(bool items) {
    const char *flag = items ? "-fold-in-items" : "-fold-in";
    const std::string &file = items ? env.fold_in_items : env.fold_in;
    Ratings nu; uint64_t skipped = 0;
    const int frc = items ? rt.read_fold_in_items(file, &nu, &skipped) : rt.read_fold_in(file, &nu, &skipped);
    if (frc) { fprintf(stderr, "error: %s: cannot %s %s\n", flag, frc == -1 ? "open" : "parse", file.c_str()); exit(1); }
    // the frozen side: the items of the model for new users, its users for new items
    const uint32_t fr = items ? n : m;
    const std::vector<uint32_t> &fids = items ? rt.seq2user : rt.seq2item;
    const std::string fbase = items ? (env.hier ? "htheta" : "theta") : (env.hier ? "hbeta" : "beta");
    const std::string fbias = items ? "thetabias" : "betabias";
    std::string err;
    std::vector<double> E, L((size_t)fr * k), rate;
    load(fbase + "_shape.tsv", E, fr, k, &fids);
    const std::string rate_path = env.hier ? load(fbase + "_rate.tsv", rate, fr, k, &fids) : load(fbase + "_rate.tsv", rate, k, 1, nullptr);
    if (gamma_expectations(E.data(), L.data(), rate.data(), fr, k, !env.hier, rate_path, &err)) model_die(err);
    std::vector<double> bE, bL(env.bias ? fr : 0);
    if (env.bias) {
      load(fbias + "_shape.tsv", bE, fr, 1, &fids);
      const std::string bp = load(fbias + "_rate.tsv", rate, fr, 1, &fids);
      if (gamma_expectations(bE.data(), bL.data(), rate.data(), fr, 1, false, bp, &err)) model_die(err);
    }
    env.lerr("%s: %s side loaded from %s", flag, items ? "user" : "item", env.model_dir.empty() ? "." : env.model_dir.c_str());

    // the folded-in side: nu.n new users, or nu.m new items (rows of the second handle)
    const uint32_t rows = items ? nu.m : nu.n;
    std::vector<uint32_t> iters(rows);
    ScoreModes f(*this);                         // the second handle: its die() reports that handle
    f.h = nullptr;
    if (!items || rows) {                        // (a handle of zero items does not exist: nothing to fold in, empty files)
      hpf_config cfg = config(nu.n, nu.n);
      cfg.n_items = nu.m;
      cfg.novb = 0;                              // the new rows are never iterated by vb_bias()
      int rc = hpf_create(&cfg, &f.h);
      if (rc) f.die("hpf_create (fold-in)", rc);
      rc = hpf_upload_csr(f.h, nu.rowptr.data(), nu.col.data(), env.binary_data ? nullptr : nu.val.data());
      if (rc) f.die("hpf_upload_csr (fold-in)", rc);
      f.put(items ? HPF_THETA_E : HPF_BETA_E, E); f.put(items ? HPF_THETA_ELOG : HPF_BETA_ELOG, L);
      if (env.bias) { f.put(items ? HPF_UBIAS_E : HPF_IBIAS_E, bE); f.put(items ? HPF_UBIAS_ELOG : HPF_IBIAS_ELOG, bL); }
      rc = items ? hpf_fold_in_items(f.h, env.fold_iters, env.fold_tol, iters.data()) : hpf_fold_in(f.h, env.fold_iters, env.fold_tol, iters.data());
      if (rc) f.die(items ? "hpf_fold_in_items" : "hpf_fold_in", rc);
    }

    // that side's files of save_model, prefix foldin_
    const std::vector<uint32_t> &ids = items ? nu.seq2item : nu.seq2user;
    std::vector<double> buf;
    auto write = [&](const std::string &name, hpf_state w, uint32_t nrows, uint32_t cols, bool as_vector) {
      buf.assign((size_t)nrows * cols, 0.0);
      const int r2 = f.h ? hpf_get_state(f.h, w, buf.data(), buf.size()) : 0;
      if (r2) f.die("hpf_get_state", r2);
      const std::string path = env.file_str("/foldin_" + name);
      if (as_vector ? save_vector(path, buf.data(), nrows, ids.data(), (uint32_t)ids.size())
                    : save_matrix(path, buf.data(), nrows, cols, ids.data(), (uint32_t)ids.size())) io_die("cannot write", path);
    };
    const char *suf[3] = {"_shape.tsv", "_rate.tsv", ".tsv"};
    const std::string tb = items ? (env.hier ? "hbeta" : "beta") : (env.hier ? "htheta" : "theta");
    const hpf_state obj = items ? HPF_BETA_SHAPE : HPF_THETA_SHAPE, prior = items ? HPF_ETA_SHAPE : HPF_XI_SHAPE, biasw = items ? HPF_IBIAS_SHAPE : HPF_UBIAS_SHAPE;
    for (int j = 0; j < 3; ++j) {
      if (j == 1 && !env.hier) { if (f.h) write(tb + suf[j], (hpf_state)(obj + 1), k, 1, true); }     // GPMatrixGR rate: the K-vector
      else write(tb + suf[j], (hpf_state)(obj + j), rows, k, false);
      if (env.hier) write(std::string(items ? "betarate" : "thetarate") + suf[j], (hpf_state)(prior + j), rows, 1, true);
      if (env.bias) write(std::string(items ? "betabias" : "thetabias") + suf[j], (hpf_state)(biasw + j), rows, 1, false);
    }
    uint32_t imin = 0, imax = 0; double isum = 0;
    for (uint32_t u = 0; u < rows; ++u) { imin = u ? std::min(imin, iters[u]) : iters[u]; imax = std::max(imax, iters[u]); isum += iters[u]; }
    write_line(env.file_str(items ? "/foldin_items.txt" : "/foldin.txt"), "%u\t%llu\t%llu\t%u\t%g\t%u\t%.5f\t%u\n", rows, (unsigned long long)nu.col.size(),
               (unsigned long long)skipped, env.fold_iters, env.fold_tol, imin, rows ? isum / rows : 0.0, imax);
    env.lerr("%s: %u %s, %llu ratings, %llu lines skipped (unknown %s), iterations %u .. %u", flag, rows, items ? "items" : "users",
             (unsigned long long)nu.col.size(), (unsigned long long)skipped, items ? "user" : "item", imin, imax);
    if (!items && env.recommend && (env.ucb_set || env.thompson) && f.h) f.load_model_shapes(true);     // after the files: the fold-in's output is that of a run without -ucb
    if (!items && env.recommend) f.recommend_lists(nu, nullptr, "/foldin_recommend");
    if (items && env.audience) f.audience_lists(nu, nullptr, "/foldin_audience");
    if (f.h) hpf_destroy(f.h);
  }
};

}  // namespace

void score(Cli &c, const std::function<void()> &gen_ranking)
{
  ScoreModes s(c);
  if (!c.env.fold_in.empty()) return s.fold_in_report(false);      // needs the item side only, as shape and rate
  if (!c.env.fold_in_items.empty()) return s.fold_in_report(true);  // ... the user side only
  s.load_model();
  if (c.env.rmse) s.compute_rmse();
  else if (c.env.msr) s.gen_msr_csv();
  else if (c.env.eval_all) s.eval_all_report();
  else if (c.env.recommend) s.recommend_report();
  else if (c.env.audience) s.audience_lists(c.rt, &c.rt.validation, "/audience");
  else if (c.env.similar_items || c.env.similar_users) {
    if (c.env.similar_items) s.similar_report(true);
    if (c.env.similar_users) s.similar_report(false);
  }
  else if (c.env.topic_items || c.env.topic_users) {
    if (c.env.topic_items) s.topic_report(true);
    if (c.env.topic_users) s.topic_report(false);
  }
  else gen_ranking();
}

}  // namespace hgaprec
