// hgaprec_cli.hpp -- what the two halves of the `hgaprec` command line share: the training run (hgaprec_main.cpp) and
// the reports on a saved model (score_modes.cpp).  The flags, the ratings, the library handle and the ways to fail.
#pragma once
#include "../../../include/hpf.h"
#include "hgaprec_host.hpp"

#include <cerrno>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace hgaprec {

struct Cli {
  Env &env; Ratings &rt; hpf_handle *h = nullptr; int rank = 0;
  Cli(Env &e, Ratings &r, int rank_ = 0) : env(e), rt(r), rank(rank_) {}

  void die(const char *what, int rc) const {
    fprintf(stderr, "error: [rank %d] %s: %s (%s)\n", rank, what, hpf_strerror(rc), h ? hpf_last_error(h) : "");
    exit(-1);
  }
  // output failures are fatal and say which file: a truncated factor file or a
  // missing part must never end in exit code 0
  [[noreturn]] void io_die(const char *what, const std::string &path) const {
    fprintf(stderr, "error: [rank %d] %s %s: %s\n", rank, what, path.c_str(), strerror(errno));
    exit(-1);
  }
  FILE *open_or_die(const std::string &path, const char *mode) const {
    FILE *f = fopen(path.c_str(), mode);
    if (!f) io_die("cannot open", path);
    return f;
  }
  void close_or_die(FILE *f, const std::string &path) const {
    if (ferror(f) | fclose(f)) io_die("cannot write", path);
  }
  [[noreturn]] void model_die(const std::string &msg) const {
    fprintf(stderr, "error: cannot load the model: %s\n", msg.c_str());
    exit(1);
  }
  bool test_hit(int v) const {                   // ratings.hh:183-189
    return env.binary_data ? v >= 1 : (uint32_t)v >= env.rating_threshold;
  }
  // a file of one formatted line (rmse.txt, max.txt, recommend.txt, ...)
  __attribute__((format(printf, 3, 4))) void write_line(const std::string &path, const char *fmt, ...) const {
    FILE *f = open_or_die(path, "w");
    va_list ap; va_start(ap, fmt); vfprintf(f, fmt, ap); va_end(ap);
    close_or_die(f, path);
  }
  template <class V>
  void put(hpf_state w, const V &v) const {
    const int rc = hpf_set_state(h, w, v.data(), v.size());
    if (rc) die("hpf_set_state", rc);
  }
  // the handle's configuration for n_users of n_users_total users, from the flags
  hpf_config config(uint32_t n_users, uint32_t n_users_total, uint32_t n_ranks = 1, uint32_t rank_ = 0) const {
    hpf_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.n_users = n_users; cfg.n_items = rt.m; cfg.K = env.k;
    cfg.hier = env.hier; cfg.bias = env.bias; cfg.binary = env.binary_data;
    cfg.novb = env.vb ? 0u : 1u;              // read by the library only where the reference reads it (vb_bias)
    cfg.tiling = env.no_tiles ? 1u : 0u;
    cfg.w_storage = env.w48 ? 2u : env.plain_rows ? 3u : 0u; // 0 / 3: exact fp64 either way (3 = never pack the rows); 2: -w48, opt-in, lossy
    cfg.n_users_total = n_users_total; cfg.device = env.device; cfg.n_ranks = n_ranks; cfg.rank = rank_;
    cfg.s_prior = 0.3; cfg.r_prior = 0.3;
    return cfg;
  }
};

// One report on a saved model, in the reference's order of tests (main.cc:254-285, then -gen-ranking); c.h holds the
// whole data set on one GPU.  gen_ranking: the training run's ranking of the test users (do_on_stop calls it too).
void score(Cli &c, const std::function<void()> &gen_ranking);

}  // namespace hgaprec
