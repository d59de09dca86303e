// host_capi.cpp -- C exports of the host side for the CPU test-suite
// (tests/test_host_*.py load libhgaprec_host.so through ctypes).  Not part of
// the device ABI; the device ABI is include/hpf.h.
#include "hgaprec_host.hpp"

#include <cstring>

using namespace hgaprec;

extern "C" {

// Env: parse argv (without argv[0]) and return the output-directory name
int hg_prefix(int argc, char **argv, char *out, size_t cap, char *bad, size_t badcap)
{
  Env e; std::string b;
  std::vector<char *> av; av.push_back((char *)"hgaprec");
  for (int i = 0; i < argc; ++i) av.push_back(argv[i]);
  int rc = e.parse((int)av.size(), av.data(), false, &b);
  if (rc) { if (bad) { strncpy(bad, b.c_str(), badcap - 1); bad[badcap - 1] = 0; } return rc; }
  std::string p = e.make_prefix();
  strncpy(out, p.c_str(), cap - 1); out[cap - 1] = 0;
  return 0;
}

// Env::open_output in the current directory (creates the dir + param.txt head)
int hg_open_output(int argc, char **argv, char *out, size_t cap)
{
  Env e; std::string b;
  std::vector<char *> av; av.push_back((char *)"hgaprec");
  for (int i = 0; i < argc; ++i) av.push_back(argv[i]);
  if (e.parse((int)av.size(), av.data(), false, &b)) return 1;
  if (e.open_output()) return -1;
  strncpy(out, e.prefix.c_str(), cap - 1); out[cap - 1] = 0;
  e.close_output();
  return 0;
}

Ratings *hg_ratings_new(uint32_t cap_n, uint32_t cap_m, int binary, uint32_t thr)
{
  Ratings *r = new Ratings(); r->cap_n = cap_n; r->cap_m = cap_m; r->binary = binary != 0;
  r->rating_threshold = thr; return r;
}
void hg_ratings_free(Ratings *r) { delete r; }
int hg_ratings_read_train(Ratings *r, const char *path) { return r->read_train(path); }
int hg_ratings_read_heldout(Ratings *r, const char *path, int which)
{ return r->read_heldout(path, which == 0 ? &r->validation : &r->test); }
// -fold-in FILE against the items of `model`: a new Ratings holding the new users (hg_ratings_free), NULL with *rc = -1 / -2
Ratings *hg_ratings_read_fold_in(const Ratings *model, const char *path, uint64_t *skipped_unknown, int *rc)
{
  Ratings *out = new Ratings();
  *rc = model->read_fold_in(path, out, skipped_unknown);
  if (*rc) { delete out; return nullptr; }
  return out;
}
// -fold-in-items FILE against the users of `model`: a new Ratings holding the new items over model's users
Ratings *hg_ratings_read_fold_in_items(const Ratings *model, const char *path, uint64_t *skipped_unknown, int *rc)
{
  Ratings *out = new Ratings();
  *rc = model->read_fold_in_items(path, out, skipped_unknown);
  if (*rc) { delete out; return nullptr; }
  return out;
}
uint32_t hg_ratings_n(const Ratings *r) { return r->n; }
uint32_t hg_ratings_m(const Ratings *r) { return r->m; }
uint64_t hg_ratings_nnz(const Ratings *r) { return r->col.size(); }
const int64_t *hg_ratings_rowptr(const Ratings *r) { return r->rowptr.data(); }
const uint32_t *hg_ratings_col(const Ratings *r) { return r->col.data(); }
const uint8_t *hg_ratings_val(const Ratings *r) { return r->val.data(); }
const uint32_t *hg_ratings_seq2user(const Ratings *r) { return r->seq2user.data(); }
const uint32_t *hg_ratings_seq2item(const Ratings *r) { return r->seq2item.data(); }
uint64_t hg_ratings_heldout_count(const Ratings *r, int w) { return (w ? r->test : r->validation).u.size(); }
const uint32_t *hg_ratings_heldout_u(const Ratings *r, int w) { return (w ? r->test : r->validation).u.data(); }
const uint32_t *hg_ratings_heldout_i(const Ratings *r, int w) { return (w ? r->test : r->validation).i.data(); }
const int32_t *hg_ratings_heldout_y(const Ratings *r, int w) { return (w ? r->test : r->validation).y.data(); }
int hg_ratings_write_marginals(const Ratings *r, const char *bu, const char *bi)
{ return r->write_marginals(bu, bi, nullptr, nullptr); }
int hg_ratings_save_cache(const Ratings *r, const char *dir) { return r->save_cache(dir); }
int hg_ratings_load_cache(Ratings *r, const char *dir) { return r->load_cache(dir); }
int hg_ratings_test_users(const Ratings *r, const char *path, uint32_t *out, uint32_t cap)
{
  std::vector<uint32_t> ids;
  if (r->read_test_users(path, &ids)) return -1;
  for (uint32_t j = 0; j < ids.size() && j < cap; ++j) out[j] = ids[j];
  return (int)ids.size();
}

void hg_mt_u32(double seed, uint32_t count, uint32_t *out)
{
  Mt19937 r = make_rng(seed);
  for (uint32_t i = 0; i < count; ++i) out[i] = r.next_u32();
}
double hg_digamma(double x) { return digamma(x); }

GammaState *hg_state_new(double seed, uint32_t n, uint32_t m, uint32_t k, int hier, int bias)
{
  GammaState *s = new GammaState();
  Mt19937 r = make_rng(seed);
  initialize_state(r, n, m, k, hier != 0, bias != 0, s);
  return s;
}
// the rows [lo, hi) of the user-side arrays, as a rank of several keeps them; *words_after = the generator's
// next word afterwards (every rank must leave the stream where a single process does)
GammaState *hg_state_new_range(double seed, uint32_t n, uint32_t m, uint32_t k, int hier, int bias,
                               uint32_t lo, uint32_t hi, uint32_t *word_after)
{
  GammaState *s = new GammaState();
  Mt19937 r = make_rng(seed);
  initialize_state(r, n, m, k, hier != 0, bias != 0, s, lo, hi);
  if (word_after) *word_after = r.next_u32();
  return s;
}
void hg_state_free(GammaState *s) { delete s; }
// which: the hpf_state index of include/hpf.h
size_t hg_state_get(const GammaState *s, int which, const double **p)
{
  const StateArray *v[24] = {
    &s->theta_shape, &s->theta_rate, &s->theta_E, &s->theta_Elog,
    &s->beta_shape, &s->beta_rate, &s->beta_E, &s->beta_Elog,
    &s->xi_shape, &s->xi_rate, &s->xi_E, &s->xi_Elog,
    &s->eta_shape, &s->eta_rate, &s->eta_E, &s->eta_Elog,
    &s->ubias_shape, &s->ubias_rate, &s->ubias_E, &s->ubias_Elog,
    &s->ibias_shape, &s->ibias_rate, &s->ibias_E, &s->ibias_Elog };
  if (which < 0 || which >= 24) { *p = nullptr; return 0; }
  *p = v[which]->data();
  return v[which]->size();
}

int hg_save_matrix(const char *path, const double *a, uint32_t rows, uint32_t cols,
                   const uint32_t *ids, uint32_t nids)
{ return save_matrix(path, a, rows, cols, ids, nids); }
int hg_save_vector(const char *path, const double *a, uint32_t rows, const uint32_t *ids, uint32_t nids)
{ return save_vector(path, a, rows, ids, nids); }

// the model reader: 0, or -1 with the message ("<path>: ...") in err
int hg_load_matrix(const char *path, double *out, uint32_t rows, uint32_t cols, const uint32_t *ids, uint32_t nids,
                   char *err, size_t errcap)
{
  std::string e;
  const int rc = load_matrix(path, out, rows, cols, ids, nids, &e);
  if (err && errcap) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return rc;
}
int hg_load_vector(const char *path, double *out, uint32_t rows, const uint32_t *ids, uint32_t nids, char *err, size_t errcap)
{
  std::string e;
  const int rc = load_vector(path, out, rows, ids, nids, &e);
  if (err && errcap) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return rc;
}
// E = shape / rate[c] in place with load_model's check of the rates: 0, or -1 with the message in err
int hg_shape_over_rate(double *E, uint32_t rows, uint32_t cols, const double *rate, const char *rate_path, char *err, size_t errcap)
{
  std::string e;
  const int rc = shape_over_rate(E, rows, cols, rate, rate_path, &e);
  if (err && errcap) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return rc;
}

// E = shape / rate in place and Elog beside it, the rate per element or (per_column) a K-vector: 0, or -1 with the message
int hg_gamma_expectations(double *E, double *Elog, const double *rate, uint64_t rows, uint64_t cols, int per_column,
                          const char *rate_path, char *err, size_t errcap)
{
  std::string e;
  const int rc = gamma_expectations(E, Elog, rate, (size_t)rows, (size_t)cols, per_column != 0, rate_path, &e);
  if (err && errcap) { strncpy(err, e.c_str(), errcap - 1); err[errcap - 1] = 0; }
  return rc;
}

// ---- the loops of the reports
uint32_t hg_ratings_r(const Ratings *r, uint32_t u, uint32_t item) { return r->r(u, item); }
uint32_t hg_ratings_ranked_items(const Ratings *r, uint32_t u) { return r->ranked_items(u); }
const uint32_t *hg_ratings_item_degrees(const Ratings *r) { return r->item_degrees().data(); }
// for_chunks: out[2 * j], out[2 * j + 1] = the j-th visit (as far as cap pairs go); chunk 0 = the default.  Returns the visits
uint64_t hg_chunk_walk(uint64_t rows, uint64_t chunk, uint64_t *out, uint64_t cap)
{
  uint64_t cnt = 0;
  auto visit = [&](size_t r0, size_t r1) { if (cnt < cap) { out[2 * cnt] = r0; out[2 * cnt + 1] = r1; } ++cnt; };
  if (chunk) for_chunks((size_t)rows, visit, (size_t)chunk); else for_chunks((size_t)rows, visit);
  return cnt;
}
void hg_chunk_offsets(const uint64_t *ptr, uint64_t b0, uint64_t b1, uint64_t *out)
{
  std::vector<uint64_t> v;
  chunk_offsets(ptr, (size_t)b0, (size_t)b1, &v);
  memcpy(out, v.data(), v.size() * sizeof(uint64_t));
}
// MaskLists::fill over the validation (which = 0) or test pairs; list may be NULL (the range [lo, hi))
MaskLists *hg_mask_lists_new(const Ratings *r, int which, const uint32_t *list, uint64_t cnt, uint32_t lo, uint32_t hi, uint32_t rebase)
{
  MaskLists *ml = new MaskLists();
  ml->fill(which ? r->test : r->validation, list, (size_t)cnt, lo, hi, rebase);
  return ml;
}
void hg_mask_lists_free(MaskLists *ml) { delete ml; }
// part 0 users (uint32), 1 ptr (uint64), 2 items (uint32): the elements, *p their address
uint64_t hg_mask_lists_get(const MaskLists *ml, int part, const void **p)
{
  if (part == 1) { *p = ml->ptr.data(); return ml->ptr.size(); }
  const std::vector<uint32_t> &v = part ? ml->items : ml->users;
  *p = v.data();
  return v.size();
}
// ItemMaskLists::fill over the validation (which = 0) or test pairs for the items [lo, hi)
ItemMaskLists *hg_item_mask_lists_new(const Ratings *r, int which, uint32_t lo, uint32_t hi)
{
  ItemMaskLists *ml = new ItemMaskLists();
  ml->fill(which ? r->test : r->validation, lo, hi);
  return ml;
}
void hg_item_mask_lists_free(ItemMaskLists *ml) { delete ml; }
// part 0 items (uint32), 1 ptr (uint64), 2 users (uint32): the elements, *p their address
uint64_t hg_item_mask_lists_get(const ItemMaskLists *ml, int part, const void **p)
{
  if (part == 1) { *p = ml->ptr.data(); return ml->ptr.size(); }
  const std::vector<uint32_t> &v = part ? ml->users : ml->items;
  *p = v.data();
  return v.size();
}
// write_topn into a new file; given != NULL: only the entries with given->r(row, item) == 0, the rule of recommend.tsv.
// Returns the lines, -1 when the file cannot be written
int64_t hg_write_topn(const char *path, const Ratings *given, const uint32_t *sel, uint64_t n_sel, const uint32_t *items,
                      const double *scores, uint32_t N, uint32_t real, const uint32_t *row_ids, const uint32_t *item_ids)
{
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  std::function<bool(uint32_t, uint32_t)> keep;
  if (given) keep = [given](uint32_t u, uint32_t it) { return given->r(u, it) == 0; };
  const uint64_t lines = write_topn(f, sel, (size_t)n_sel, items, scores, N, real, row_ids, item_ids, keep);
  return (ferror(f) | fclose(f)) ? -1 : (int64_t)lines;
}
// write_thompson into a new file, as hg_write_topn: items / scores are [D x n_sel x N]
int64_t hg_write_thompson(const char *path, const Ratings *given, const uint32_t *sel, uint64_t n_sel, const uint32_t *items,
                          const double *scores, uint32_t D, uint32_t N, uint32_t real, const uint32_t *row_ids, const uint32_t *item_ids)
{
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  std::function<bool(uint32_t, uint32_t)> keep;
  if (given) keep = [given](uint32_t u, uint32_t it) { return given->r(u, it) == 0; };
  const uint64_t lines = write_thompson(f, sel, (size_t)n_sel, items, scores, D, N, real, row_ids, item_ids, keep);
  return (ferror(f) | fclose(f)) ? -1 : (int64_t)lines;
}
// write_diverse into a new file, as hg_write_topn: items / scores / maxsim are [n_sel x N]; *maxsim_sum (may be null) the sum
// of the maxsim column
int64_t hg_write_diverse(const char *path, const Ratings *given, const uint32_t *sel, uint64_t n_sel, const uint32_t *items,
                         const double *scores, const double *maxsim, uint32_t N, const uint32_t *row_ids, const uint32_t *item_ids,
                         double *maxsim_sum)
{
  FILE *f = fopen(path, "w");
  if (!f) return -1;
  std::function<bool(uint32_t, uint32_t)> keep;
  if (given) keep = [given](uint32_t u, uint32_t it) { return given->r(u, it) == 0; };
  if (maxsim_sum) *maxsim_sum = 0.0;
  const uint64_t lines = write_diverse(f, sel, (size_t)n_sel, items, scores, maxsim, N, row_ids, item_ids, keep, maxsim_sum);
  return (ferror(f) | fclose(f)) ? -1 : (int64_t)lines;
}

// -eval-all's arithmetic from ranks to metrics.  per_user: n_users x 6 integers (ntest, hits10, hits100, best_rank,
// sum_rank, nranked as given); means: users, pairs, precision@10, precision@100, recall@100, mrr, meanrank
void hg_eval_from_ranks(const uint64_t *q_ptr, const uint32_t *rank, const uint32_t *nranked, uint64_t n_users,
                        uint64_t *per_user, double *means)
{
  std::vector<EvalUser> pu(n_users); EvalMeans t;
  eval_from_ranks(q_ptr, rank, nranked, (size_t)n_users, pu.data(), &t);
  for (uint64_t b = 0; b < n_users; ++b) {
    uint64_t *o = per_user + 6 * b;
    o[0] = pu[b].ntest; o[1] = pu[b].hits10; o[2] = pu[b].hits100; o[3] = pu[b].best_rank; o[4] = pu[b].sum_rank; o[5] = nranked[b];
  }
  means[0] = (double)t.users; means[1] = (double)t.pairs; means[2] = t.precision10; means[3] = t.precision100;
  means[4] = t.recall100; means[5] = t.mrr; means[6] = t.meanrank;
}

// user ranges of a multi-process run: out[2*r], out[2*r+1] = [lo, hi) of rank r
void hg_partition_users(const int64_t *rowptr, uint32_t n, int world, uint32_t *out)
{
  std::vector<int64_t> rp(rowptr, rowptr + n + 1);
  auto parts = partition_users(rp, world);
  for (int r = 0; r < world; ++r) { out[2 * r] = parts[r].first; out[2 * r + 1] = parts[r].second; }
}

// format_fixed8 over an array; out receives the strings separated by '\n'
size_t hg_format_fixed8(const double *v, size_t n, char *out)
{
  char *o = out;
  for (size_t i = 0; i < n; ++i) { o += format_fixed8(v[i], o); *o++ = '\n'; }
  return (size_t)(o - out);
}

// feed a validation series through the stop rule; returns the index at which
// it stops (or -1), why[] receives the max.txt code per step
int hg_stop_rule(const uint32_t *iters, const double *a, uint32_t cnt, int *why)
{
  StopRule s; int stop_at = -1;
  for (uint32_t i = 0; i < cnt; ++i) {
    bool st = s.update(iters[i], a[i], &why[i]);
    if (st && stop_at < 0) { stop_at = (int)i; break; }
  }
  return stop_at;
}

}  // extern "C"
