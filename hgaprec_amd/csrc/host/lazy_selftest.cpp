// lazy_selftest.cpp -- hpf_lazy.hpp against a deliberately naive model of the buffers, on a CPU (make lazy; ASan/UBSan).
// The model (Truth) knows nothing of flags.  Per side it says what the buffers hold -- S raw sums or a shape, E current, Elog
// current, W from a sweep / from Elog / outdated -- and per handle whether a fall-back from the packed rows is due and
// whether the start sums are current (and handed to the exchange).  A Sim drives a hpf_lazy::State the way hpf_capi.hip
// does: ask, run the jobs in the order given, report the event.  Over seeded random event orders it checks that
//   - after the jobs of a request everything the request named is current in the model, and no job refreshed a buffer
//     while a fall-back was due or refreshed one twice (a shape materialised twice has the prior added twice);
//   - laziness is not observable: a twin that exports everything after every event refuses exactly the calls the lazy
//     handle refuses, and both hold the same flags and the same buffers once the lazy one has exported everything too;
//   - a refused request leaves every flag as it was;
//   - the snapshot words round-trip, for every combination of the fourteen side bits and both handle bits, a snapshot inside
//     a sequence gives back every flag, and a side word from before bits 9 .. 14 existed loads as it did then.
#include "../hpf_lazy.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

using namespace hpf_lazy;

static int g_failures = 0;
static void fail(const char *fmt, ...)
{
  va_list ap; va_start(ap, fmt);
  fprintf(stderr, "FAIL: "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n");
  va_end(ap);
  if (++g_failures > 20) { fprintf(stderr, "too many failures\n"); exit(1); }
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

enum { W_SWEEP, W_ELOG, W_OUTDATED };

struct Truth {
  bool s_raw[2] = {false, false}, e_cur[2] = {true, true}, l_cur[2] = {true, true};
  int w[2] = {W_OUTDATED, W_OUTDATED};
  bool e_exists[2] = {false, false};
  bool s_exists[2] = {false, false}, bs_exists[2] = {false, false}, be_exists[2] = {false, false};   // a shape, a bias shape, a bias E is in place
  bool unpackable[2] = {false, false};     // the Elog handed in has a spread the packed rows cannot hold
  bool due = false; int skipped = 0;       // a fall-back is due; iterations the passes have skipped since
  bool packed = false;
  bool sums_cur = false, exchanged = false;
  int phase = 0; uint32_t iterations = 0;
  bool same(const Truth &o) const
  {
    for (int k = 0; k < 2; ++k)
      if (s_raw[k] != o.s_raw[k] || e_cur[k] != o.e_cur[k] || l_cur[k] != o.l_cur[k] || w[k] != o.w[k] || e_exists[k] != o.e_exists[k] ||
          s_exists[k] != o.s_exists[k] || bs_exists[k] != o.bs_exists[k] || be_exists[k] != o.be_exists[k]) return false;
    return due == o.due && packed == o.packed && sums_cur == o.sums_cur && exchanged == o.exchanged && phase == o.phase && iterations == o.iterations;
  }
};

// event kinds: 24 sets (obj * 4 + kind; the two bias rates are accepted and ignored before anything is asked), then these
enum { EV_USER_SWEEP = 24, EV_ITEM_SWEEP, EV_ITERATE, EV_FLUSH, EV_FOLD_USERS, EV_FOLD_ITEMS, EV_SNAPSHOT, EV_REQUEST, N_EVENTS };
static bool event_exists(int k) { return k != 4 * 4 + 1 && k != 5 * 4 + 1; }
struct Event { int kind; int need, side; bool flag; int count; };

static std::set<int> g_events_seen, g_needs_seen;
static std::set<std::pair<int, int>> g_pairs;

struct Sim {
  Config cfg; bool comm; const char *name; unsigned seed;
  State st; Truth t;
  int last_event = -1;

  Sim(const Config &c, bool comm_, bool packed, const char *name_, unsigned seed_) : cfg(c), comm(comm_), name(name_), seed(seed_), st(c) { t.packed = packed; }
  Now now() const { return {t.phase, t.iterations, t.packed, comm}; }

  // ---- the executors, as the model sees them
  void sweep(int sd) { st.swept(sd); t.e_exists[sd] = t.s_exists[sd] = t.bs_exists[sd] = t.be_exists[sd] = true; if (cfg.rows[sd]) { t.s_raw[sd] = true; t.e_cur[sd] = t.l_cur[sd] = false; t.w[sd] = W_SWEEP; } }
  bool iterate()
  {
    if (!request(ITERATION)) return false;
    st.iteration_begun();
    if (t.due) t.skipped++;
    sweep(USERS); sweep(ITEMS);
    t.iterations++;
    return true;
  }
  void fall_back()
  {
    t.due = false; t.packed = false;
    const int redo = t.skipped; t.skipped = 0;
    for (int sd = 0; sd < 2; ++sd) {
      const Repair how = st.fell_back(sd);
      if (!cfg.rows[sd]) { CHECK(how == REPAIR_NOTHING, "%s seed %u: repair %d of an empty side", name, seed, how); continue; }
      switch (how) {
        case REPAIR_FROM_ELOG: CHECK(t.w[sd] != W_SWEEP, "%s seed %u: W of side %d was a sweep's, to be derived from Elog", name, seed, sd); t.w[sd] = W_OUTDATED; break;
        case REPAIR_REPEAT_SWEEP: CHECK(t.w[sd] == W_SWEEP && t.s_raw[sd], "%s seed %u: repeat of a sweep on side %d: W %d, S raw %d", name, seed, sd, t.w[sd], t.s_raw[sd]); break;
        case REPAIR_REPEAT_ON_SHAPE: CHECK(t.w[sd] == W_SWEEP && !t.s_raw[sd], "%s seed %u: repeat on the shape on side %d: W %d, S raw %d", name, seed, sd, t.w[sd], t.s_raw[sd]); break;
        case REPAIR_NOTHING: fail("%s seed %u: no repair of side %d", name, seed, sd); break;
      }
    }
    CHECK(!redo || !cfg.several, "%s seed %u: iterations skipped on a rank of several", name, seed);
    t.iterations -= redo;
    for (int k = 0; k < redo; ++k) CHECK(iterate(), "%s seed %u: a skipped iteration was refused", name, seed);
  }
  void run(Job j)
  {
    const int sd = (j == ES_ITEMS || j == ELOG_ITEMS) ? ITEMS : USERS;
    switch (j) {
      case RECOVER: if (t.due) fall_back(); break;
      case REPORT: CHECK(!t.due, "%s seed %u: flags reported while a fall-back is due", name, seed); break;
      case ES_USERS: case ES_ITEMS:
        if (cfg.rows[sd]) {
          CHECK(!t.due, "%s seed %u: S / E of side %d refreshed while a fall-back is due", name, seed, sd);
          CHECK(t.s_raw[sd], "%s seed %u: shape of side %d materialised twice", name, seed, sd);
          t.s_raw[sd] = false; t.e_cur[sd] = true;
        }
        st.refreshed(j);
        break;
      case ELOG_USERS: case ELOG_ITEMS:
        if (cfg.rows[sd]) {
          CHECK(!t.due && !t.s_raw[sd], "%s seed %u: Elog of side %d rebuilt from raw sums or while a fall-back is due", name, seed, sd);
          CHECK(!t.l_cur[sd], "%s seed %u: Elog of side %d rebuilt though current", name, seed, sd);
          t.l_cur[sd] = true;
        }
        st.refreshed(j);
        break;
      case DERIVE_W:
        for (int attempt = 0; attempt < 2; ++attempt) {
          bool flushed = false;
          for (int k = 0; k < 2; ++k) {
            if (!st.w_due(k)) continue;
            st.w_derived(k);
            CHECK(t.l_cur[k], "%s seed %u: W of side %d derived from an outdated Elog", name, seed, k);
            t.w[k] = W_ELOG;
            if (t.packed && t.unpackable[k]) flushed = true;
          }
          if (!flushed) break;
          t.due = true; fall_back();
        }
        break;
      case COLUMN_SUMS:
        CHECK(t.e_cur[ITEMS] && (!cfg.jacobi || t.e_cur[USERS] || !cfg.rows[USERS]), "%s seed %u: column sums of an outdated E", name, seed);
        t.sums_cur = true; t.exchanged = false;
        break;
      case DERIVED_DONE: st.derived(); break;
      case EXCHANGE_START_SUMS:
        CHECK(t.sums_cur, "%s seed %u: outdated start sums handed to the exchange", name, seed);
        t.exchanged = true; st.start_sums_handed(comm);
        break;
      case N_JOBS: break;
    }
  }

  // what the request named is current
  bool side_ok(int sd, bool elog) const { return !cfg.rows[sd] || (!t.s_raw[sd] && t.e_cur[sd] && (!elog || t.l_cur[sd])); }
  bool derived_ok() const { return (!cfg.rows[USERS] || t.w[USERS] != W_OUTDATED) && t.w[ITEMS] != W_OUTDATED && t.sums_cur; }
  bool holds(Need need, int sd, int kind) const
  {
    const int oth = 1 - sd;
    switch (need) {
      case FLAGS: case PATCH_VECTOR: case OVERWRITE_ALL: return !t.due;
      case FOLD_SWEEPS: return !cfg.rows[sd] || !t.due;
      case SWEEP_VECTORS: case BIAS_RATE: return t.phase != 0 || !t.due;
      case STATE_E: case FACTORS: return !t.due && side_ok(sd, false);
      case STATE_ELOG: return !t.due && side_ok(sd, true);
      case PATCH: return !t.due && side_ok(sd, kind == 0 || kind == 3);
      case SCORING: return !t.due && side_ok(USERS, false) && side_ok(ITEMS, false);
      case SCORES: return side_ok(USERS, false) && side_ok(ITEMS, false);
      case E_IS_SET: return true;
      case ELBO: return side_ok(USERS, true) && side_ok(ITEMS, true);
      case ELBO_FROM_W: return side_ok(USERS, true) && side_ok(ITEMS, true) && derived_ok();
      case ITERATION: return derived_ok() && (!(cfg.jacobi && cfg.several) || t.exchanged) && (!(cfg.several && t.packed) || !t.due);
      case DERIVED: return derived_ok();
      case GATHER_PROBE: return !t.due && derived_ok();
      case START_SUMS: return derived_ok() && (!(cfg.jacobi && cfg.several) || t.exchanged);
      case FOLD_FUSED: return !cfg.rows[sd] || (!t.due && side_ok(oth, true));
      case FOLD_SWEEPS_RUN: return derived_ok() && (sd != ITEMS || side_ok(oth, false));
      case FOLD_SWEEPS_END: return side_ok(sd, true);
      case BECAUSE: return !t.due && side_ok(USERS, true) && side_ok(ITEMS, true);
      case MOMENTS: return !t.due && side_ok(USERS, false) && side_ok(ITEMS, false);
      case N_NEEDS: break;
    }
    return false;
  }

  // E and the shape of a side, with -bias of its bias too, are in place: handed in, folded in or a sweep's
  bool moments_exist(int sd) const { return t.e_exists[sd] && t.s_exists[sd] && (!cfg.bias || (t.be_exists[sd] && t.bs_exists[sd])); }

  // a call's prologue -> it was not refused
  bool request(Need need, int sd = -1, int kind = -1)
  {
    g_needs_seen.insert(need); g_pairs.insert({last_event, (int)need});
    const uint32_t before = st.fingerprint();
    const Todo todo = st.ask(need, now(), sd, kind);
    CHECK(st.fingerprint() == before, "%s seed %u: asking for %d changed the flags", name, seed, need);
    if (todo.status) {
      CHECK(todo.status == HPF_ERR_STATE && todo.error && todo.n == 0, "%s seed %u: a refusal of %d without a message", name, seed, need);
      if (need == SCORING || need == SCORES || need == E_IS_SET) CHECK(!(t.e_exists[USERS] && t.e_exists[ITEMS]), "%s seed %u: E exists, need %d refused", name, seed, need);
      if (need == MOMENTS)
        CHECK(!(moments_exist(USERS) && moments_exist(ITEMS)), "%s seed %u: E and shape exist, need %d refused", name, seed, need);
      return false;
    }
    if (need == MOMENTS) CHECK(moments_exist(USERS) && moments_exist(ITEMS), "%s seed %u: need %d granted though E or a shape does not exist", name, seed, need);
    if (need == SCORING || need == SCORES || need == FACTORS || need == BECAUSE)
      CHECK(need == FACTORS ? t.e_exists[sd] : (t.e_exists[USERS] && t.e_exists[ITEMS]), "%s seed %u: need %d granted though E does not exist", name, seed, need);
    for (int j = 0; j < todo.n; ++j) run(todo.job[j]);
    CHECK(holds(need, sd, kind), "%s seed %u: after the jobs of need %d (side %d, kind %d) not everything it named is current", name, seed, need, sd, kind);
    return true;
  }

  void fold_mark(int sd)
  {
    st.folded(sd);
    t.s_raw[sd] = false; t.e_cur[sd] = t.l_cur[sd] = true; t.w[sd] = W_OUTDATED; t.e_exists[sd] = true; t.unpackable[sd] = false; t.sums_cur = false;
    t.s_exists[sd] = true; if (cfg.bias) t.bs_exists[sd] = t.be_exists[sd] = true;
  }

  // -> the event happened (false: refused, or not a call for this moment)
  bool apply(const Event &e)
  {
    bool done = false;
    if (e.kind < 24) {
      const int obj = e.kind / 4, kind = e.kind % 4, sd = obj & 1;
      if (t.phase != 0 || ((obj == 2 || obj == 3) && !cfg.hier) || (obj >= 4 && !cfg.bias) || (kind == 1 && obj >= 4)) return false;
      const bool vector = obj == 2 || obj == 3 || kind == 1;
      if ((done = request(vector ? PATCH_VECTOR : PATCH, sd, kind))) {
        st.state_set(obj, kind);
        if (!vector && kind == 2 && obj <= 1) t.e_exists[sd] = true;
        if (!vector && kind == 2 && obj >= 4) t.be_exists[sd] = true;
        if (!vector && kind == 0) (obj <= 1 ? t.s_exists : t.bs_exists)[sd] = true;
        if (!vector && cfg.rows[sd]) {
          if (kind == 2) t.sums_cur = false;
          if (kind == 3) { t.w[sd] = W_OUTDATED; if (obj <= 1) t.unpackable[sd] = e.flag; }
        }
      }
    } else switch (e.kind) {
      case EV_USER_SWEEP:       // the first three steps of an iteration
        if (t.phase != 0 || !request(ITERATION)) break;
        st.iteration_begun(); if (t.due) t.skipped++;
        sweep(USERS); t.phase = 3; done = true;
        break;
      case EV_ITEM_SWEEP:
        if (t.phase != 3) break;
        sweep(ITEMS); t.phase = 0; t.iterations++; done = true;
        break;
      case EV_ITERATE: case EV_FLUSH:      // a call of e.count iterations; EV_FLUSH: the first sweep cannot pack its rows
        if (t.phase != 0) break;
        for (int k = 0; k < e.count; ++k) {
          if (!iterate()) break;
          done = true;
          if (e.kind == EV_FLUSH && k == 0 && t.packed) t.due = true;
          if (cfg.several && k + 1 < e.count && t.due) break;      // the next iteration of the call would repair first: the same thing
        }
        break;
      case EV_FOLD_USERS: case EV_FOLD_ITEMS: {
        const int sd = e.kind == EV_FOLD_ITEMS;
        if (t.phase != 0 || (sd == ITEMS && cfg.several)) break;
        if (!request(e.flag ? FOLD_SWEEPS : FOLD_FUSED, sd)) break;
        done = true;
        if (!cfg.rows[sd]) break;
        if (e.flag) {
          fold_mark(sd);
          CHECK(request(FOLD_SWEEPS_RUN, sd), "%s seed %u: the sweeps of a fold-in were refused", name, seed);
          for (int k = 0; k < e.count; ++k) sweep(sd);
          request(FOLD_SWEEPS_END, sd);
        }
        fold_mark(sd);
        request(FLAGS);
        break;
      }
      case EV_SNAPSHOT: {
        if (t.phase != 0) break;
        request(SWEEP_VECTORS); request(FLAGS);
        const uint32_t words[2] = {st.snap_side_word(USERS, e.flag, !e.flag), st.snap_side_word(ITEMS, !e.flag, e.flag)};
        const uint32_t dd = st.snap_derived_dirty(), more = st.snap_more_flags();
        request(OVERWRITE_ALL);
        State loaded(cfg);
        loaded.snapshot_loaded(words, dd, more);
        CHECK(loaded.snap_side_word(USERS, e.flag, !e.flag) == words[0] && loaded.snap_side_word(ITEMS, !e.flag, e.flag) == words[1] &&
              loaded.snap_derived_dirty() == dd && loaded.snap_more_flags() == more, "%s seed %u: the snapshot words do not round-trip", name, seed);
        CHECK(loaded.ask(ITERATION, now()).n == st.ask(ITERATION, now()).n, "%s seed %u: a restored handle begins its iteration otherwise", name, seed);
        // (bit 3, tail_partial, is about the exchange buffer of a running job and is not part of a snapshot)
        CHECK((loaded.fingerprint() | 8u) == (st.fingerprint() | 8u), "%s seed %u: flags %#x come back from a snapshot as %#x", name, seed, st.fingerprint(), loaded.fingerprint());
        st = loaded;               // the model is untouched: a snapshot says what was handed in, shapes and bias columns included
        done = true;
        break;
      }
      case EV_REQUEST:
        if (t.phase != 0 && e.need != SWEEP_VECTORS && e.need != BIAS_RATE) break;
        if ((e.need == BIAS_RATE && !cfg.bias) || ((e.need == ELBO || e.need == ELBO_FROM_W) && t.iterations == 0)) break;
        done = request((Need)e.need, e.side);
        break;
    }
    last_event = e.kind;
    if (done) g_events_seen.insert(e.kind);
    return done;
  }

  // nothing is left pending
  void export_everything()
  {
    if (t.phase != 0) return;
    request(STATE_ELOG, USERS); request(STATE_ELOG, ITEMS); request(FLAGS);
  }
};

static void sequences(unsigned n_seeds, unsigned long *n_events)
{
  static const int standalone[] = {FLAGS, SWEEP_VECTORS, BIAS_RATE, STATE_E, STATE_ELOG, SCORING, SCORES, E_IS_SET, FACTORS, ELBO, ELBO_FROM_W,
                                   ITERATION, DERIVED, GATHER_PROBE, START_SUMS, BECAUSE, MOMENTS};
  for (unsigned seed = 0; seed < n_seeds; ++seed) {
    std::mt19937 rng(seed * 2654435761u + 12345u);
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    Config cfg;
    cfg.hier = seed & 1; cfg.bias = seed & 2;
    const bool novb = seed & 4;
    cfg.jacobi = novb && cfg.bias && !cfg.hier;
    cfg.several = seed & 8;
    const bool comm = seed & 16, packed = seed & 32;
    cfg.rows[USERS] = (seed & 0x3c0) != 0x3c0;         // now and then a rank without users
    std::vector<Event> evs;
    // a start state first, most of the time: otherwise nearly everything is refused
    if (seed % 7) for (int obj = 0; obj < 6; ++obj) for (int kind = 2; kind < 4; ++kind) evs.push_back({obj * 4 + kind, 0, 0, false, 0});
    const int len = 20 + pick(21);
    for (int k = 0; k < len; ++k) {
      Event e{0, 0, pick(2), pick(4) == 0, 1 + pick(3)};
      const int r = pick(100);
      if (r < 30) e.kind = pick(24);
      else if (r < 38) e.kind = EV_USER_SWEEP;
      else if (r < 48) e.kind = EV_ITEM_SWEEP;
      else if (r < 58) e.kind = EV_ITERATE;
      else if (r < 64) e.kind = EV_FLUSH;
      else if (r < 68) e.kind = EV_FOLD_USERS;
      else if (r < 72) e.kind = EV_FOLD_ITEMS;
      else if (r < 76) e.kind = EV_SNAPSHOT;
      else { e.kind = EV_REQUEST; e.need = standalone[pick((int)(sizeof standalone / sizeof standalone[0]))]; }
      if (e.kind == EV_REQUEST && e.need == DERIVED) e.side = -1;
      evs.push_back(e);
      if (e.kind == EV_USER_SWEEP && pick(3)) evs.push_back({EV_ITEM_SWEEP, 0, 0, false, 0});
    }
    *n_events += evs.size();
    Sim lazy(cfg, comm, packed, "lazy", seed), twin(cfg, comm, packed, "twin", seed);
    for (const Event &e : evs) {
      const bool a = lazy.apply(e), b = twin.apply(e);
      CHECK(a == b, "seed %u: event %d happened on %s only", seed, e.kind, a ? "the lazy handle" : "the twin");
      twin.export_everything();
    }
    if (lazy.t.phase != 0) { const Event fin{EV_ITEM_SWEEP, 0, 0, false, 0}; lazy.apply(fin); twin.apply(fin); twin.export_everything(); }
    lazy.export_everything();
    CHECK(lazy.st.fingerprint() == twin.st.fingerprint(), "seed %u: flags %#x (lazy) against %#x (twin) with nothing pending", seed, lazy.st.fingerprint(), twin.st.fingerprint());
    CHECK(lazy.t.same(twin.t), "seed %u: the buffers of the lazy handle and of the twin differ with nothing pending", seed);
  }
}

// decoding then encoding is the identity on the bits the format carries
static unsigned snapshot_words()
{
  unsigned n = 0;
  // the fourteen bits of a side word under SNAP_SAYS_HANDED_IN, which every word written now carries
  for (uint32_t w = 0; w < 16384; ++w)
    for (uint32_t more = 0; more < 4; ++more)
      for (uint32_t dd = 0; dd < 2; ++dd, ++n) {
        const uint32_t words[2] = {w | SNAP_SAYS_HANDED_IN, (w ^ 0x3fffu) | SNAP_SAYS_HANDED_IN};
        State st;
        st.snapshot_loaded(words, dd, more);
        for (int k = 0; k < 2; ++k)
          CHECK(st.snap_side_word(k, words[k] & SNAP_RATE_SET, words[k] & SNAP_PRIOR_SHAPE_SET) == words[k], "side word %#x comes back as %#x", words[k],
                st.snap_side_word(k, words[k] & SNAP_RATE_SET, words[k] & SNAP_PRIOR_SHAPE_SET));
        CHECK(st.snap_derived_dirty() == dd && st.snap_more_flags() == more, "handle words %u / %#x do not come back", dd, more);
      }
  // a word written before those bits existed (nine bits, the rest zero) loads as it did then: the bias columns of E and Elog
  // count as handed in with the factors', no shape and no bias rate do -- and is written back saying so
  for (uint32_t w = 0; w < 512; ++w, ++n) {
    const uint32_t words[2] = {w, w ^ 0x1ffu};
    State st;
    st.snapshot_loaded(words, 0, 0);
    for (int k = 0; k < 2; ++k) {
      const uint32_t want = words[k] | SNAP_SAYS_HANDED_IN | ((words[k] & SNAP_HAVE_E) ? SNAP_HAVE_BIAS_E : 0u) | ((words[k] & SNAP_HAVE_L) ? SNAP_HAVE_BIAS_L : 0u);
      const uint32_t got = st.snap_side_word(k, words[k] & SNAP_RATE_SET, words[k] & SNAP_PRIOR_SHAPE_SET);
      CHECK(got == want, "old side word %#x is written back as %#x, not %#x", words[k], got, want);
    }
  }
  return n;
}

int main(int argc, char **argv)
{
  const unsigned n_seeds = argc > 1 ? (unsigned)atoi(argv[1]) : 4096;
  unsigned long n_events = 0;
  sequences(n_seeds, &n_events);
  const unsigned n_words = snapshot_words();
  for (int k = 0; k < N_EVENTS; ++k) if (event_exists(k) && !g_events_seen.count(k)) fail("event kind %d never occurred", k);
  for (int k = 0; k < N_NEEDS; ++k) if (!g_needs_seen.count(k)) fail("request kind %d never occurred", k);
  if (g_failures) { fprintf(stderr, "lazy_selftest: %d failures\n", g_failures); return 1; }
  printf("lazy_selftest ok: %u sequences, %lu events, %zu (event, request) pairs, %zu of %d event kinds, %zu of %d request kinds, %u snapshot words\n",
         n_seeds, n_events, g_pairs.size(), g_events_seen.size(), (int)N_EVENTS - 2, g_needs_seen.size(), (int)N_NEEDS, n_words);
  return 0;
}
