// hpf_lazy.hpp -- what the handle has put off, and what a call must have done before it reads a buffer.
// The library defers work: after a sweep S holds raw sums until somebody asks for a shape, Elog is rebuilt on export, W
// follows a handed-in Elog at the next iteration, a fall-back from the packed rows is repaired at the next synchronisation
// point.  What is pending is the private state of `State`.  hpf_capi.hip can do three things with it: report an event (a
// transition), ask what a call needs (`ask` -> the deferred jobs to run first, in order, or the error the call returns), and
// turn the flags into the words of a snapshot and back.  Plain C++17 without a HIP header: host/lazy_selftest.cpp walks
// random event orders against a naive model of the buffers on a CPU (tests/test_lazy_state.py).
#pragma once
#include "../../include/hpf.h"

#include <cstdint>

namespace hpf_lazy {

enum { USERS = 0, ITEMS = 1 };

// what never changes on a handle
struct Config {
  bool hier = false, bias = false;
  bool jacobi = false;          // -novb with -bias and without -hier: the first item rate reads the start state's sum_u E[theta]
  bool several = false;         // n_ranks > 1
  bool rows[2] = {true, true};  // the side has rows (a rank may hold no users)
};

// what the caller knows about this moment
struct Now {
  int phase = 0;                // hpf_plan::next_phase: 0 = between iterations
  uint32_t iterations = 0;
  bool packed = false;          // the rows of W are p59: a sweep may report an entry it could not hold
  bool comm = false;            // the library owns the exchange (hpf_comm_init)
};

// A deferred job.  hpf_capi.hip has one executor per job; none of them decides whether it is due.
enum Job : uint8_t {
  RECOVER,                 // look at the device's flag word; a flushed entry: plain rows, W again, the skipped iterations
  REPORT,                  // fail on a softmax underflow the kernels flagged
  ES_USERS, ES_ITEMS,      // shape (prior added, in place) and E from the raw sums and the rate the last sweep used
  ELOG_USERS, ELOG_ITEMS,  // Elog from shape and that rate
  DERIVE_W,                // W from Elog of the sides w_due() names (a spread p59 cannot hold: RECOVER's repair, then again)
  COLUMN_SUMS,             // sum_i E[beta] for the first user sweep; jacobi: sum_u E[theta] for the first item rate
  DERIVED_DONE,            // the launches of the three above are checked: report derived()
  EXCHANGE_START_SUMS,     // jacobi on several ranks: the tail of the exchange buffer all-reduced (the library's communicator)
                           // or left to the caller: report start_sums_handed()
  N_JOBS
};

// what a call is about to read or overwrite
enum Need : uint8_t {
  FLAGS,           // nothing but the kernels' report (hpf_synchronize, hpf_snapshot_save, the end of a fold-in)
  SWEEP_VECTORS,   // what only the sweeps write: a rate's column sums, the xi / eta vectors, the exchange buffer, W's size
  BIAS_RATE,       // (side) the constant bias rate
  STATE_E,         // (side) S or E of a side, for export
  STATE_ELOG,      // (side) Elog of a side, for export
  PATCH,           // (side, kind) an array of kind k of theta / beta or of a bias column is about to be overwritten
  PATCH_VECTOR,    // a rate or a xi / eta vector is about to be overwritten
  OVERWRITE_ALL,   // a snapshot is about to replace the state
  SCORING,         // E of both sides, checked: a kernel scores pairs from it
  SCORES,          // E of both sides for the unfused ranking calls
  E_IS_SET,        // only the check that E of both sides exists (hpf_rank_queries with no query)
  FACTORS,         // (side) E of one side: hpf_similar, hpf_factor_top
  ELBO,            // S, E and Elog of both sides
  ELBO_FROM_W,     // ... and W
  ITERATION,       // everything an iteration reads
  DERIVED,         // (side = the frozen side whose xi / eta nobody reads, or -1) W and the start sums
  GATHER_PROBE,    // W as an iteration would read it
  START_SUMS,      // hpf_start_sums
  FOLD_FUSED,      // (side = the folded-in side) E and Elog of the other side; this side is overwritten
  FOLD_SWEEPS,     // (side) the same call through the training kernels: this side is overwritten ...
  FOLD_SWEEPS_RUN, // (side) ... and, once it holds the prior, W, the start sums and E of the other side
  FOLD_SWEEPS_END, // (side) S, E and Elog of the folded-in side from its last sweep
  BECAUSE,         // E and Elog of both sides, checked: hpf_because evaluates phi per pair from them
  MOMENTS,         // E and shape of both sides, checked: hpf_score_moments / hpf_recommend_ucb take Var = E^2 / shape from them
  N_NEEDS
};

struct Todo {
  int status = HPF_OK;           // not HPF_OK: the call returns it with `error`, and nothing has been run
  const char *error = nullptr;
  int n = 0;
  Job job[16];
};

// where W of a side comes from again after a fall-back to plain rows
enum Repair : uint8_t {
  REPAIR_NOTHING,          // no rows
  REPAIR_FROM_ELOG,        // derive_w at the next DERIVE_W (now pending)
  REPAIR_REPEAT_SWEEP,     // a W-only repeat of the side's last sweep; S holds that sweep's raw sums: the prior is added
  REPAIR_REPEAT_ON_SHAPE   // ... an export has turned S into the shape since: the same sum, not taken twice
};

// the snapshot's flag words (HPFSNAP4).  Bits 6 and 7 of a side word say which optional arrays follow: the caller's.
// Bits 9 .. 13 say what was handed in (or folded in) before the first sweep beyond E and Elog of the factors -- a shape, the
// bias column of E / Elog / the shape apart, the bias rate -- and bit 14 that the word says so at all: a blob written before
// these bits existed has none of them and loads as it always did (the bias columns as the factors', no shape, no bias rate).
enum : uint32_t {
  SNAP_HAVE_E = 1, SNAP_HAVE_L = 2, SNAP_HAVE_PRIOR = 4, SNAP_W_DIRTY = 8, SNAP_L_STALE = 16, SNAP_ES_STALE = 32,
  SNAP_RATE_SET = 64, SNAP_PRIOR_SHAPE_SET = 128, SNAP_W_FROM_SWEEP = 256,
  SNAP_HAVE_S = 512, SNAP_HAVE_BIAS_S = 1024, SNAP_HAVE_BIAS_E = 2048, SNAP_HAVE_BIAS_L = 4096, SNAP_BIAS_RATE_KNOWN = 8192,
  SNAP_SAYS_HANDED_IN = 16384,
  SNAP_SUMS_DIRTY = 1, SNAP_START_SUMS_DONE = 2
};
static_assert(SNAP_HAVE_E == 1u && SNAP_HAVE_L == 2u && SNAP_HAVE_PRIOR == 4u && SNAP_W_DIRTY == 8u && SNAP_L_STALE == 16u &&
              SNAP_ES_STALE == 32u && SNAP_RATE_SET == 64u && SNAP_PRIOR_SHAPE_SET == 128u && SNAP_W_FROM_SWEEP == 256u, "HPFSNAP4 side word");
static_assert(SNAP_HAVE_S == 512u && SNAP_HAVE_BIAS_S == 1024u && SNAP_HAVE_BIAS_E == 2048u && SNAP_HAVE_BIAS_L == 4096u &&
              SNAP_BIAS_RATE_KNOWN == 8192u && SNAP_SAYS_HANDED_IN == 16384u, "HPFSNAP4 side word: what was handed in");
static_assert(SNAP_SUMS_DIRTY == 1u && SNAP_START_SUMS_DONE == 2u, "HPFSNAP4 more_flags");

class State {
 public:
  State() = default;
  explicit State(const Config &c) : cfg(c) {}

  // ---- events ---------------------------------------------------------------------------------------------------------
  // hpf_set_state put an array in place.  obj: 0 theta, 1 beta, 2 xi, 3 eta, 4 user bias, 5 item bias (which / 4 of
  // hpf_state); kind: 0 shape, 1 rate, 2 E, 3 Elog.  A rate is kept for export only; of xi / eta the iteration reads E.
  void state_set(int obj, int kind)
  {
    Flags &s = side[obj & 1];
    if (obj == 2 || obj == 3) { if (kind == 2) s.have_prior = true; return; }
    if (kind == 1) return;
    if (obj <= 1) {
      if (kind == 0) s.have_S = true;
      if (kind == 2) s.have_E = true;
      if (kind == 3) s.have_L = true;
    } else {
      if (kind == 0) s.have_bias_S = true;
      if (kind == 2) s.have_bias_E = true;
      if (kind == 3) s.have_bias_L = true;
    }
    if (kind == 3) s.w_dirty = true;          // Elog of theta/beta or of a bias column
    if (kind != 0) derived_dirty = sums_dirty = true;
  }
  // a sweep of the side is on the stream: S holds raw sums, E and Elog predate it, W is the sweep's
  void swept(int sd) { Flags &s = side[sd]; s.l_stale = s.es_stale = s.w_from_sweep = true; }
  // derive_w wrote W of the side from its Elog
  void w_derived(int sd) { side[sd].w_dirty = side[sd].w_from_sweep = false; }
  // DERIVED_DONE.  jacobi on several ranks: the sums just taken are this rank's part only, until EXCHANGE_START_SUMS
  void derived()
  {
    if (cfg.jacobi && sums_dirty) start_sums_done = false;
    derived_dirty = sums_dirty = false;
  }
  // the folded-in side after the call: what hpf_set_state of every array of that side would leave behind
  void folded(int sd)
  {
    Flags &s = side[sd];
    s.have_E = s.have_L = s.have_S = true;            // a fold-in leaves shapes
    if (cfg.hier) s.have_prior = true;
    if (cfg.bias) s.have_bias_E = s.have_bias_L = s.have_bias_S = s.bias_rate_known = true;
    s.es_stale = s.l_stale = false;
    s.w_dirty = true; s.w_from_sweep = false;
    derived_dirty = sums_dirty = true;
  }
  // EXCHANGE_START_SUMS ran.  Without a communicator THIS RANK'S PART of the sum is in the tail for a caller that owns
  // the exchange; start_sums_pending() keeps reading true until the first pass of the next iteration, so that a caller may
  // look at it before or after hpf_start_sums
  void start_sums_handed(bool comm) { start_sums_done = true; tail_partial = !comm; }
  void iteration_begun() { tail_partial = false; }
  // The rows have become plain doubles after a sweep (or derive_w) met an entry p59 cannot hold.  W is written again by a
  // W-ONLY repeat of the side's last sweep (same S, the prior and the column sums that sweep used: the same arithmetic, so
  // the same bits a w_storage = 3 handle has) or by derive_w where W came from a handed-in Elog.  Only W is then pending:
  // the start sums in place -- on several ranks the all-reduced ones -- stay (sums_dirty is not raised)
  Repair fell_back(int sd)
  {
    Flags &s = side[sd];
    if (!cfg.rows[sd]) return REPAIR_NOTHING;
    if (!s.w_from_sweep || s.w_dirty) { s.w_dirty = true; derived_dirty = true; return REPAIR_FROM_ELOG; }
    return s.es_stale ? REPAIR_REPEAT_SWEEP : REPAIR_REPEAT_ON_SHAPE;
  }
  // an ES_* or ELOG_* job finished
  void refreshed(Job j)
  {
    if (j == ES_USERS || j == ES_ITEMS) side[j == ES_ITEMS].es_stale = false;
    if (j == ELOG_USERS || j == ELOG_ITEMS) side[j == ELOG_ITEMS].l_stale = false;
  }

  // ---- questions ------------------------------------------------------------------------------------------------------
  bool w_due(int sd) const { return cfg.rows[sd] && side[sd].w_dirty; }      // DERIVE_W's sides
  // hpf_work_info.start_sums_pending
  bool start_sums_pending() const { return cfg.jacobi && cfg.several && (sums_dirty || !start_sums_done || tail_partial); }

  // The jobs a call runs before it touches what it named, or the error it returns.  Changes nothing: a refused call leaves
  // every flag as it was.
  Todo ask(Need need, const Now &now, int sd = -1, int kind = -1) const
  {
    Plan p{*this, now};
    const bool fresh = now.iterations == 0;         // no sweep has run: what was not handed in does not exist
    const int oth = sd >= 0 ? 1 - sd : -1;
    switch (need) {
      case FLAGS: p.report(); break;
      // Between iterations only -- inside one the item side's S already holds the sums of the iteration in flight, not
      // those its last sweep read.  No REPORT: an underflow report is about E, and these exports never failed on it.
      case SWEEP_VECTORS: p.recover_if_idle(); break;
      case BIAS_RATE:
        if (fresh && !side[sd].bias_rate_known) return p.refuse("bias rate is defined after the first sweep");
        p.recover_if_idle();
        break;
      case STATE_E: p.report(); p.es(sd); break;
      case STATE_ELOG: p.report(); p.elog(sd); break;
      // A new state supersedes whatever the kernels flagged about the old one -- but iterations a flushed entry made the
      // passes skip are part of the old one: they are run first.  The rest of S / E must be current before patching.
      // Elog: the rest of L predates the last sweep, rebuild it before patching in the new part.  Shape: L is rebuilt from
      // S, and a shape handed in is not the sweep's -- an Elog exported later must not depend on whether one was exported before
      case PATCH:
        p.recover();
        if (kind == 3 || kind == 0) p.elog(sd); else p.es(sd);
        break;
      case PATCH_VECTOR: case OVERWRITE_ALL: p.recover(); break;
      case SCORING: case SCORES: case E_IS_SET:
        if (!(side[USERS].have_E && side[ITEMS].have_E) && fresh) return p.refuse("E state not set");
        if (need == SCORING) p.report();
        if (need != E_IS_SET) { p.es(USERS); p.es(ITEMS); }
        break;
      case FACTORS:
        if (!side[sd].have_E && fresh) return p.refuse("E state not set");
        p.report(); p.es(sd);
        break;
      case ELBO: case ELBO_FROM_W:
        p.elog(USERS); p.elog(ITEMS);
        if (need == ELBO_FROM_W) p.derive(-1);      // W follows a set_state(ELOG), if any
        break;
      case ITERATION: {
        // several ranks: a pass that skipped would leave this rank's sums out of the all-reduce, so the host looks at the
        // flag before every iteration (one stream synchronisation) and repairs the rows first; one rank lets the passes
        // skip and catches up at its next synchronisation point
        if (cfg.several && now.packed) p.recover();
        // (sums_dirty, not derived_dirty: a rank that only has to write its W again after a fall-back from the packed rows
        // keeps the all-reduced sums it holds and must not enter a collective the other ranks never issue)
        const bool exchange = cfg.jacobi && cfg.several && (sums_dirty || !start_sums_done);
        if (exchange && !now.comm)
          return p.refuse("-novb on several ranks: call hpf_start_sums and sum-all-reduce the last ld doubles of the exchange buffer before the first iteration");
        p.derive(-1);
        if (exchange) p.exchange_start_sums();
        break;
      }
      case DERIVED: p.derive(sd); break;
      case GATHER_PROBE: p.recover(); p.derive(-1); break;
      case START_SUMS: p.derive(-1); p.exchange_start_sums(); break;
      case FOLD_FUSED: case FOLD_SWEEPS:
        if (fresh && !(side[oth].have_E && side[oth].have_L))
          return p.refuse(sd == ITEMS ? "user side not set: hand in THETA_E and THETA_ELOG before folding in"
                                      : "item side not set: hand in BETA_E and BETA_ELOG before folding in");
        if (fresh && cfg.bias && !(side[oth].have_bias_E && side[oth].have_bias_L))
          return p.refuse(sd == ITEMS ? "user side not set: hand in UBIAS_E and UBIAS_ELOG before folding in (-bias)"
                                      : "item side not set: hand in IBIAS_E and IBIAS_ELOG before folding in (-bias)");
        if (!cfg.rows[sd]) break;                   // nothing to fold in
        // the folded-in state supersedes whatever the kernels flagged about the old one, like a state handed in
        p.recover();
        if (need == FOLD_FUSED) p.elog(oth);        // E and Elog of the frozen side as of its last sweep
        break;
      // the sums of the frozen side the sweep's rate reads: the item side's are COLUMN_SUMS'; the user side's own are the
      // product of a user sweep, so an item call takes them from E into a temporary
      case FOLD_SWEEPS_RUN: p.derive(oth); if (sd == ITEMS) p.es(oth); break;
      case FOLD_SWEEPS_END: p.elog(sd); break;
      case BECAUSE:
        if (fresh && !(side[USERS].have_E && side[USERS].have_L && side[ITEMS].have_E && side[ITEMS].have_L))
          return p.refuse("E and Elog state not set: hand in THETA_E, THETA_ELOG, BETA_E and BETA_ELOG, or iterate");
        if (fresh && cfg.bias && !(side[USERS].have_bias_E && side[USERS].have_bias_L && side[ITEMS].have_bias_E && side[ITEMS].have_bias_L))
          return p.refuse("E and Elog state not set: hand in E and ELOG of UBIAS and IBIAS (-bias), or iterate");
        p.report(); p.elog(USERS); p.elog(ITEMS);
        break;
      // after a sweep S is the shape once ES_* has run; before the first one only what was handed in (or folded in) exists
      case MOMENTS:
        if (fresh && !(side[USERS].have_E && side[USERS].have_S && side[ITEMS].have_E && side[ITEMS].have_S))
          return p.refuse("E and shape state not set: hand in THETA_E, THETA_SHAPE, BETA_E and BETA_SHAPE, or iterate");
        if (fresh && cfg.bias && !(side[USERS].have_bias_E && side[USERS].have_bias_S && side[ITEMS].have_bias_E && side[ITEMS].have_bias_S))
          return p.refuse("E and shape state not set: hand in E and SHAPE of UBIAS and IBIAS (-bias), or iterate");
        p.report(); p.es(USERS); p.es(ITEMS);
        break;
      case N_NEEDS: break;
    }
    if (p.overflow) return p.refuse("internal: too many deferred jobs");
    return p.todo;
  }

  // every flag in one word, for host/lazy_selftest.cpp to compare two handles by
  uint32_t fingerprint() const
  {
    uint32_t f = (derived_dirty ? 1u : 0u) | (sums_dirty ? 2u : 0u) | (start_sums_done ? 4u : 0u) | (tail_partial ? 8u : 0u);
    for (int k = 0; k < 2; ++k) {
      const Flags &s = side[k];
      const uint32_t w = (s.have_E ? 1u : 0u) | (s.have_L ? 2u : 0u) | (s.have_prior ? 4u : 0u) | (s.have_bias_E ? 8u : 0u) | (s.have_bias_L ? 16u : 0u) |
                         (s.bias_rate_known ? 32u : 0u) | (s.w_dirty ? 64u : 0u) | (s.w_from_sweep ? 128u : 0u) | (s.l_stale ? 256u : 0u) | (s.es_stale ? 512u : 0u) |
                         (s.have_S ? 1024u : 0u) | (s.have_bias_S ? 2048u : 0u);
      f |= w << (4 + 12 * k);
    }
    return f;
  }

  // ---- the snapshot's words -------------------------------------------------------------------------------------------
  uint32_t snap_side_word(int sd, bool rate_set, bool prior_shape_set) const
  {
    const Flags &s = side[sd];
    return (s.have_E ? SNAP_HAVE_E : 0u) | (s.have_L ? SNAP_HAVE_L : 0u) | (s.have_prior ? SNAP_HAVE_PRIOR : 0u) |
           (s.w_dirty ? SNAP_W_DIRTY : 0u) | (s.l_stale ? SNAP_L_STALE : 0u) | (s.es_stale ? SNAP_ES_STALE : 0u) |
           (rate_set ? SNAP_RATE_SET : 0u) | (prior_shape_set ? SNAP_PRIOR_SHAPE_SET : 0u) | (s.w_from_sweep ? SNAP_W_FROM_SWEEP : 0u) |
           (s.have_S ? SNAP_HAVE_S : 0u) | (s.have_bias_S ? SNAP_HAVE_BIAS_S : 0u) | (s.have_bias_E ? SNAP_HAVE_BIAS_E : 0u) |
           (s.have_bias_L ? SNAP_HAVE_BIAS_L : 0u) | (s.bias_rate_known ? SNAP_BIAS_RATE_KNOWN : 0u) | SNAP_SAYS_HANDED_IN;
  }
  uint32_t snap_derived_dirty() const { return derived_dirty ? 1u : 0u; }
  // (a handle whose W alone was pending must not come back as one whose start sums are pending -- on several ranks it
  // would enter a collective alone)
  uint32_t snap_more_flags() const { return (sums_dirty ? SNAP_SUMS_DIRTY : 0u) | (start_sums_done ? SNAP_START_SUMS_DONE : 0u); }
  // a snapshot has replaced the state
  void snapshot_loaded(const uint32_t side_words[2], uint32_t derived_word, uint32_t more_flags)
  {
    for (int k = 0; k < 2; ++k) {
      Flags &s = side[k]; const uint32_t f = side_words[k];
      s.have_E = f & SNAP_HAVE_E; s.have_L = f & SNAP_HAVE_L; s.have_prior = f & SNAP_HAVE_PRIOR; s.w_dirty = f & SNAP_W_DIRTY;
      s.l_stale = f & SNAP_L_STALE; s.es_stale = f & SNAP_ES_STALE; s.w_from_sweep = f & SNAP_W_FROM_SWEEP;
      // The arrays came with the blob, S among them: what was handed in before the first sweep is still there, and a restored
      // handle answers what the old one answered.  A blob from before the word said so: the whole rows count as the factors'
      // columns do, and the shapes have to be handed in again
      if (f & SNAP_SAYS_HANDED_IN) {
        s.have_S = f & SNAP_HAVE_S; s.have_bias_S = f & SNAP_HAVE_BIAS_S; s.have_bias_E = f & SNAP_HAVE_BIAS_E;
        s.have_bias_L = f & SNAP_HAVE_BIAS_L; s.bias_rate_known = f & SNAP_BIAS_RATE_KNOWN;
      } else {
        s.have_bias_E = s.have_E; s.have_bias_L = s.have_L;
        s.have_S = s.have_bias_S = false;
        s.bias_rate_known = false;
      }
    }
    derived_dirty = derived_word != 0;
    sums_dirty = (more_flags & SNAP_SUMS_DIRTY) != 0;
    start_sums_done = (more_flags & SNAP_START_SUMS_DONE) != 0;      // the tail of the exchange buffer came with the snapshot
  }

 private:
  struct Flags {
    bool have_E = false, have_L = false, have_prior = false;
    bool have_bias_E = false, have_bias_L = false;   // the bias column of E / L was handed in (a fold-in asks for the other side's)
    bool have_S = false, have_bias_S = false;        // a shape was handed in or folded in (MOMENTS asks for it before the first sweep)
    bool bias_rate_known = false;   // a fold-in left the bias at rate r_prior + bias_rate_add (readable before the first sweep)
    bool w_dirty = false;           // L was handed in by hpf_set_state: W must be derived from it
    bool w_from_sweep = false;      // W was written by a sweep (a W-only repeat of it restores it), not derived from Elog
    bool l_stale = false;           // a sweep ran since L was last valid: rebuild L on export
    bool es_stale = false;          // S holds raw phi sums and E predates the last sweep
  };

  // the list under construction
  struct Plan {
    const State &st; const Now &now;
    Todo todo;
    bool recovered = false, overflow = false;
    bool es_listed[2] = {false, false}, elog_listed[2] = {false, false};
    void push(Job j) { if (todo.status) return; if (todo.n <(int)(sizeof todo.job / sizeof todo.job[0])) todo.job[todo.n++] = j; else overflow = true; }
    Todo refuse(const char *msg) { Todo t; t.status = HPF_ERR_STATE; t.error = msg; return t; }
    // once per list: nothing after it raises the flag again, but DERIVE_W
    void recover() { if (!recovered) push(RECOVER); recovered = true; }
    void recover_if_idle() { if (now.phase == 0) recover(); }
    void report() { recover(); push(REPORT); }
    // a repeat of the last sweep needs S as the pass left it: no refresh while a fall-back is due
    void es(int sd)
    {
      if (!st.side[sd].es_stale || es_listed[sd]) return;
      if (st.cfg.rows[sd]) recover();
      push(sd ? ES_ITEMS : ES_USERS); es_listed[sd] = true;
    }
    void elog(int sd)
    {
      es(sd);
      if (!st.side[sd].l_stale || elog_listed[sd]) return;
      push(sd ? ELOG_ITEMS : ELOG_USERS); elog_listed[sd] = true;
    }
    // W and the start sums; frozen: the side whose xi / eta is not read (a fold-in through the training kernels)
    void derive(int frozen)
    {
      if (!st.derived_dirty) return;
      const Flags &u = st.side[USERS], &it = st.side[ITEMS];
      const char *err = nullptr;
      if (!(u.have_L && it.have_L && it.have_E)) err = "state not initialised: set THETA_ELOG, BETA_ELOG and BETA_E before iterating";
      else if (st.cfg.hier && !((u.have_prior || frozen == USERS) && (it.have_prior || frozen == ITEMS))) err = "state not initialised: set XI_E and ETA_E (-hier)";
      else if (st.cfg.jacobi && st.sums_dirty && !u.have_E) err = "state not initialised: -novb needs THETA_E (the first item rate is built from it)";
      if (err) { todo = refuse(err); return; }
      push(DERIVE_W); recovered = false;
      if (st.sums_dirty) {                           // c[k] = sum_i E[beta_ik]: consumed by the first user sweep
        es(ITEMS);
        if (st.cfg.jacobi) es(USERS);                // sum_u E[theta] of the start state: the first item rate uses it
        push(COLUMN_SUMS);
      }
      push(DERIVED_DONE);
    }
    void exchange_start_sums()
    {
      if (todo.status || !st.cfg.jacobi || !st.cfg.several) return;
      const bool part_only = st.derived_dirty && st.sums_dirty;      // derived() will have said so by then
      if (part_only || !st.start_sums_done) push(EXCHANGE_START_SUMS);
    }
  };

  Config cfg;
  Flags side[2];
  bool derived_dirty = true;
  bool sums_dirty = true;          // a state array was handed in since the start state's column sums were taken: COLUMN_SUMS
                                   // takes them again.  derived_dirty without it = only W has to be written again (fell_back):
                                   // the sums in place -- on several ranks the all-reduced ones -- stay
  bool start_sums_done = false;    // jacobi on several ranks: the start state's sum_u E[theta] has been handed to the exchange
  bool tail_partial = false;       // see start_sums_handed
};

}  // namespace hpf_lazy
