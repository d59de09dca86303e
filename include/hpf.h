/*
 * hpf.h -- C-ABI of libhpf_hip.so: the MI355X (gfx950) device side of the
 * hgaprec CAVI inner loop (hierarchical / Bayesian Poisson factorization).
 *
 * The reference (premgopalan/hgaprec) is one C++ executable with no plugin or
 * FFI seam; this ABI is the seam a maintainer would cut where the inference
 * driver (src/hgaprec.cc, class HGAPRec) meets the Gamma containers
 * (src/gpbase.hh) and the ratings store (src/ratings.hh).  Each entry point
 * names the reference code it replaces (file:line, relative to the reference's
 * src/).  INTEGRATION.md shows the reference-side patch.
 *
 * Conventions
 *  - plain C types only; the caller owns every host pointer and may free it
 *    as soon as the call returns; the handle owns all device memory.
 *  - every function returns HPF_OK (0) or a negative hpf_status and never
 *    throws or aborts; hpf_last_error(h) gives the text of the last failure.
 *  - one host thread per handle; distinct handles are independent.
 *  - all real-valued state is fp64, like the reference (env.hh / gpbase.hh use
 *    double throughout); ids are uint32, ratings uint8 (yval_t, env.hh:20).
 *  - multi-GPU: one handle per rank holding a contiguous range of users (and
 *    their nonzeros); item-side state is replicated.  The only exchange per
 *    iteration is a sum-all-reduce of hpf_exchange_buffer() between
 *    hpf_iterate_local() and hpf_iterate_global().
 */
#ifndef HPF_H
#define HPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HPF_ABI_VERSION 8

typedef struct hpf_handle hpf_handle;

typedef enum {
  HPF_OK = 0,
  HPF_ERR_INVALID = -1,      /* bad argument / call order                    */
  HPF_ERR_NO_DEVICE = -2,    /* no usable gfx950 device / HIP runtime error   */
  HPF_ERR_OOM = -3,          /* device or host allocation failed              */
  HPF_ERR_HIP = -4,          /* a HIP call or kernel launch failed            */
  HPF_ERR_UNSUPPORTED = -5,  /* e.g. K + 2*bias > HPF_MAX_COLUMNS             */
  HPF_ERR_STATE = -6         /* state not initialised (no CSR / no E, Elog)   */
} hpf_status;

#define HPF_MAX_COLUMNS 1024

/* Gamma objects of the model (HGAPRec members, hgaprec.hh:94-112) x the four
 * per-object arrays of gpbase.hh (shape_curr, rate_curr, expected_v,
 * expected_logv).  Host layout is dense row-major doubles:
 *   THETA_* : n_users x K   (htheta, or theta without -hier)
 *   BETA_*  : n_items x K   (hbeta / beta)
 *   XI_*    : n_users       (thetarate; -hier only)
 *   ETA_*   : n_items       (betarate;  -hier only)
 *   UBIAS_* : n_users       (thetabias; -bias only)
 *   IBIAS_* : n_items       (betabias;  -bias only)
 * Without -hier, THETA_RATE / BETA_RATE are K-vectors (GPMatrixGR::_rcurr,
 * gpbase.hh:520). */
typedef enum {
  HPF_THETA_SHAPE = 0, HPF_THETA_RATE, HPF_THETA_E, HPF_THETA_ELOG,
  HPF_BETA_SHAPE, HPF_BETA_RATE, HPF_BETA_E, HPF_BETA_ELOG,
  HPF_XI_SHAPE, HPF_XI_RATE, HPF_XI_E, HPF_XI_ELOG,
  HPF_ETA_SHAPE, HPF_ETA_RATE, HPF_ETA_E, HPF_ETA_ELOG,
  HPF_UBIAS_SHAPE, HPF_UBIAS_RATE, HPF_UBIAS_E, HPF_UBIAS_ELOG,
  HPF_IBIAS_SHAPE, HPF_IBIAS_RATE, HPF_IBIAS_E, HPF_IBIAS_ELOG,
  HPF_NUM_STATE
} hpf_state;

typedef struct {
  uint32_t struct_size;    /* sizeof(hpf_config), for ABI growth             */
  uint32_t n_users;        /* users owned by THIS handle (its shard)         */
  uint32_t n_items;        /* all items (replicated)                         */
  uint32_t K;              /* factors (-k)                                   */
  uint32_t hier;           /* -hier : vb_hier()  else vb() / vb_bias()       */
  uint32_t bias;           /* -bias                                          */
  uint32_t binary;         /* -binary-data (held-out likelihood form)        */
  uint32_t n_users_total;  /* users over all ranks (item-bias rate 0.3 + n,  */
                           /* hgaprec.cc:1393); 0 => n_users                 */
  int32_t  device;         /* HIP device ordinal                             */
  uint32_t n_ranks;        /* 1 => hpf_iterate() needs no exchange           */
  uint32_t rank;
  uint32_t w_storage;      /* how W = exp(Elog - rowmax), the matrix the phi      */
                           /* passes gather, is stored (arithmetic and             */
                           /* accumulators are fp64 in every mode):                */
                           /* 0: fp64, exact (default; the only mode chosen        */
                           /*    implicitly).  The library may PACK the rows       */
                           /*    losslessly (59 bits per element: every W is a     */
                           /*    positive double in [2^-126, 2) or zero, so the    */
                           /*    sign and four exponent bits carry nothing) when   */
                           /*    that saves a 128-byte line per row -- K = 100:    */
                           /*    six lines instead of seven.  A W below 2^-126 of  */
                           /*    its row maximum (Elog spread > 88 inside a row;   */
                           /*    HPF states have 10-20) cannot be packed: the      */
                           /*    library then moves the rows to plain doubles by   */
                           /*    itself and goes on with the bits a handle made    */
                           /*    with 3 has (hpf_work_info.w_fallbacks).           */
                           /* 3: fp64 as plain doubles, never packed (where 0      */
                           /*    would pack: in the packed shape's pieces).        */
                           /* 1: EXPERIMENTAL fp32 -- drifts out of the 1e-4       */
                           /*    parity contract after ~30 iterations. */
                           /* 2: OPT-IN 48 bits: the top 48 bits of the fp64 value */
                           /*    (36 mantissa bits, rounded to nearest even); rows */
                           /*    are 25-30 % shorter, both phi passes faster by    */
                           /*    about that; measured drift vs the fp64 oracle     */
                           /*    ~1e-11 per early sweep, inside 1e-4 after         */
                           /*    hundreds (tests/w32_error_growth.py).             */
  void    *stream;         /* hipStream_t to run on, NULL => own stream      */
  double   s_prior;        /* 0.3 (hgaprec.cc:13-20 hard-codes both)         */
  double   r_prior;        /* 0.3                                            */
  uint32_t novb;           /* -novb (Env::vb == false).  Read only where the  */
                           /* reference reads it: vb_bias(), i.e. bias without */
                           /* hier (hgaprec.cc:1250,1276-1297) -- both rates   */
                           /* are then built from the PREVIOUS iteration's     */
                           /* expectations before anything is swapped (the     */
                           /* item rate takes the old sum_u E[theta]).  On     */
                           /* several ranks see hpf_start_sums.                */
  uint32_t tiling;         /* 0: the library decides per side whether the phi  */
                           /* pass is tiled (cache blocking of the gathered    */
                           /* rows, one tile per XCD L2) */
                           /* 1: never -- row-major work lists only.  Tiling   */
                           /* changes the ORDER in which a row's nonzeros are  */
                           /* summed (same for every run of one build), not    */
                           /* what is summed.                                  */
} hpf_config;

/* per-kernel device time, milliseconds, from hipEvents recorded on the
 * handle's stream around each launch group */
typedef struct {
  float phi_user_ms;     /* K1a: phi_pass_kernel<..,0>, user-major (theta sums) */
  float combine_user_ms; /*      combine of long user rows                      */
  float phi_item_ms;     /* K1b: phi_pass_kernel<..,1>, item-major (beta sums)  */
  float combine_item_ms; /*      combine of long item rows                      */
  float sweep_user_ms;   /* K2 + K4(xi) + K5(user bias) + K7                    */
  float sweep_item_ms;   /* K3 + K4(eta) + K5(item bias) + K7                   */
  float iteration_ms;    /* first launch -> last launch of the iteration        */
  uint32_t iterations;   /* iterations executed so far                          */
  float exchange_wait_ms;/* end of the user sweep -> start of the item sweep:   */
                         /* the part of the all-reduce the stream had to wait   */
                         /* for (n_ranks > 1; ~0 on one rank)                   */
} hpf_timing;

int  hpf_abi_version(void);
const char *hpf_strerror(int status);
const char *hpf_last_error(const hpf_handle *h);

/* replaces: HGAPRec::HGAPRec allocation of the 8 Gamma objects
 * (hgaprec.cc:8-33) */
int  hpf_create(const hpf_config *cfg, hpf_handle **out);
void hpf_destroy(hpf_handle *h);

/* replaces: the per-user adjacency + rating maps built by
 * Ratings::read_generic (ratings.cc:63-119) and walked by
 * Ratings::get_movies / Ratings::r (ratings.hh:175-181,153-165).
 * CSR over this handle's users in the reference's visiting order; col = item
 * seq id; val = rating as stored by the reference (uint8, already wrapped,
 * last duplicate wins), NULL => every rating is 1 (-binary-data).
 * Host pointers (staged through pinned buffers).  The item-major (CSC) view is
 * built in HBM by a stable radix sort on the item id: inside an item the users
 * stay ascending -- the order in which the reference's serial loop
 * (hgaprec.cc:1340-1345) reaches them. */
int  hpf_upload_csr(hpf_handle *h, const int64_t *rowptr, const uint32_t *col,
                    const uint8_t *val);
/* the same for a CSR that already lives in HBM (DEVICE pointers on the handle's
 * device; the library copies what it keeps, the caller may free on return).
 * The producer's work must have completed before the call. */
int  hpf_upload_csr_device(hpf_handle *h, const int64_t *d_rowptr, const uint32_t *d_col,
                           const uint8_t *d_val);
/* replaces: the per-item user lists Ratings keeps beside the per-user ones
 * (Ratings::get_users, ratings.hh:167-173): host copies of the item-major view
 * (colptr[n_items + 1], users[nnz] ascending inside an item, vals[nnz]); any
 * pointer may be NULL. */
int  hpf_get_csc(hpf_handle *h, int64_t *colptr, uint32_t *users, uint8_t *vals);

/* replaces: the result of HGAPRec::initialize (hgaprec.cc:153-204) -- the host
 * draws the MT19937 stream and hands over E / Elog (and shapes, for export).
 * count must equal the element count of that array.
 * A refused call (a wrong count, a state that is not part of the model) and the bias-rate set, which is accepted and
 * ignored, leave the handle untouched: the model, what is pending and a report of an underflow not yet delivered. */
int  hpf_set_state(hpf_handle *h, hpf_state which, const double *host, size_t count);
/* replaces: reads of shape_curr()/rate_curr()/expected_v()/expected_logv()
 * by save_model (hgaprec.cc:2137-2158).
 * Every export, between iterations, is of the last iteration hpf_iterate returned for, whatever was exported before. */
int  hpf_get_state(hpf_handle *h, hpf_state which, double *host, size_t count);
/* the same with DEVICE pointers (dense row-major doubles in HBM, same element
 * counts): no PCIe round trip for callers whose state is already resident */
int  hpf_set_state_device(hpf_handle *h, hpf_state which, const double *dev, size_t count);
int  hpf_get_state_device(hpf_handle *h, hpf_state which, double *dev, size_t count);

/* Snapshot (extension; the reference has no training resume: `-load` is parsed
 * and never consulted, main.cc:137-140): the loop's whole device state as one
 * opaque host blob -- the gathered matrices W, raw sums, expectations, xi/eta
 * vectors, column sums and the bookkeeping flags, verbatim.  A handle of the same
 * shape that loads it continues with IDENTICAL bits (hpf_set_state(ELOG) would
 * re-derive W and round differently).  Call between iterations. */
int  hpf_snapshot_size(hpf_handle *h, size_t *bytes);
int  hpf_snapshot_save(hpf_handle *h, void *host, size_t bytes);
int  hpf_snapshot_load(hpf_handle *h, const void *host, size_t bytes);

/* replaces: n_iters passes of steps A-F of HGAPRec::vb_hier
 * (hgaprec.cc:1340-1414), or of vb (927-956) / vb_bias (1226-1272) without
 * -hier.  With n_ranks > 1 it needs hpf_comm_init and runs the overlapped
 * exchange (see below) itself; every rank must make the same call.
 * Asynchronous on the handle's stream.
 * If a sweep meets an element the packed rows of W cannot hold (hpf_config.w_storage),
 * the passes launched after it return at once; the next synchronising call moves the rows
 * to plain doubles and runs what was skipped (hpf_work_info.w_fallbacks) -- results are
 * those of a handle that never packed, only the timing of that call is not representative.
 * Launch-bound problems (nnz <= 4 Mi, or HPF_GRAPH=1; HPF_GRAPH=0 disables)
 * replay one captured iteration as a hipGraph: same kernels in the same
 * order, identical bits; such iterations report only iteration_ms in
 * hpf_timing (the per-kernel fields read 0).  With n_ranks > 1 (or a communicator)
 * the iteration is cut by its collectives; HPF_GRAPH=1 (experimental, opt-in: measured, it does
 * not pay) replays it as THREE graphs -- item pass | user pass + user sweep | item sweep --
 * (v8; hpf_work_info.graph_replay = 2). */
int  hpf_iterate(hpf_handle *h, int n_iters);

/* n_ranks > 1: step A for the local users, the local user sweep (B, D-user,
 * E) and the local partial sums ... */
int  hpf_iterate_local(hpf_handle *h);
/* hpf_iterate_local in pieces, for callers that overlap communication.  Step A
 * is two independent passes over the same W: the item-major one runs first.
 *   _items : item phi pass -- after it the first n_items*ld doubles of the
 *            exchange buffer (the item shape sums) are final and their
 *            all-reduce may start;
 *   _users : user phi pass + user sweep (B, D-user, E); only writes the last
 *            ld doubles (sum_u E[theta_u,:]), reduced in a second, tiny
 *            all-reduce.  (_phi = _items + the user phi pass, _sweep = the
 *            user sweep alone: the same work cut after step A instead.)
 * Order per iteration: _items, _users (or _phi, _sweep), hpf_iterate_global;
 * anything else returns HPF_ERR_STATE. */
int  hpf_iterate_local_items(hpf_handle *h);
int  hpf_iterate_local_users(hpf_handle *h);
int  hpf_iterate_local_phi(hpf_handle *h);
int  hpf_iterate_local_sweep(hpf_handle *h);
/* ... the caller sum-all-reduces this device buffer of `count` doubles in
 * place (RCCL ncclAllReduce(ncclDouble, ncclSum) / torch.distributed) on the
 * handle's stream ... */
int  hpf_exchange_buffer(hpf_handle *h, void **device_ptr, size_t *count);
/* optional: make the handle use caller-owned device memory (>= count doubles,
 * 16-byte aligned) as the exchange buffer; call before hpf_upload_csr.  The
 * buffer is cleared on the handle's stream: no work queued on another stream
 * may still be using that memory (a caching allocator can hand out a block
 * that earlier kernels of ITS stream are not done with). */
int  hpf_bind_exchange_buffer(hpf_handle *h, void *device_ptr, size_t count);
/* ... then the replicated item sweep (C, D-item, F) on every rank. */
int  hpf_iterate_global(hpf_handle *h);
/* -novb (hpf_config.novb with bias, without hier) on SEVERAL ranks: the first item rate is built
 * from sum_u E[theta_u,:] of the START state (hgaprec.cc:1281-1282 reads _theta.sum_rows() before
 * _theta.swap()), which then has to be summed over the ranks once, before the first iteration.
 * hpf_start_sums derives what the first iteration needs from the state handed in and leaves this
 * rank's part of that sum in the tail of the exchange buffer (its last `ld` doubles,
 * hpf_work_info.ld).  With hpf_comm_init done it also all-reduces the tail itself (and hpf_iterate
 * calls it on its own); otherwise the caller sum-all-reduces those ld doubles in place, like the
 * per-iteration exchange -- but ONLY when hpf_work_info.start_sums_pending reads 1: after
 * hpf_snapshot_load the tail is the reduced sum already (v7).  From v8 on the field may be read before OR after the call:
 * it keeps reading 1 while the tail holds this rank's part only, until the first pass of the next iteration.  Call it after the last hpf_set_state /
 * hpf_snapshot_load and before the first hpf_iterate_local_*: iterating without it returns
 * HPF_ERR_STATE.  A no-op elsewhere. */
int  hpf_start_sums(hpf_handle *h);

/* The library can run that all-reduce itself: RCCL is dlopen'ed on first use
 * (no link-time dependency).  One rank calls hpf_comm_unique_id and ships the
 * HPF_COMM_ID_BYTES bytes to the others by any means; every rank then calls
 * hpf_comm_init (collective) once, and hpf_allreduce_exchange between
 * iterate_local and iterate_global.  = ncclGetUniqueId / ncclCommInitRank /
 * ncclAllReduce(ncclDouble, ncclSum) in place on the handle's stream.
 * Overlapped form: hpf_iterate_local_items, hpf_allreduce_items_begin (the
 * item part goes out on a second, library-owned stream), hpf_iterate_local_users
 * (runs meanwhile), hpf_allreduce_exchange (adds the tail and makes the
 * handle's stream wait for both), hpf_iterate_global. */
#define HPF_COMM_ID_BYTES 128
int  hpf_comm_unique_id(void *id_out);
int  hpf_comm_init(hpf_handle *h, const void *id);
int  hpf_allreduce_items_begin(hpf_handle *h);
int  hpf_allreduce_exchange(hpf_handle *h);
/* host copies of the exchange buffer (host-staged reduction, tests) */
int  hpf_exchange_read(hpf_handle *h, double *host, size_t count);
int  hpf_exchange_write(hpf_handle *h, const double *host, size_t count);

/* replaces: the per-pair loop of HGAPRec::compute_likelihood
 * (hgaprec.cc:1455-1465) with rating_likelihood_hier / rating_likelihood
 * (1538-1560 / 1503-1536).  u is a LOCAL user index, y the int stored in the
 * CountMap (wrapped to uint8 like `yval_t r = i->second`).  Pairs are summed
 * in the order given (the caller passes them sorted by (user, item) like the
 * std::map).  Synchronous. */
int  hpf_heldout_ll(hpf_handle *h, const uint32_t *u, const uint32_t *i,
                    const int32_t *y, size_t cnt, double *sum_out,
                    uint64_t *cnt_out);
/* ABI v8.  A report step evaluates the same validation and test pairs every time (hgaprec.cc:1439-1470 walks the same
 * two maps): hpf_heldout_bind validates and uploads a set ONCE into one of HPF_HELDOUT_SLOTS slots (binding again
 * replaces it; cnt = 0 binds an empty set); hpf_heldout_ll_bound is then the kernel, one DMA of the per-pair values
 * into a page-locked buffer the handle keeps, and the same serial sum in the order the pairs were bound -- the value
 * hpf_heldout_ll returns for the same pairs, bit for bit.  The caller's arrays may be freed after the bind. */
#define HPF_HELDOUT_SLOTS 4
int  hpf_heldout_bind(hpf_handle *h, int slot, const uint32_t *u, const uint32_t *i, const int32_t *y, size_t cnt);
int  hpf_heldout_ll_bound(hpf_handle *h, int slot, double *sum_out, uint64_t *cnt_out);

/* replaces: HGAPRec::logl (hgaprec.cc:2160-2255), the bound written to
 * logl.txt with -logl: the per-nonzero term over this handle's nonzeros plus
 * the Gamma terms (gpbase.hh:360-387,717-741,951-969) of the user-side
 * objects and -- on rank 0 only -- of the replicated item-side objects, so
 * that the sum over ranks is the reference's value.  Needs >= 1 iteration.
 * Synchronous. */
int  hpf_elbo(hpf_handle *h, double *out);

/* ---- ranking evaluation (report steps) ------------------ */
/* DOMAIN of every ranking call below (hpf_rank_topn, hpf_item_ranks, hpf_loo_ranks,
 * hpf_rank_queries): "score descending" is defined for expectations E (theta, beta and both
 * biases) that are finite and >= +0.0, as every Gamma expectation is.  The kernels order scores
 * by their 64-bit pattern, which is the order of the values on that domain only: a negative
 * score, a NaN or an infinity would sort in FRONT of every proper score.  hpf_set_state does not
 * scan what it is handed; the model reader of the CLI refuses such a file (hgaprec_host.cpp,
 * load_matrix).  A masked item counts as +0.0 and ties with every other zero score by item. */
/* replaces: prediction_score_hier / prediction_score (hgaprec.cc:1966-1991,
 * 1850-1877; _use_rate_as_score) for every item: out[n_sel x n_items] =
 * E_theta[users] . E_beta^T (+ biases), on the fp64 matrix cores.  Host out. */
int  hpf_scores(hpf_handle *h, const uint32_t *users, uint32_t n_sel, double *out);
/* replaces: the scoring loop, qsort and top-N walk input of
 * HGAPRec::compute_precision (hgaprec.cc:1722-1765): per selected (local)
 * user the topn best items in the reference's order -- score descending, ties
 * by ascending item (glibc's stable qsort) -- after zeroing the user's
 * training items with a stored rating > 0 and the items of the caller's mask
 * list (CSR over the selected users; the validation items).  topn <= 1024;
 * entries beyond n_items are (0xffffffff, 0). */
int  hpf_rank_topn(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                   const uint64_t *mask_ptr, const uint32_t *mask_items, uint32_t topn,
                   uint32_t *out_items, double *out_scores);
/* replaces: the position j of a test item in the fully sorted list of
 * HGAPRec::compute_itemrank (hgaprec.cc:1628-1680): query q asks for item
 * q_item[q] in the list of selected user q_sel[q] (an index into users). */
int  hpf_item_ranks(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                    const uint64_t *mask_ptr, const uint32_t *mask_items,
                    const uint32_t *q_sel, const uint32_t *q_item, uint32_t nq,
                    uint32_t *out_rank, double *out_score);

/* ---- scoring a saved model (v8 additions: new functions only, no struct changed) ---- */
/* replaces: prediction_score_hier / prediction_score (hgaprec.cc:1966-1991, 1850-1877;
 * _use_rate_as_score) for a list of pairs: out[p] = E_theta[u[p]] . E_beta[i[p]]
 * (+ E_ubias[u[p]] + E_ibias[i[p]]).  u is a LOCAL user index.  Needs E on both sides
 * (hpf_set_state(*_E) or an iteration) and no CSR.  An index out of range is
 * HPF_ERR_INVALID before anything is launched; cnt = 0 is HPF_OK.  Synchronous. */
int  hpf_predict(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, double *out);
/* replaces: the scoring loop, qsort and walk of HGAPRec::gen_msr_csv (hgaprec.cc:2024-2055):
 * for selected user b, where item t = q_item[b] stands among the items [0, item_limit)
 * (0 => n_items) under score descending, item ascending -- scores as hpf_scores gives them,
 * replaced by +0.0 for the user's training items with a stored rating > 0 (all of them when the
 * handle has no values) and for the items of the mask list (CSR over the selected users), like
 * hpf_rank_topn.  out_rank[b] counts the items i != t below item_limit that come before t,
 * out_score[b] = s(b, t), out_masked[b] (may be NULL) the DISTINCT masked items below
 * item_limit.  t >= item_limit gives rank 0 and score 0.0 (the reference's loop never scores
 * item m - 1 and leaves rank = 0); t >= n_items is HPF_ERR_INVALID.
 * With item_limit = 0, out_rank and out_score equal, bit for bit, what hpf_item_ranks returns
 * for q_sel = 0 .. n_sel - 1 on the same handle: the scores come out of the same MFMA chain.
 * No n_sel x n_items array exists anywhere: a tile of scores is compared and counted in
 * registers; the masked items are one BIT per (user, item) for a batch of users at a time
 * (<= 256 MB; HPF_LOO_BATCH=<users> makes the batches smaller -- a test knob, read when the
 * handle is created). */
int  hpf_loo_ranks(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                   const uint64_t *mask_ptr, const uint32_t *mask_items,
                   const uint32_t *q_item, uint32_t item_limit,
                   uint32_t *out_rank, double *out_score, uint32_t *out_masked);
/* replaces: the position j of EVERY test item of a user in the fully sorted list of
 * HGAPRec::compute_itemrank (hgaprec.cc:1628-1680), for any number of users, without a score
 * matrix.  Queries are a CSR over the selected users: selected user b asks for items
 * q_items[q_ptr[b] .. q_ptr[b+1]).  out_rank[q] / out_score[q] (q indexes q_items) equal, bit for
 * bit, what hpf_item_ranks returns for the same users, masks and the expanded (q_sel, q_item)
 * list.  A user may have no query; an item may be asked for twice.  The queried item itself is
 * not counted, the user's other queried items are.  The user's row of scores is computed ONCE
 * (hpf_loo_ranks with one entry per pair computes it once per pair); internally a user's queries
 * go through in rows of at most 32 (RQ_QCAP in hpf_kernels.hpp).  q_ptr[0] != 0, a decreasing
 * q_ptr, an item >= n_items or a user out of range is HPF_ERR_INVALID before anything is
 * launched; n_sel = 0 or no query is HPF_OK.  At most 2^32 - 1 queries per call.  Device memory
 * beyond inputs and outputs: the bit rows of a batch of users (<= 256 MB, HPF_LOO_BATCH as for
 * hpf_loo_ranks) and 16 bytes per query + 12 per row. */
int  hpf_rank_queries(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                      const uint64_t *mask_ptr, const uint32_t *mask_items,
                      const uint64_t *q_ptr, const uint32_t *q_items,
                      uint32_t *out_rank, double *out_score);
/* replaces: the scoring loop, qsort and top-N walk input of HGAPRec::compute_precision
 * (hgaprec.cc:1722-1765) for ANY number of users -- the list of recommended items of each --
 * without a score matrix.  Arguments, domain, masking, order, padding and error cases are
 * hpf_rank_topn's: topn = 0 or > 1024, a user or a mask item out of range, mask_ptr[0] != 0 or a
 * decreasing mask_ptr is HPF_ERR_INVALID before anything is launched; n_sel = 0 is HPF_OK.
 * out_items and out_scores equal, bit for bit, what hpf_rank_topn returns for the same arguments:
 * the scores come out of the same MFMA chain, and the top-N of a total order (score descending,
 * item ascending) does not depend on how it is found.
 * topn <= 256: one sweep over the items per batch of users; a score that can still be among a
 * user's best topn is appended to a candidate buffer, which is sorted and cut back to topn whenever
 * it fills up; a second kernel merges the buffers of a user.  Device memory beyond inputs and
 * outputs: the bit rows of a batch of users (<= 256 MB, HPF_LOO_BATCH as for hpf_loo_ranks) and its
 * candidate buffers, 12 bytes x 2 pow2(max(topn, 64)) per user and split of the item range
 * (<= 512 MB: the batch shrinks until they fit; 10^5 items, topn = 100: 21 440 users x 4 splits x
 * 256 entries = 263 MB).  Nothing of size n_sel x n_items exists.  An odd row stride is
 * HPF_ERR_UNSUPPORTED, as for the other fused calls.
 * 256 < topn <= 1024: the call runs hpf_rank_topn's route (scores of a batch of users in memory). */
int  hpf_recommend(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                   const uint64_t *mask_ptr, const uint32_t *mask_items, uint32_t topn,
                   uint32_t *out_items, double *out_scores);

/* (an extension; the reference has no counterpart.)  Nearest neighbours in factor space: for selected row ids[b] of one
 * side -- 0: the rows of E[theta] of this handle's users (with several ranks the LOCAL users only; nothing is
 * exchanged), 1: the rows of E[beta] -- the topn OTHER rows of the same side, by score descending, ties by ascending id:
 * the ranking calls' one ordering rule, taken on the bit pattern of the computed fp64 score.  The score is taken over
 * the K factor columns only; bias columns take no part.
 *   HPF_SIM_DOT     s(a, b) = sum_k E_ak E_bk, out of the same MFMA chain as hpf_scores (bit for bit what hpf_scores
 *                   returns on a handle whose E[theta] and E[beta] are both this matrix, without bias).
 *   HPF_SIM_COSINE  the same chain over the rows at unit length, U_ak = x_k / sqrt(sum_k x_k^2) with x_k = E_ak 2^-e and
 *                   2^e the power of two of the row's largest entry: no square and no sum overflows, and a row scaled by
 *                   a power of two has the same U bit for bit; sqrt and the division are correctly rounded, the sum is
 *                   taken in an order fixed by K (run to run the same bits).  |U_ak - exact| <= (K/2 + 3) 2^-53 exact,
 *                   and a returned cosine is within (2K + 8) 2^-53 of the exact one.  An all-zero row is all-zero in U:
 *                   its cosine with every row is +0.0, never NaN.
 * The row itself is never in its own list -- left out, not counted as +0.0.  Another row with identical factors is
 * listed, with the score it gets.  An id may be selected twice; both output rows are then equal.  Entries beyond
 * rows - 1 are (0xffffffff, 0.0), as in hpf_rank_topn.  Domain: the ranking calls' -- E finite and >= +0.0.
 * topn is 1 .. 256 (only the fused route exists).  topn outside that, a side or metric not listed above, an id out of
 * range, or a null pointer with n_sel > 0 is HPF_ERR_INVALID before anything is launched; n_sel = 0 is HPF_OK; no E on
 * that side (neither hpf_set_state of it nor an iteration) is HPF_ERR_STATE; an odd row stride is HPF_ERR_UNSUPPORTED,
 * as for the other fused calls.  Needs no CSR.  Synchronous.  The model state is not written.
 * Device memory beyond inputs and outputs: for the cosine one rows x ld matrix of unit rows, freed when the call
 * returns; the candidate buffers of a batch of selected rows as in hpf_recommend (<= 512 MB; HPF_LOO_BATCH makes the
 * batches smaller).  No bit rows; nothing of size n_sel x rows. */
typedef enum { HPF_SIM_COSINE = 0, HPF_SIM_DOT = 1 } hpf_similarity;
int  hpf_similar(hpf_handle *h, int side, const uint32_t *ids, uint32_t n_sel,
                 uint32_t topn, int metric, uint32_t *out_ids, double *out_scores);

/* (an extension; the reference has no counterpart.)  Whom to show an item to: hpf_recommend transposed.  For selected item
 * items[b] the topn LOCAL users of this handle (with several ranks the local users only; nothing is exchanged, as for
 * hpf_similar side 0), in the ranking calls' one order, taken on the bit pattern: score descending, ties by ascending
 * user: out_users[b x topn + j] / out_scores[b x topn + j].
 * The score of (u, i) is, bit for bit, the double hpf_scores returns for that pair: the sweep issues the same MFMA chain
 * over k = 0, 4, 8, ... with the same zero padding, the item rows as the A operand and the user rows as the B operand --
 * a product does not depend on which operand is which -- and with bias the epilogue adds (E_ibias_i + E_ubias_u) as ONE
 * parenthesised sum, as the other fused calls do; that sum is commutative too.
 * Masking: a user's score is replaced by +0.0 when the user has a stored training rating > 0 for the item (ALL users of
 * the item's column when the handle has no values; a uint8-wrapped 0 is NOT masked, as for the users' calls), or when the
 * user is in the caller's mask list -- a CSR over the selected items, item b's entries mask_users[mask_ptr[b] ..
 * mask_ptr[b+1]) being local user ids: the validation pairs of that item.  mask_ptr = NULL: no list.  Masked users stay
 * candidates at +0.0 and tie with every other zero score by user id, like masked items in hpf_recommend.
 * Entries beyond n_users are (0xffffffff, 0.0).  topn is 1 .. 256 (only the fused route exists, as for hpf_similar).  An
 * item may be selected twice; both output rows are then equal.  Domain: the ranking calls' -- E finite and >= +0.0.
 * topn outside 1 .. 256, an item or a mask user out of range, mask_ptr[0] != 0, a decreasing mask_ptr, or a null pointer
 * with work to do is HPF_ERR_INVALID before anything is launched; n_sel = 0 is HPF_OK; no CSR, or no E on either side, is
 * HPF_ERR_STATE; an odd row stride is HPF_ERR_UNSUPPORTED, as for the other fused calls.
 * Synchronous.  The model state is not written.  The call waits for what hpf_recommend waits for: right after
 * hpf_iterate or hpf_fold_in_items it sees what hpf_get_state would export.
 * Device memory beyond inputs and outputs: the bit rows of a batch of items, one bit per USER (<= 256 MB; HPF_LOO_BATCH
 * makes the batches smaller), and the candidate buffers of the batch as in hpf_recommend (<= 512 MB: 10^6 users, topn =
 * 100: 2 112 items x 32 splits x 256 entries = 208 MB beside 264 MB of bit rows).  Nothing of size n_sel x n_users. */
int  hpf_audience(hpf_handle *h, const uint32_t *items, uint32_t n_sel,
                  const uint64_t *mask_ptr, const uint32_t *mask_users, uint32_t topn,
                  uint32_t *out_users /* n_sel x topn */, double *out_scores /* n_sel x topn */);

/* (an extension; the reference has no counterpart.)  How sure the model is of a score.  Every theta_uk, beta_ik and bias
 * is a Gamma with a shape and a rate; under the mean-field posterior the factors are independent, so per factor
 *   Var(theta beta) = vt * s + q * vb,   q = m * m, vt = q / a, p = n * n, vb = p / b, s = p + vb
 * with m = E[theta_uk], a = shape(theta_uk), n = E[beta_ik], b = shape(beta_ik) -- the doubles hpf_get_state would export
 * at the moment of the call; each of the five is ONE IEEE fp64 operation, nothing contracted into an FMA, no reciprocal,
 * the division correctly rounded.  The variance of a score is the sum over k, with bias plus Var(ubias_u) + Var(ibias_i),
 * each E * E / shape formed the same way.  It is taken as ONE dot product of C = 2 K + 2 * bias columns,
 *   X_u = [ vt_0 .. vt_{K-1} | q_0 .. q_{K-1}   | (bias:) Var ubias_u , 1.0         ]
 *   Y_i = [ s_0  .. s_{K-1}  | vb_0 .. vb_{K-1} | (bias:) 1.0         , Var ibias_i ]
 * by the chain hpf_scores issues (one MFMA accumulator per output over c = 0, 4, 8, ..., the tail padded by zeros): out_var
 * is, bit for bit, the double hpf_scores returns on a handle with K' = C, no bias, E[theta] = X and E[beta] = Y.  All terms
 * are >= 0, an element of X carries at most 2 roundings and one of Y at most 3: |var - exact| <= (C + 9) 2^-53 exact where
 * no intermediate is subnormal.  out_mean is, bit for bit, what hpf_scores returns for the pair on this handle.
 * Either output may be NULL.  A pair may be given twice.  Domain: the ranking calls' (E finite and >= +0.0) and shapes
 * finite and > 0; the library does not scan them.
 * C must fit HPF_MAX_COLUMNS -- K <= 511 with bias, K <= 512 without --, else HPF_ERR_UNSUPPORTED, as for an odd row
 * stride; an index out of range or a null u or i is HPF_ERR_INVALID; cnt = 0 is HPF_OK.  HPF_ERR_STATE: before the first
 * iteration E or the SHAPE of either side (with bias: of either bias) was not handed in with hpf_set_state or left by a
 * fold-in.  A snapshot records what was handed in: a handle that loads one taken before any iteration answers as the
 * handle it was taken from (a blob written by an earlier build of the library does not say so, and the shapes have to be
 * handed in again).  All of these are returned before anything is launched.
 * Synchronous.  The model state is not written (after a sweep S becomes the shape, as for an export: the same bits
 * hpf_get_state returns before and after, and a following hpf_iterate returns what it returns without the call).  Any
 * n_ranks: local users only, nothing exchanged.  No CSR is needed.  Device memory beyond inputs and outputs: none (the
 * derived columns are formed on the way). */
int  hpf_score_moments(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt,
                       double *out_mean, double *out_var);

/* (an extension.)  What to show when a guess is worth trying: hpf_recommend ordered by the optimistic score
 *   sd = sqrt(var), t = z * sd, ucb = mean + t        (three fp64 operations, sqrt correctly rounded, nothing contracted)
 * of the two moments above.  Arguments, masking (a masked item scores +0.0 and stays a candidate), order (ucb descending
 * on the bit pattern, ties by ascending item), padding (0xffffffff, 0.0), batches and error cases are hpf_recommend's;
 * topn is 1 .. 256 (only the fused route exists, as for hpf_similar / hpf_audience).  With z = 0 ucb is mean bit for bit
 * and the lists are hpf_recommend's.
 * For a listed item out_mean and out_var (n_sel x topn each; either may be NULL) are the pair's hpf_score_moments values
 * bit for bit, and out_ucb is the three-operation expression of them -- also for a masked item that got listed at +0.0:
 * the list says where it was ranked, out_ucb what it would have scored.  Padding entries are 0.0 in all three.
 * HPF_ERR_INVALID: z < 0, NaN or infinite (a negative z gives negative scores, which the key order does not cover), topn
 * outside 1 .. 256, a user or mask item out of range, a malformed mask_ptr, a null pointer with work to do.
 * HPF_ERR_UNSUPPORTED: C > HPF_MAX_COLUMNS or an odd row stride.  HPF_ERR_STATE: no CSR, or no E or no shape as for
 * hpf_score_moments.  n_sel = 0 is HPF_OK.  All returned before anything is launched.
 * Synchronous; the model state is not written; any n_ranks (local users only).
 * Device memory beyond inputs and outputs: hpf_recommend's bit rows and candidate buffers, and two temporaries freed when
 * the call returns: Y, n_items x ldx doubles, and X, (users of a batch) x ldx doubles, ldx = C padded to a multiple of 4
 * (10^5 items, K = 100: 10^5 x 200 x 8 B = 160 MB for Y). */
int  hpf_recommend_ucb(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                       const uint64_t *mask_ptr, const uint32_t *mask_items, uint32_t topn, double z,
                       uint32_t *out_items /* n_sel x topn */, double *out_ucb /* n_sel x topn */,
                       double *out_mean /* n_sel x topn, may be NULL */, double *out_var /* may be NULL */);

/* (an extension.)  Thompson sampling: one draw of the model from its posterior, and the top-N of that draw.  Every
 * theta_uk, beta_ik and bias is a Gamma(shape, rate) with E = shape / rate; an element's sample is g * (E / shape) with g a
 * Gamma(shape, 1) variate, so the rate is never read.  The variate is a pure function of (seed, draw, side, row, column):
 * Philox4x32-10 (multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85) with the key (seed low, seed high) and,
 * for block b of attempt j, the counter (column, row, draw, side | b << 4 | j << 8) -- side 0 users, 1 items; row the LOCAL
 * user index or the item index; column the element's column in the handle's row layout (factor k at k; with bias the user
 * bias at K, the item bias at K + 1).  Two words x, y give u = ((x >> 6) 2^26 + (y >> 6) + 0.5) 2^-52; block 0 gives u1, u2,
 * block 1 u3, u4.  Marsaglia-Tsang with a' = a < 1 ? a + 1 : a, d = a' - 1/3, cc = 1 / sqrt(9 d), for j = 0 .. 31:
 *   z = sqrt(-2 log u1) cos(2 pi u2); w = cc z; w > -1 and log u3 < z^2 / 2 + d (3 log1p(w) - w (3 + w (3 + w))) accepts
 *   g = d (1 + w)^3; for a < 1 then g = g exp(log(u4) / a).
 * Each line is one fp64 operation or one ocml call, nothing contracted (hgaprec_amd/csrc/hpf_rng.hpp compiles for host and
 * device; tests/thompson_ref.py is the numpy statement).  It does not depend on batches, grid, selection or call order:
 * the same (seed, draw) gives the same bits in every call, another draw or seed an independent model.
 * Domain: E finite and >= +0.0, shapes finite and > 0 (not scanned): every sample is finite and >= +0.0 (E = +0.0 gives
 * +0.0; a tiny shape may give +0.0), so the key order of the ranking calls covers a draw.
 *
 * hpf_sample_state: the draw of rows ids[0 .. n_sel) of one side (ids NULL: rows 0 .. n_sel - 1), out[n_sel x C], C = K +
 * bias, dense row-major: the K factor columns, then (bias) the side's own bias -- the host layout hpf_get_state uses for
 * THETA_E / BETA_E with UBIAS_E / IBIAS_E appended.  A row may be named twice.
 *
 * hpf_recommend_thompson: hpf_recommend on ONE draw (seed, draw) of both sides -- bit for bit, items and scores, what
 * hpf_recommend returns on a handle whose E are the two hpf_sample_state outputs: score = theta~ . beta~ (+ ubias~ + ibias~),
 * masking (a masked item scores +0.0 and stays a candidate), order, padding (0xffffffff, 0.0) and batches hpf_recommend's.
 * The item side is drawn ONCE per (seed, draw) and shared by all users of the call (and of every call with that pair): each
 * user's list is marginally a Thompson draw, the lists of different users are correlated through beta~.  topn is 1 .. 256
 * (only the fused route exists).
 *
 * HPF_ERR_INVALID: a side other than 0 or 1, an index out of range, a null pointer with work to do, and for the recommend
 * call hpf_recommend's cases (topn outside 1 .. 256 here).  HPF_ERR_STATE: no CSR (the recommend call), or no E or no shape
 * as for hpf_score_moments.  HPF_ERR_UNSUPPORTED: an odd row stride (the recommend call).  n_sel = 0 is HPF_OK.  All
 * returned before anything is launched.
 * Synchronous; the model state is not written (as for hpf_score_moments); any n_ranks (local users only).
 * Device memory beyond inputs and outputs, freed when the call returns: hpf_sample_state a piece of at most 256 MB of
 * sampled rows and its dense copy; hpf_recommend_thompson hpf_recommend's bit rows and candidate buffers, beta~ of n_items x
 * ld doubles and theta~ of (users of a batch) x ld doubles, ld the handle's row stride. */
int  hpf_sample_state(hpf_handle *h, int side, const uint32_t *ids, uint32_t n_sel,   /* ids NULL: rows 0 .. n_sel-1 */
                      uint64_t seed, uint32_t draw, double *out /* n_sel x (K + bias) */);
int  hpf_recommend_thompson(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                            const uint64_t *mask_ptr, const uint32_t *mask_items, uint32_t topn,
                            uint64_t seed, uint32_t draw,
                            uint32_t *out_items /* n_sel x topn */, double *out_scores /* n_sel x topn */);

/* (an extension.)  Diversified top-N: greedy maximal marginal relevance (MMR) over a pool of hpf_recommend's candidates --
 * pick the next item by relevance minus its similarity to what is already picked, so that the head of a list is not filled
 * by the near-duplicates that load on the user's strongest factor.
 *
 * Pool.  For a selected user the pool is the entries (c_j, r_j), j = 0 .. P - 1, of the list hpf_recommend returns for the
 * same user, mask list and topn = pool whose score is > +0.0 (no padding, no masked item, no true zero): a prefix of that
 * list, in its order, items and scores bit for bit hpf_recommend's.  P may be 0 and may be less than topn.
 *
 * Similarity.  G(a, b) is the cosine of rows a and b of E[beta] over the K factor columns as hpf_similar(side 1,
 * HPF_SIM_COSINE) defines it: the rows at unit length U (overflow-free, a row scaled by a power of two has the same U),
 * then the chain hpf_scores issues -- one MFMA accumulator per output over c = 0, 4, 8, ..., the tail padded by zeros.  Bit
 * for bit it is the double hpf_scores returns for (a, b) on a handle without bias whose E[theta] and E[beta] are both U.
 * Bias columns take no part.  G is symmetric bit for bit (a product does not depend on which operand is which).
 *
 * Greedy selection.  Every step is ONE IEEE fp64 operation, nothing contracted into an FMA, no reciprocal:
 *   rel_j = r_j / r_0 (correctly rounded);  om = 1.0 - lambda;  pen_j = 0.0
 *   for t = 0 .. min(topn, P) - 1:
 *     key_j = lambda * rel_j - om * pen_j            for every pool entry not yet picked
 *     j* = the entry with the largest key, compared as values (keys may be negative); among equal keys the smallest j
 *     out_items[t] = c_j*, out_scores[t] = r_j*, out_maxsim[t] = pen_j*, out_mmr[t] = key_j*
 *     pen_j = max(pen_j, G(c_j, c_j*))               for every entry still unpicked
 * Positions from min(topn, P) on are (0xffffffff, 0.0, 0.0, 0.0).
 * So: with lambda = 1 the lists are the entries of hpf_recommend(topn) with a positive score, bit for bit, then padding;
 * with pool == topn a list is a permutation of that set; the first pick is always c_0; a user's result depends only on the
 * user's pool and the rows of U of the pool's items -- not on batches, selection, grid or call order; a user selected
 * twice gives two equal rows.
 *
 * HPF_ERR_INVALID: topn outside 1 .. 256, pool outside topn .. HPF_DIVERSE_POOL_MAX, lambda NaN or outside [0, 1], and
 * hpf_recommend's cases (a user or mask item out of range, a malformed mask_ptr, a null pointer with work to do).
 * HPF_ERR_STATE: no CSR, or no E on either side.  HPF_ERR_UNSUPPORTED: an odd row stride.  n_sel = 0 is HPF_OK.  All
 * returned before anything is launched.
 * Synchronous; the model state is not written; any n_ranks (local users only).
 * Device memory beyond inputs and outputs, freed when the call returns: hpf_recommend's bit rows and candidate buffers, the
 * pool lists (n_sel x pool), U of n_items x ld doubles, and per workgroup of the persistent grid a slab of Pp x Pp doubles
 * for the Gram matrix (Pp = pool rounded up to 16; at most 512 KB each, 256 MB in all). */
#define HPF_DIVERSE_POOL_MAX 256
int  hpf_recommend_diverse(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                           const uint64_t *mask_ptr, const uint32_t *mask_items,
                           uint32_t topn, uint32_t pool, double lambda,
                           uint32_t *out_items /* n_sel x topn */, double *out_scores /* n_sel x topn */,
                           double *out_maxsim /* n_sel x topn, may be NULL */,
                           double *out_mmr /* n_sel x topn, may be NULL */);

/* (an extension; the reference has no counterpart.)  Why a score is what it is: the T largest of the terms whose sum a
 * pair's score is.  For pair p the terms are c_k = E[theta_u k] * E[beta_i k], k < K -- each ONE IEEE fp64 multiplication,
 * nothing fused into it and no reciprocal: the double returned is, bit for bit, the product a host forms from the two
 * hpf_get_state rows -- and with bias two more in the reference's K + 2 layout (hgaprec.cc:1347-1353): term K is
 * E[ubias_u] and term K + 1 is E[ibias_i], copied.  out_factor[p x T + r] / out_contrib[p x T + r] are the r-th term of
 * pair p in the ranking calls' one order, taken on the bit pattern: the larger term first, of equal terms the smaller
 * factor number.  Entries beyond the K + 2 * bias terms a score has are (0xffffffff, 0.0).  Domain: the ranking calls' --
 * E finite and >= +0.0 (a product may be subnormal or +0.0 and is ordered by its pattern like the rest).
 * u is a LOCAL user index.  A pair may be given twice; both rows are then equal.  T is 1 .. HPF_EXPLAIN_MAX.  T outside
 * that, a user or an item out of range, or a null pointer with cnt > 0 is HPF_ERR_INVALID before anything is launched;
 * cnt = 0 is HPF_OK; no E on either side is HPF_ERR_STATE, as for hpf_predict.  Needs no CSR.  Synchronous.  The model
 * state is not written.
 * The sum of a row with T = K + 2 * bias is NOT held to the bits of hpf_predict for the pair: that call adds the same
 * products in another order and fused (sixteen chains of FMAs, a tree, then the biases).  All terms are >= 0, so the two
 * agree to the roundings each takes: |hpf_predict - sum| <= (ceil(K / 16) + 10) 2^-53 sum for an exactly added row.
 * A wave per pair, the terms in registers; device memory beyond inputs and outputs: none. */
#define HPF_EXPLAIN_MAX 32
int  hpf_explain(hpf_handle *h, const uint32_t *u, const uint32_t *i, size_t cnt, uint32_t T,
                 uint32_t *out_factor /* cnt x T */, double *out_contrib /* cnt x T */);
/* (an extension.)  What a factor is: for every factor column k < K of one side -- 0: the rows of E[theta] of this handle's
 * users (with several ranks the LOCAL users only; nothing is exchanged, as for hpf_similar), 1: the rows of E[beta] -- the
 * topn rows with the largest E[r, k], ids ascending among equal values: out_ids[k x topn + j] / out_vals[k x topn + j].
 * The values are copies.  Bias columns take no part.  Entries beyond the row count are (0xffffffff, 0.0).  Domain: the
 * ranking calls'.  topn is 1 .. 1024, the limit of hpf_rank_topn, whose selection it is (one workgroup per column).  A
 * side not listed, topn outside that or a null pointer is HPF_ERR_INVALID before anything is launched; no E on that side
 * is HPF_ERR_STATE.  Needs no CSR.  Synchronous.  The model state is not written.
 * Device memory beyond the outputs: a batch of columns transposed to rows, <= 512 MB (one column where a single column
 * is longer), freed when the call returns; more than 2^32 / 8 rows in one column is HPF_ERR_UNSUPPORTED. */
int  hpf_factor_top(hpf_handle *h, int side, uint32_t topn,
                    uint32_t *out_ids /* K x topn */, double *out_vals /* K x topn */);

/* (an extension; the reference has no counterpart.)  "Because you rated": which of the user's OWN ratings carry a score.
 * All quantities are those hpf_get_state would export at the moment of the call.  For a local user u, hist(u) is the
 * nonzeros of u's CSR row in CSR order, each with the factor yy of the phi pass (y if y > 1, otherwise 1; 1 throughout when
 * the ratings were uploaded with val = NULL).  For a history item i
 *   phi_uic = exp(Elog theta_uc + Elog beta_ic) / sum_c' exp(...)
 * over the K factor entries and, with bias, the two bias entries of the reference's K + 2 layout (hgaprec.cc:1347-1353):
 * entry K is Elog ubias_u, entry K + 1 is Elog ibias_i and takes part in the denominator only.  With
 *   D_uc = s_prior + sum_{i in hist(u)} yy_i phi_uic      (c < K; with bias also c = K) -- the shape the user half of one
 *                                                          iteration would give row u from the current Elog --
 *   g_c  = E[theta_uc] E[beta_jc] / D_uc  (c < K),  g_K = E[ubias_u] / D_uK   for a target item j,
 * history item i contributes c(i -> j) = yy_i sum_c phi_uic g_c to the score of (u, j); prior(j) = s_prior sum_c g_c is the
 * prior's share and E[ibias_j] (with bias) belongs to nobody.  In exact arithmetic
 *   sum_i c(i -> j) + prior(j) + E[ibias_j] = sum_k E[theta_uk] E[beta_jk] + E[ubias_u] + E[ibias_j],
 * the score hpf_predict returns.  The definition reads E and Elog only -- no rate -- so it holds with and without hier.
 * Targets are a CSR over the selected users like the queries of hpf_rank_queries: selected user b asks for the items
 * t_items[t_ptr[b] .. t_ptr[b+1]); nt = t_ptr[n_sel].  Row q of out_item / out_contrib (q indexes t_items) holds the T
 * history items of the target's user with the largest c(i -> j), in the ranking calls' one order taken on the bit pattern:
 * the larger contribution first, ascending item among equal ones; entries beyond the history's length are
 * (0xffffffff, 0.0).  out_sum[q] (may be NULL) is the sum over the WHOLE history, added in CSR order; out_prior[q] (may be
 * NULL) is prior(j).  A target may be in the user's own history, a user may be selected twice, a target asked twice: equal
 * requests give equal rows, and a pair's result depends on nothing but the user's history, the state and the target.  Two
 * history items whose item rows and ratings are bit-identical get bit-identical contributions.
 * T outside 1 .. HPF_BECAUSE_MAX, a user or an item out of range, t_ptr[0] != 0, a decreasing t_ptr or a null pointer with
 * work to do is HPF_ERR_INVALID before anything is launched; n_sel = 0 or nt = 0 is HPF_OK; no CSR, or no E or Elog on
 * either side (with bias: of either bias), is HPF_ERR_STATE.  A softmax denominator that underflows is HPF_ERR_STATE too;
 * it is reported by this call alone and the handle stays usable.  Any n_ranks: the local users only, nothing is
 * exchanged.  Synchronous.  The model state is not written: every hpf_get_state returns the same bits before and after,
 * and a following hpf_iterate the bits it returns without the call.
 * A returned contribution and out_prior are within (4 S + H + 64) 2^-53 relative of the exact value, H the history's
 * length and S the largest Elog spread inside the user's row or a gathered item row.
 * Two kernels: a wave per selected user writes D, a wave per target pair walks the history again with g in registers and
 * the T best in its lanes.  Device memory beyond inputs and outputs, freed when the call returns: a plain fp64 copy of
 * exp(Elog beta - row max) (n_items x the padded column count) and D (n_sel x the same). */
#define HPF_BECAUSE_MAX 32
int  hpf_because(hpf_handle *h, const uint32_t *users, uint32_t n_sel,
                 const uint64_t *t_ptr, const uint32_t *t_items, uint32_t T,
                 uint32_t *out_item   /* nt x T */, double *out_contrib /* nt x T */,
                 double *out_sum      /* nt, may be NULL */, double *out_prior /* nt, may be NULL */);

/* replaces: HGAPRec::test() (hgaprec.cc:2257-2346) -- load the item factors, put the user at the prior
 * (set_to_prior + set_to_prior_curr, 2278-2279), run user-side CAVI iterations over the user's ratings with the item
 * side untouched.  The handle's users are the NEW users: their ratings uploaded with hpf_upload_csr[_device] (val = NULL:
 * every rating is 1), the item side handed in with hpf_set_state -- BETA_E and BETA_ELOG, with bias also IBIAS_E and
 * IBIAS_ELOG; no user-side state is needed or read.  A missing CSR or item state is HPF_ERR_STATE, n_iters = 0, tol < 0
 * or a NaN tol HPF_ERR_INVALID, all before anything is launched; zero users is HPF_OK.  Any n_ranks: the local users
 * only, nothing is exchanged.
 * Start: every user-side Gamma object (theta; xi with hier; the user bias with bias) at shape s_prior, rate r_prior,
 * E = s_prior / r_prior, Elog = psi(s_prior) - log(r_prior).  One iteration for user u is the user half of the
 * reference's: phi over the user's nonzeros in CSR order (K + 2 entries with bias, hgaprec.cc:1347-1353; scaled by y when
 * y > 1), theta shape = s_prior + sum_i phi_k, bias shape = s_prior + sum_i phi_K; theta rate = E[xi_u] of the PREVIOUS step
 * + c_k with c_k = sum over ALL items of E[beta_ik] (hier, 1370-1378) or the K-vector r_prior + c_k (vb, 927-956); bias
 * rate r_prior + n_items (1389); xi shape s_prior + K s_prior, rate r_prior + sum_k E[theta_uk] of the new theta
 * (1398-1405); E and Elog as gpbase.hh:248-262.  novb changes nothing here.
 * tol = 0: every user runs n_iters iterations.  tol > 0: user u stops after the first iteration t >= 2 with
 * max_k |E_t[theta_uk] - E_t-1[theta_uk]| <= tol max_k E_t[theta_uk], after n_iters at the latest.  iters_out[u] (may be
 * NULL) is the number of iterations u ran.  A user's result depends on nothing but its own ratings and the item side.
 * Leaves the user side as hpf_set_state of THETA_* (XI_*, UBIAS_*) would: every hpf_get_state, the scoring and ranking
 * calls and a later hpf_iterate see the folded-in state.  The item side is not written.  Synchronous.  A softmax
 * denominator that underflows surfaces as in the training passes (HPF_ERR_STATE).
 * One kernel launch runs all iterations of all users: a wave owns a user from the prior to its stop, with the user's
 * state in registers and its gathered item rows in LDS when they fit. */
int  hpf_fold_in(hpf_handle *h, uint32_t n_iters, double tol, uint32_t *iters_out /* n_users, may be NULL */);

/* The mirror of hpf_fold_in for a catalogue that grows: the item half of the reference's iteration (hgaprec.cc:1340-1414)
 * against a frozen user side.  The handle's ITEMS are the NEW items, its users the trained users: the ratings uploaded
 * with hpf_upload_csr[_device] -- a CSR over the trained users whose columns are new-item ids (val = NULL: every rating
 * is 1) -- and walked through the item-major view the upload built (users ascending inside an item); the user side handed
 * in with hpf_set_state -- THETA_E and THETA_ELOG, with bias also UBIAS_E and UBIAS_ELOG; no item-side state is needed or
 * read.  A missing CSR or user state is HPF_ERR_STATE, n_iters = 0, tol < 0 or a NaN tol HPF_ERR_INVALID, n_ranks > 1
 * HPF_ERR_UNSUPPORTED (users are sharded across ranks: an item's sums would need an exchange per iteration), all before
 * anything is launched; zero items is HPF_OK.
 * Start: every item-side Gamma object (beta; eta with hier; the item bias with bias) at shape s_prior, rate r_prior,
 * E = s_prior / r_prior, Elog = psi(s_prior) - log(r_prior).  One iteration for item i: phi over the item's nonzeros in
 * item-major order (K + 2 entries with bias, hgaprec.cc:1347-1353; scaled by y when y > 1), beta shape = s_prior +
 * sum_u phi_k, bias shape = s_prior + sum_u phi_K+1; beta rate = E[eta_i] of the PREVIOUS step + c_k with c_k = sum over
 * ALL users of the handle of E[theta_uk] (hier) or the K-vector r_prior + c_k; bias rate r_prior + n_users_total (1393;
 * 0 => n_users); eta shape s_prior + K s_prior, rate r_prior + sum_k E[beta_ik] of the new beta; E and Elog as
 * gpbase.hh:248-262.  novb changes nothing here.
 * tol = 0: every item runs n_iters iterations.  tol > 0: item i stops after the first iteration t >= 2 with
 * max_k |E_t[beta_ik] - E_t-1[beta_ik]| <= tol max_k E_t[beta_ik], after n_iters at the latest.  iters_out[i] (may be
 * NULL) is the number of iterations i ran.  An item's result depends on nothing but its own ratings and the user side --
 * not on its place in the list or on what else the handle holds.
 * Leaves the item side as hpf_set_state of BETA_* (ETA_*, IBIAS_*) would: every hpf_get_state, the scoring and ranking
 * calls and a later hpf_iterate see the folded-in state.  The user side is not written (c_k goes into a temporary).
 * Synchronous.  A softmax denominator that underflows surfaces as HPF_ERR_STATE.
 * Two kernels share the items: hpf_fold_in's (a wave per item) takes those with fewer than 256 ratings, a second one gives
 * every longer item to a whole workgroup whose waves walk contiguous parts of it and add their sums in a fixed order
 * (DESIGN.md section 4g): the same bits from run to run. */
int  hpf_fold_in_items(hpf_handle *h, uint32_t n_iters, double tol, uint32_t *iters_out /* n_items, may be NULL */);

/* how the uploaded matrix was cut into work (diagnostics, tests, bench):
 * a "segment" is <= 512 consecutive nonzeros of one row; rows longer than that
 * are "long" (their segment sums are combined by a second kernel) and rows with
 * more than 256 segments "huge" (combined in two levels).  On a TILED side
 * (tiles_* > 0) a segment is a run of one row inside one tile of the gathered
 * matrix, and the long rows also count the rows without any nonzero (the
 * combine zeroes them). */
typedef struct {
  uint64_t nnz;
  uint32_t user_segments, user_long_rows, user_huge_rows;
  uint32_t item_segments, item_long_rows, item_huge_rows;
  uint32_t phi_G, phi_R, phi_V;      /* lanes per nonzero, loads per lane, doubles per load */
  uint32_t sweep_G, sweep_R;         /* row sweep: lanes per row, columns per lane */
  uint32_t ld;                       /* row stride of the device matrices, doubles */
  uint32_t graph_replay;             /* 1: hpf_iterate replays a captured hipGraph; 2 (v8, opt-in): a rank of several replays the */
                                     /* iteration as three graphs cut by its collectives (hpf_iterate_local_items,        */
                                     /* hpf_iterate_local_users, hpf_iterate_global; hpf_timing then holds the item half   */
                                     /* under phi_item_ms, the user half under phi_user_ms, combine_* / sweep_user_ms 0)   */
  uint32_t w_layout;                 /* rows of W: 0 plain (phi_V elements per load), 3 packed 59-bit (lossless),  */
                                     /* 2 packed 48-bit (w_storage = 2), 4 plain doubles in the packed shape's     */
                                     /* 16-byte pieces (w_storage = 3, or after a fallback); 2-4: phi_R = pieces per lane */
  uint32_t tiles_user, tiles_item;   /* tiled phi pass: tiles of the gathered matrix (0: the side is row-major)   */
  /* ABI v5 */
  uint32_t tile_rows_user, tile_rows_item;   /* gathered rows per tile of that side's pass (0: row-major)          */
  uint64_t heavy_min_nnz_user, heavy_min_nnz_item; /* an owner row with at least this many nonzeros is regrouped  */
                                     /* tile by tile ("heavy"); the others stay row-major in the same launch       */
  uint32_t w_fallbacks;              /* how often the rows of W moved from the packed form to plain doubles because a    */
                                     /* state turned up that p59 cannot hold (w_layout then reads 4); 0 or 1            */
  uint32_t notes;                    /* bit 0 / 1: the user / item side was left row-major because the device is too     */
                                     /* small for the tiling's temporaries; bit 2 / 3: because their allocation failed   */
  /* ABI v7 */
  uint32_t start_sums_pending;       /* 1: -novb on several ranks and the tail of the exchange buffer does not hold the   */
                                     /* all-reduced sum_u E[theta] of the start state yet -- hpf_start_sums will leave    */
                                     /* this rank's PART there and a caller that owns the exchange has to sum-all-reduce  */
                                     /* it.  0 after hpf_snapshot_load of a state saved between iterations: the tail came */
                                     /* with the snapshot, already reduced; reducing it again would multiply it by the    */
                                     /* number of ranks.  v8: stays 1 after hpf_start_sums (no hpf_comm_init) until the   */
                                     /* next iteration begins -- read it before or after that call.                       */
  /* ABI v8 */
  uint32_t tile_chunk_user;          /* segments per workgroup of that side's tiled pass (0: row-major): two per wave     */
  uint32_t tile_chunk_item;          /* unless the list is too long for one launch of such chunks                         */
  uint32_t reserved0;
} hpf_work_info;
int  hpf_get_work_info(hpf_handle *h, hpf_work_info *out);

/* measurement: one phi pass with the arithmetic taken out -- same work list, index stream and
 * rows, the gathered bytes only folded into a register, nothing written.  The mean time of
 * `reps` launches (side 0: user-major pass, 1: item-major pass) is what the memory system needs
 * for that access pattern: the ceiling bench.py prints beside the pass itself.  Does not touch
 * the model state. */
int  hpf_gather_only(hpf_handle *h, int side, int reps, float *ms_out);

/* TEST HOOK (tests/test_gpu_fullsize.py): overwrite ONE entry of the index stream a phi pass
 * walks (side 0: user-major, 1: item-major; `pos` indexes the pass's own array -- the tiled copy
 * when the side is tiled) with `value` (< rows of the gathered side).  Returns the old value and
 * the owner row whose sum the entry feeds.  A pass over the damaged list still conserves mass
 * (every phi sums to its rating whichever row was gathered); the sampled-row checks must not
 * pass.  Never called by the product path. */
int  hpf_debug_poke_index(hpf_handle *h, int side, uint64_t pos, uint32_t value,
                          uint32_t *old_value, uint32_t *owner_row);

/* Page-locked host memory (ABI v6).  hpf_get_state / hpf_set_state / hpf_upload_csr / the snapshot calls
 * accept any host pointer; ordinary (pageable) memory goes through the library's two pinned staging
 * buffers and a threaded host copy -- on the MI355X boxes measured 44 GB/s out of the device into memory
 * that has been written before, 11-14 GB/s into freshly allocated pages (their first touch is most of
 * the time), 30-44 GB/s into the device -- while a buffer from hpf_host_alloc is the target of the DMA
 * itself (54 GB/s either way; tools/d2h_probe.hip, bench.py --host-handover).  Worth it for buffers that
 * are used again and again (page-locking costs ~0.15 s per GB, and as much again to undo): the CLI's
 * copies of the factor matrices, fetched at every report step (hgaprec.cc:1422 save_model).  No handle
 * is needed; HPF_ERR_OOM when the memory cannot be had (the caller falls back to malloc),
 * HPF_ERR_NO_DEVICE without a HIP device. */
int  hpf_host_alloc(void **ptr, size_t bytes);
int  hpf_host_free(void *ptr);

int  hpf_synchronize(hpf_handle *h);
int  hpf_last_timing(hpf_handle *h, hpf_timing *out);
/* mean over the last n_last iterations (at most 64 are kept); synchronises */
int  hpf_mean_timing(hpf_handle *h, uint32_t n_last, hpf_timing *out);
/* iteration_ms of each of the last n_last iterations, oldest first (hipEvents on the
 * handle's stream: first launch -> last launch of that iteration); *n_out = how many
 * were written (<= n_last, <= 64).  For a median instead of a mean. */
int  hpf_iteration_times(hpf_handle *h, uint32_t n_last, float *ms_out, uint32_t *n_out);

/* algorithmic bytes (SURVEY.md section 8d / DESIGN.md) moved by one launch of
 * the two phi passes and of the row sweeps for the uploaded matrix */
int  hpf_algorithmic_bytes(hpf_handle *h, uint64_t *phi_user, uint64_t *phi_item,
                           uint64_t *rows);

#ifdef __cplusplus
}
#endif
#endif /* HPF_H */
