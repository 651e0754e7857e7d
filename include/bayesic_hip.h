/* bayesic_hip.h -- C ABI of libbayesic_hip.so, the MI355X (gfx950) backend for
 * Bayesic's ELBO-gradient / mean-field update path.
 *
 * The reference (mjwillson/Bayesic) has no FFI: its numeric boundary is the
 * Python hook set that emits Theano ops.  Every entry
 * point below names the reference interface it stands behind.  All functions:
 *
 *   - are extern "C", take plain pointers and sizes, and return 0 on success or
 *     a negative bsc_status; bsc_last_error() gives the thread-local message;
 *   - take DEVICE pointers unless the parameter is named host_*;
 *   - are asynchronous on the context's HIP stream (no host sync, no
 *     allocation) unless documented otherwise, so a caller may capture a
 *     sequence of them into a hipGraph;
 *   - never fall back to a CPU implementation.
 *
 * Arithmetic: data operands float32 (the reference default dtype,
 * bayesic/algebra.py:109); statistics, gradients and variational parameters
 * float64 unless stated.
 */
#ifndef BAYESIC_HIP_H
#define BAYESIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSC_VERSION 100 /* 0.1.0 */
#define BSC_MAX_RANK 6  /* strided-tensor entry points accept up to 6 axes */

typedef enum bsc_status {
    BSC_OK = 0,
    BSC_ERR_INVALID = -1,     /* bad argument (shape, alignment, null pointer) */
    BSC_ERR_HIP = -2,         /* a HIP runtime call failed */
    BSC_ERR_UNSUPPORTED = -3, /* valid request outside what the kernels cover */
    BSC_ERR_NOMEM = -4
} bsc_status;

typedef struct bsc_ctx bsc_ctx;

/* ---- context, memory, timing (build decision; reference has none) ------- */

/* Binds to `device`; `stream` is a hipStream_t (or NULL for the null stream)
 * owned by the caller -- e.g. torch.cuda.current_stream().cuda_stream. */
int bsc_ctx_create(int device, void* stream, bsc_ctx** out);
int bsc_ctx_destroy(bsc_ctx* ctx);
int bsc_ctx_set_stream(bsc_ctx* ctx, void* stream);
/* Pre-size the context workspace (partial-sum slabs).  Synchronous.  Entry
 * points grow it on demand; call this first when capturing into a graph. */
int bsc_ctx_reserve(bsc_ctx* ctx, size_t bytes);
int bsc_ctx_sync(bsc_ctx* ctx);

/* ---- a launch sequence as one hipGraph ------------------------------------------------------
 * The reference re-walks its expression tree on every evaluation (bayesic/algebra.py:34-40, 60-61,
 * 767-768); a device update built from a few dozen short launches is then bound by the host walk,
 * not by the GPU.  Between bsc_capture_begin and bsc_capture_end every entry point called on the
 * context records its launches into a graph instead of running them (hipStreamBeginCapture on the
 * context's stream -- which must not be the null stream); bsc_graph_launch replays them in one
 * submission.  The graph holds the POINTERS the calls were given: the caller keeps every buffer
 * alive and at the same address, and refreshes inputs by writing into them.  Entry points that
 * synchronise (bsc_ctx_sync, bsc_d2h, bsc_h2d, a workspace that has to grow) fail inside a capture:
 * run the sequence once eagerly first.  bsc_capture_end returns an error, and leaves the stream
 * usable, when something inside could not be captured. */
typedef struct bsc_graph bsc_graph;
int bsc_capture_begin(bsc_ctx* ctx);
int bsc_capture_end(bsc_ctx* ctx, bsc_graph** out);
int bsc_graph_launch(bsc_ctx* ctx, bsc_graph* g);
int bsc_graph_destroy(bsc_graph* g);
/* info[0]=CU count, [1]=wavefront size, [2]=max LDS bytes per workgroup,
 * [3]=clock kHz, [4]=L2 bytes, [5]=gcn arch number (950 for gfx950). */
int bsc_device_info(bsc_ctx* ctx, int64_t info[8]);
const char* bsc_last_error(void);
int bsc_version(void);

int bsc_malloc(bsc_ctx* ctx, size_t bytes, void** out); /* synchronous */
int bsc_free(bsc_ctx* ctx, void* ptr);                  /* synchronous */
int bsc_h2d(bsc_ctx* ctx, void* dst, const void* host_src, size_t bytes);
int bsc_d2h(bsc_ctx* ctx, void* host_dst, const void* src, size_t bytes); /* syncs */
int bsc_memset(bsc_ctx* ctx, void* dst, int value, size_t bytes);

/* Arithmetic of the MFMA-bound contractions.  terms = 0 (default; the dtype of every reported figure): f32
 * operands on the f32 MFMA, products and sums exactly those of an fmaf chain.  terms = 2 or 3: every f32
 * operand is written as a sum of that many bf16 terms (round to nearest, repeatedly) and the product is
 * taken on the bf16 MFMA -- 16 x the f32 rate per instruction -- from the 3 resp. 6 leading cross products,
 * accumulated in f32: relative error per product <= ~2^-17 resp. ~2^-23 (the f32 class).  Honoured by
 * bsc_lda_sstats / bsc_lda_sstats_bound at K = 128 (2 and 3), bsc_logreg_bbvi_loglik for 36 <= S <= 64, S % 4 == 0
 * (2; with 3 it computes as with 0) and bsc_mog_estep (either value: its forward product -- differences of large
 * terms -- always takes three terms, its backward two) and by bsc_gemm_strided_batched / bsc_gemm_epilogue when both
 * operands are the SAME row-major matrix of <= 256 columns, a multiple of 32 (X^T X: 2); every other entry computes as
 * with 0.  Also the option
 * "mfma_split" of bsc_ctx_set_option.  Replaces nothing in the reference (bayesic/algebra.py:1347-1383
 * contracts in the dtype of its operands); SURVEY.md 8(d) config 4 leaves the operand-split variant open. */
int bsc_ctx_set_mfma_split(bsc_ctx* ctx, int terms);

/* Kernel selection is a property of the CONTEXT, set by explicit calls: the library reads no environment
 * variable.  Every A/B switch and tuning knob is a named integer option (csrc/bsc_api.hip OPTIONS: "blr_q_bias",
 * "gemm_dma", "lda_stream", "mfma_split", ...; bsc_ctx_option_name enumerates them, *host_key = NULL past the
 * last); a value outside an option's accepted set is an error, nothing is coerced.  Options that select
 * deletion builds (kernels with parts removed, for timing: their RESULTS ARE WRONG) are refused until the
 * option "profiling_builds" has been set to 1 on the same context, and then warn on stderr.  Defaults are the
 * measured best; a drop-in caller never needs these.  (The reference has no counterpart: its one backend
 * switch is Theano's own configuration, bayesic/algebra.py:54.) */
int bsc_ctx_set_option(bsc_ctx* ctx, const char* key, int64_t value);
int bsc_ctx_get_option(bsc_ctx* ctx, const char* key, int64_t* host_value);
int bsc_ctx_option_name(int32_t index, const char** host_key);

/* Per-kernel timing of the dominant kernel of each entry point, with hipEvents
 * recorded on the ctx stream immediately around that one launch.  enable = 0: off
 * (default); enable = n >= 1: time every n-th such launch (an event pair costs a
 * few microseconds of stream time, so a sampling period keeps the perturbation of
 * a timed region small).  bsc_ctx_profile_read synchronises, returns the summed
 * duration and the number of TIMED launches since the last read, and resets both. */
int bsc_ctx_profile(bsc_ctx* ctx, int enable);
int bsc_ctx_profile_read(bsc_ctx* ctx, double* host_total_ms, int64_t* host_launches);
/* The same reading per timing slot: 0 = the dominant kernel (what bsc_ctx_profile_read
 * returns), 1 = the collective of bsc_allreduce_sum, 2 = the finish kernel of
 * bsc_blr_fused_update.  Every slot is sampled with the period given to bsc_ctx_profile. */
int bsc_ctx_profile_read_slot(bsc_ctx* ctx, int slot, double* host_total_ms,
                              int64_t* host_launches);

/* ---- the exchange step of the data-parallel update: RCCL over xGMI -------------------
 * (ABSENT in reference; README.md:69-79 mini-batch SVI)  Rows are iid
 * (bayesic/distribution/base.py:146-172), every per-batch quantity is a SUM over rows, so
 * rank r of p holds a row block and the ranks exchange ONE vector per update: the
 * all-reduce(sum) of the concatenated statistic / gradient vector, after which every rank
 * applies the identical update.  The communicator is an ncclComm_t owned by the context;
 * the collective is enqueued on the context's own stream (pass -> all-reduce -> finish is
 * one in-order queue).  librccl is bound at run time by the first bsc_comm_* call, so a
 * single-GPU caller never maps it.
 *
 * bsc_comm_unique_id: rank 0 fills host_id[BSC_COMM_ID_BYTES] (ncclGetUniqueId) and hands
 *   the bytes to the other ranks over any host channel (a file, MPI, torch.distributed's
 *   store).  bsc_comm_init_rank: collective over all `world` ranks, synchronous; one
 *   communicator per context; world == 1 is allowed (the RCCL path at world size 1).
 *   bsc_comm_destroy is implied by bsc_ctx_destroy.
 * bsc_allreduce_sum / _max: in place over buf[n] (BSC_F32 | BSC_F64) on the ctx stream;
 *   on a context without a communicator they are the identity (a world of one). */
#define BSC_COMM_ID_BYTES 128
int bsc_comm_unique_id(void* host_id);
int bsc_comm_init_rank(bsc_ctx* ctx, const void* host_id, int32_t rank, int32_t world);
int bsc_comm_destroy(bsc_ctx* ctx);
int bsc_comm_info(bsc_ctx* ctx, int32_t* host_rank, int32_t* host_world,
                  int32_t* host_rccl_version);
int bsc_allreduce_sum(bsc_ctx* ctx, void* buf, int64_t n, int dtype);
int bsc_allreduce_max(bsc_ctx* ctx, void* buf, int64_t n, int dtype);
/* The same collective OVERLAPPED with the kernels that follow on the context's stream: _begin orders the
 * all-reduce behind everything enqueued so far (an event) and issues it on a second stream of the context;
 * kernels enqueued afterwards run beside it; _end(slot) makes the context's stream wait for that collective
 * (call it before the first kernel that reads `buf`).  slot < 16 names the collective in flight; each _begin
 * is ended once.  A context without a communicator (a world of one) does nothing in either; inside a graph
 * capture the collective stays on the captured stream.  Used where a statistic is finished piece by piece
 * (svi/lda.py: config 4's 51.2 MB all-reduce) -- only the last piece's collective is
 * exposed.  bsc_ctx_profile's slot 1 times every piece. */
int bsc_allreduce_sum_begin(bsc_ctx* ctx, void* buf, int64_t n, int dtype, int32_t slot);
int bsc_allreduce_sum_end(bsc_ctx* ctx, int32_t slot);

/* hipEvent wrappers so a ctypes caller can time the ctx stream. */
/* Measurement aid: best pure streaming-read rate (GB/s) over `buf` on this device, from
 * kernels that do nothing but read it: 16-byte loads into registers (two launch shapes) and
 * LDS-DMA of whole 1-KiB runs (one and two workgroups per CU; the first 4 GiB of `buf`) --
 * best of `reps` timed launches each.  Synchronises.  bench.py quotes the data pass against
 * this as well as against the spec-sheet peak. */
int bsc_hbm_read_probe(bsc_ctx* ctx, const void* buf, size_t bytes, int reps, double* host_gbps);

/* ---- mini-batch streaming: host memory -> HBM slots on a copy stream --------------
 * (README.md:69-79 "stochastic updates applied via subsampled minibatches"; the
 * reference has no loader -- SURVEY.md 8(f) rank 4.)  While the update of batch t
 * runs on the context's stream, batch t+1 crosses PCIe; the update kernels only ever
 * see device-resident batches.  submit queues the copy (after the kernels that last
 * read the slot), acquire makes the context's stream wait for the oldest submitted
 * batch and returns its device pointers, release marks the point on the context's
 * stream after which the slot may be overwritten.  At most n_slots batches may be
 * between submit and release.  Host buffers should be page-locked BY THE RUNTIME: allocated
 * with bsc_host_alloc (hipHostMalloc; torch pin_memory tensors qualify).  Memory that malloc
 * owns is never shown to the device -- there is no register-in-place entry point (round 2 had
 * one; a heap page it had registered, or the runtime had locked on the fly, was the address of a
 * later GPU memory fault: DESIGN.md section 10): a PAGEABLE source is copied by
 * the host, inside submit, into a page-locked bounce buffer of the slot, at a fraction of the
 * PCIe rate; it is free again when submit returns.  bsc_host_free drains the device before it
 * frees.  HOST BUFFER LIFETIME of a page-locked source: it
 * must stay valid and unchanged until submission k + n_slots has returned (submit
 * host-synchronises on the copy that last targeted the slot it is about to reuse), or
 * until bsc_loader_destroy.  Not thread-safe. */
typedef struct bsc_loader bsc_loader;
int bsc_host_alloc(size_t bytes, void** out);      /* hipHostMalloc: page-locked memory to stream from */
int bsc_host_free(void* host_ptr);
int bsc_loader_create(bsc_ctx* ctx, int64_t max_rows, int32_t D, int32_t n_slots, bsc_loader** out);
int bsc_loader_destroy(bsc_loader* loader);
int bsc_loader_submit(bsc_loader* loader, const float* host_X, int64_t ldx, const float* host_y,
                      int64_t rows);
int bsc_loader_acquire(bsc_loader* loader, const float** dX, const float** dy, int64_t* rows);
int bsc_loader_release(bsc_loader* loader);

int bsc_event_create(void** event);
int bsc_event_destroy(void* event);
int bsc_event_record(bsc_ctx* ctx, void* event);
int bsc_event_elapsed_ms(void* start, void* stop, float* host_ms); /* syncs on stop */

/* ---- reparameterisation sampler (ABSENT in reference; README.md:51) ----- */

/* Philox4x32-10 keyed standard normals, float64:
 *   eps[s*n_params + d], counter=(d/4, s, stream, step), key=(seed lo, hi). */
int bsc_philox_normal(bsc_ctx* ctx, uint64_t seed, uint32_t stream, uint32_t step,
                      int32_t n_samples, int32_t n_params, double* eps);

/* Bayesian linear regression q(w)=N(m,diag e^{2rho}), q(xi)=N(a,e^{2b});
 * lam=[m(D),rho(D),a,b] float64.  Writes eps[S,(D+1)] f64, W[S,D] f32
 * (w_s = m + e^rho * eps_s, rounded), xi[S] f64. */
int bsc_blr_sample(bsc_ctx* ctx, const double* lam, int32_t D, int32_t S,
                   uint64_t seed, uint32_t step, double* eps, float* W, double* xi);

/* The same noise for n_steps consecutive Philox steps [step0, step0+n_steps) in
 * one launch: eps[(k*S + s)*(D+1) + d].  The noise does not depend on the
 * parameters, so a driver produces it ahead of time (off the update's latency
 * chain) and hands it to bsc_blr_fused_update with eps_next_ready = 1. */
int bsc_blr_noise(bsc_ctx* ctx, int32_t D, int32_t S, uint64_t seed, uint32_t step0,
                  int32_t n_steps, double* eps);

/* ---- the mini-batch data pass (ABSENT in reference; README.md:51,69-79;
 *      likelihood decomposition bayesic/distribution/base.py:47-69) --------
 *
 * One streaming pass over X[B,D] (row-major, leading dimension ldx floats)
 * and y[B]:
 *      r[n,s] = y[n] - sum_d X[n,d] W[s,d]
 *      Q[s]   = sum_n r[n,s]^2            (float64 out)
 *      G[s,d] = sum_n r[n,s] X[n,d]       (float64 out, [S,D])
 * Requires D % 4 == 0, D <= 256, 1 <= S <= 64, X 16-byte aligned, ldx % 4 == 0.
 * Deterministic: fixed partition, fixed-order float64 finish.
 * S > 8: X is read once per SIXTEEN draws at D == 256 (both contractions on the MFMA pipe:
 * 1M x 256, S = 16 in 202-232 us, S = 64 in 751-775 us), once per eight otherwise. */
int bsc_blr_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                      int64_t B, int32_t D, const float* W, int32_t S,
                      double* Q, double* G);

/* Same pass, but leaves the per-workgroup float32 partials in the context
 * workspace for bsc_blr_fused_update(stats = NULL) to finish -- saves the
 * separate reduction launch on the single-GPU path.  Requires S <= 8.  The
 * partials stay valid until the next call that uses the workspace. */
int bsc_blr_data_pass_partial(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                              int64_t B, int32_t D, const float* W, int32_t S);

/* The same two passes with the SWEEP ORDER chosen by the caller -- for a mini-batch that is
 * read again by the next pass (the following update of a resident batch; the next group of 8
 * draws when S > 8).  MI355X keeps the last ~256 MiB it has read in the Infinity Cache unless a
 * load says otherwise, so passes that alternate BSC_SWEEP_FORWARD_KEEP / BSC_SWEEP_BACKWARD_KEEP
 * start in the rows the previous pass ended with: 0.25 of a 1M x 256 mini-batch is then served
 * on-die (164 -> 158 us per pass), all of a shard below 256 MiB.  BSC_SWEEP_STREAM is what the
 * plain entry points do: forward, every load non-temporal, nothing left behind -- right for a batch
 * that is read once.  The statistics are the same sums taken in another order (float32 block
 * partials, so the last bits differ between orders; each order is deterministic).  When S > 8 the
 * sample groups alternate, starting from `sweep`.  D == 256 only; other widths always stream. */
#define BSC_SWEEP_STREAM 0
#define BSC_SWEEP_FORWARD_KEEP 1
#define BSC_SWEEP_BACKWARD_KEEP 2
int bsc_blr_data_pass_sweep(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                            int64_t B, int32_t D, const float* W, int32_t S,
                            double* Q, double* G, int32_t sweep);
int bsc_blr_data_pass_partial_sweep(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                                    int64_t B, int32_t D, const float* W, int32_t S,
                                    int32_t sweep);

/* Measurement aid (option "blr_stamps" = 1): the D = 256, S <= 8 pass leaves per workgroup
 * {start, end} in s_memrealtime ticks (100 MHz), the XCD it ran on and its HW_ID; this copies the
 * stamps of the LAST such launch to host_stamps[8 * rows] (synchronises; entries 4..7 of a row are unused).
 * Shows how evenly a static partition of the mini-batch finishes (tools/ab_q.py).
 * Option "blr_finish_stamps" = 1: the fused finish (bsc_blr_fused_update*, bsc_blr_pass_update*) leaves, per
 * workgroup (the column workgroups, then the scalar one), nine stage stamps in two rows of eight words
 * {wave start, small operands landed, slab summed, after the workgroup barrier, the scalar workgroup's
 * per-draw terms handed over and their sums done, Adam done, stores issued, end, seven unused}; a stage a workgroup does not have repeats the one
 * before it.  The rows of the LAST stamped finish follow the pass's rows (none when blr_stamps is off).  Nothing is
 * stamped while capturing. */
int bsc_blr_read_stamps(bsc_ctx* ctx, uint64_t* host_stamps, int32_t capacity_rows, int32_t* host_rows);

/* How many launches of the pass kernel bsc_blr_data_pass[_sweep] makes for S draws (eight per pass, or
 * sixteen while more than eight are left at D = 256): what a caller that alternates sweep directions
 * per update needs to know, answered by the library that decides it. */
int bsc_blr_pass_count(bsc_ctx* ctx, const float* y, int32_t D, int32_t S, int32_t* count);

/* Monte-Carlo ELBO and pathwise gradient from the (all-reduced) pass outputs.
 * batch_rows = global mini-batch rows, scale = N_total / batch_rows.
 * Writes elbo[1], grad[2D+2] (float64). */
int bsc_blr_elbo_grad(bsc_ctx* ctx, const double* lam, const double* eps,
                      const float* W, const double* xi, const double* Q,
                      const double* G, int32_t D, int32_t S, double batch_rows,
                      double scale, double alpha0, double beta0, double* elbo,
                      double* grad);

/* Fused finish of one update, one launch: (float64 reduction of the pending
 * partials when stats == NULL, else stats = [Q (S) | G (S*D)] as all-reduced)
 * -> ELBO + pathwise gradient (as bsc_blr_elbo_grad) -> Adam ascent step t
 * (as bsc_adam_ascent) written to lam_out (lam_in is not modified; m1, m2
 * updated in place) -> when the *_next buffers are non-NULL, the reparameterised
 * draws of Philox step `next_step` from lam_out (as bsc_blr_sample); with
 * eps_next_ready != 0 eps_next is an INPUT already holding that step's noise
 * (bsc_blr_noise) and only W_next / xi_next are written.  The caller
 * double-buffers lam and the draws: *_next must not alias eps/W/xi. */
int bsc_blr_fused_update(bsc_ctx* ctx, const double* stats, const double* lam_in,
                         double* lam_out, double* m1, double* m2, const double* eps,
                         const float* W, const double* xi, int32_t D, int32_t S,
                         double batch_rows, double scale, double alpha0, double beta0,
                         int64_t t, double lr, double beta1, double beta2, double adam_eps,
                         uint64_t seed, uint32_t next_step, double* eps_next,
                         int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo,
                         double* grad);

/* The same fused finish for any log-joint per draw of the family
 *     f(w, xi; Q) = c0 + c_xi xi + e^{-xi} (-s_q Q / 2 - k_w |w|^2 / 2 - beta),   Q = sum_n (y_n - x_n.w)^2,
 *     d f / d w = e^{-xi} (s_q G - k_w w),   d f / d xi = c_xi + e^{-xi} (s_q Q / 2 + k_w |w|^2 / 2 + beta)
 * -- a Gaussian-linear likelihood with log noise variance xi, a zero-mean Gaussian prior on w of precision
 * k_w e^{-xi} and a log-variance prior linear in xi and e^{-xi} (an inverse-Gamma on the variance, a Gamma
 * on the precision, flat).  bsc_blr_fused_update is the member c0 = -(scale B + D)/2 log 2 pi + alpha0 log
 * beta0 - lnGamma(alpha0), c_xi = -(scale B + D)/2 - alpha0, s_q = scale, k_w = 1, beta = beta0.  This is what
 * bayesic_amd.inference.ReparamVI launches when it recognises such a model written with Distribution nodes
 * and bayesic.algebra expressions (bayesic/distribution/base.py:47-69 decomposition; coefficient extraction
 * with match, bayesic/algebra.py:1037-1063). */
/* One call per update: the data pass of bsc_blr_data_pass_partial_sweep followed by the finish of
 * bsc_blr_fused_update[_general] with stats = NULL -- the same two launches, with the same results bit for bit.
 * (Carrying the finish in the pass launch's tail was built and measured break-even, and removed: DESIGN.md
 * section 9.)  Arguments: those of the two entry points it replaces.  README.md:51, 69-79. */
int bsc_blr_pass_update(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D, int32_t sweep,
                        const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps, const float* W,
                        const double* xi, int32_t S, double batch_rows, double scale, double alpha0, double beta0,
                        int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                        uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next,
                        double* elbo, double* grad);
int bsc_blr_pass_update_general(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                                int32_t sweep, const double* lam_in, double* lam_out, double* m1, double* m2,
                                const double* eps, const float* W, const double* xi, int32_t S, double c0, double c_xi,
                                double s_q, double k_w, double beta, int64_t t, double lr, double beta1, double beta2,
                                double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                                int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo, double* grad);
int bsc_blr_fused_update_general(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out,
                                 double* m1, double* m2, const double* eps, const float* W, const double* xi,
                                 int32_t D, int32_t S, double c0, double c_xi, double s_q, double k_w, double beta,
                                 int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                                 uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                                 double* xi_next, double* elbo, double* grad);

/* The finish of bsc_blr_fused_update_general for a FULL-COVARIANCE Gaussian guide (full-rank ADVI, Kucukelbir et al.):
 * q(z) = N(mu, L L^T) over z = [w (D) | xi], P = D + 1, L lower-triangular with L_ii = e^{rho_i}.
 *     lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal (P(P+1)/2)]
 * row i of L starts at lam[P + i(i+1)/2] and its diagonal slot holds rho_i (33 410 doubles at D = 256); m1, m2 and
 * grad have lam's layout.  Same family f(w, xi; Q) and arguments as bsc_blr_fused_update_general; per update, with
 * eps_s in bsc_blr_noise's [S, D+1] layout (stream 0 for w, stream 1 for xi) and g_s = d f / d z at
 * z_s = mu + L eps_s (the w part at the float32-rounded W):
 *     ELBO = mean_s f_s + sum_i rho_i + P/2 (1 + log 2 pi)
 *     d / d mu = mean_s g_s,   d / d L_ij = mean_s g_si eps_sj (j < i),   d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
 * then Adam ascent on every entry (bsc_blr_fused_update's hyper-parameters and bias correction) and, when the *_next
 * buffers are set, the next draw z'_s = mu' + L' eps'_s into W_next (float32 [S, D]) and xi_next [S].
 * eps_next_ready = 0: the noise of next_step is drawn into eps_next first (one bsc_blr_noise launch).  With every
 * off-diagonal entry zero the update equals the mean-field one on the same noise, term by term.
 * stats = [Q (S) | G (S*D)] as the data pass and the all-reduce leave them (NULL is refused: the pending partials of
 * bsc_blr_data_pass_partial are not read).  One launch of (D + 2) / 2 workgroups, workgroup k owning rows k and
 * D - k of L; fixed-order sums, no atomics: reproducible bit for bit.  The caller double-buffers lam and the draws.
 * Requires D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64. */
int bsc_blr_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, const double* xi, int32_t D, int32_t S,
                            double c0, double c_xi, double s_q, double k_w, double beta, int64_t t, double lr,
                            double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                            double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo,
                            double* grad);

/* ---- reparameterised SVI for canonical-link GLMs (csrc/bsc_glm.hip; ABSENT in the reference: README.md:51,
 *      69-79 on the likelihood split of bayesic/distribution/base.py:47-69) ----------------------------------
 *
 * One streaming pass over X[B,D] (row-major, leading dimension ldx floats) and y[B], for S draws W[S,D]:
 *      l[n,s]  = sum_d X[n,d] W[s,d]
 *      ell[s]  = sum_n ( y[n] l[n,s] - A(l[n,s]) )          (float64 out)
 *      G[s,d]  = sum_n ( y[n] - A'(l[n,s]) ) X[n,d]         (float64 out, [S,D])
 * link = BSC_GLM_LOGISTIC: A = softplus, max(l, 0) + log1p(exp(-|l|)), A' = sigmoid from the same exponential
 * (finite for every finite l); y in {0, 1}.  link = BSC_GLM_POISSON: A = A' = exp(l), NOT clamped -- a clamp
 * would change the gradient silently -- so the results are finite for l <= 88 only; ell leaves the constant
 * -sum_n lnGamma(y[n] + 1) of the Poisson log-density out.
 * The envelope is bsc_blr_data_pass's: D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 (eight draws per launch), X and W
 * 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26, contiguous y; B = 0 gives zeros.  Deterministic: fixed
 * partition, float32 block partials, fixed-order float64 finish, no float atomics. */
#define BSC_GLM_LOGISTIC 0
#define BSC_GLM_POISSON 1
int bsc_glm_data_pass(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                      const float* W, int32_t S, double* ell, double* G);

/* Finish of one update for q(w) = N(m, diag e^{2 rho}), lam = [m (D) | rho (D)], under the prior
 * w ~ N(0, I / prior_precision), in one launch: (float64 reduction of the pending pass partials when
 * stats == NULL -- S <= 8 --, else stats = [ell (S) | G (S*D)] as the pass and the all-reduce leave them) ->
 *     elbo   = mean_s [scale ell_s - tau/2 |w_s|^2] + D/2 log(tau / 2 pi) + sum rho + D/2 (1 + log 2 pi)
 *     g_s    = scale G_s - tau w_s          (w_s: the float32 draw the pass read),   scale = n_total / batch_rows
 *     d/d m  = mean_s g_s,     d/d rho_d = mean_s g_sd eps_sd e^{rho_d} + 1
 * -> Adam ascent step t (bsc_blr_fused_update's form and bias correction; lam_in is not modified, m1 and m2 are
 * updated in place) -> when the *_next buffers are set, W_next = m' + e^{rho'} eps_next rounded to float32.
 * eps and eps_next are in bsc_blr_noise's [S, D+1] layout (Philox stream 0 in columns 0 .. D-1; column D is not
 * read); eps_next_ready = 0: the noise of next_step is drawn into eps_next first (one bsc_blr_noise launch).
 * For the Poisson link elbo leaves -scale sum_n lnGamma(y_n + 1) out (it does not depend on lam).
 * The caller double-buffers lam and the draws: *_next must not alias eps / W. */
int bsc_glm_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                   const double* eps, const float* W, int32_t D, int32_t S, double scale, double prior_precision,
                   int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                   double* eps_next, int32_t eps_next_ready, float* W_next, double* elbo, double* grad);

/* One call per update: the pass (S <= 8, its partials left in the workspace) followed by the finish with
 * stats = NULL -- two launches. */
int bsc_glm_pass_update(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                        const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps, const float* W,
                        int32_t S, double scale, double prior_precision, int64_t t, double lr, double beta1, double beta2,
                        double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                        float* W_next, double* elbo, double* grad);

/* The same pass with a per-row offset o[B] and a per-row weight v[B] (csrc/bsc_glm_obs.hip; float32, contiguous, any
 * 4-byte alignment; each may be NULL: o = 0, v = 1):
 *      l[n,s]  = sum_d X[n,d] W[s,d] + o[n]
 *      ell[s]  = sum_n v[n] ( y[n] l[n,s] - A(l[n,s]) )
 *      G[s,d]  = sum_n v[n] ( y[n] - A'(l[n,s]) ) X[n,d]
 * A and A' as above.  The offset carries an exposure (Poisson rate model: o[n] = log exposure[n]) or any fixed part
 * of the linear predictor; the weights are the trials of aggregated binomial rows (y = k / n, v = n), survey or
 * importance weights, or a row mask.  They are part of the likelihood: the mini-batch scale of the finish stays
 * n_total / batch_rows.  A row with v[n] = 0 contributes EXACTLY nothing to ell and G -- a select, not a product --
 * also when its link value overflows (a Poisson logit of 200); its x, y and o must be finite.  Negative weights are
 * the caller's to exclude: the pass does not check them (a row with v[n] < 0 is dropped like one with v[n] = 0).
 * The slab, the float64 reduction and the outputs are bsc_glm_data_pass's, and so are the envelope and its refusals.
 * With offset == weight == NULL the kernels of bsc_glm_data_pass run and the outputs are bit-identical to it.  The
 * 16-row MFMA kernel (D == 256) is taken when y and the vectors that are set are all 16-byte aligned, else the 8-row
 * kernel. */
int bsc_glm_data_pass_obs(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, const float* offset,
                          const float* weight, int64_t B, int32_t D, const float* W, int32_t S, double* ell, double* G);

/* bsc_glm_pass_update with offset and weight (bsc_glm_data_pass_obs) after y: the pass for S <= 8 followed by the
 * finish with stats = NULL.  With both NULL it is bit-identical to bsc_glm_pass_update. */
int bsc_glm_pass_update_obs(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y,
                            const float* offset, const float* weight, int64_t B, int32_t D, const double* lam_in,
                            double* lam_out, double* m1, double* m2, const double* eps, const float* W, int32_t S,
                            double scale, double prior_precision, int64_t t, double lr, double beta1, double beta2,
                            double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                            float* W_next, double* elbo, double* grad);

/* ---- random-intercept logistic / Poisson regression on the same pass (csrc/bsc_glm_group.hip) ---------------------
 *
 *      y_n ~ Bernoulli(sigmoid(l_n)) or Poisson(exp(l_n)),   l[n,s] = sum_d X[n,d] W[s,d] + b_s[g[n]] + o[n]
 *      w ~ N(0, I / prior_precision),   b_j | zeta ~ N(0, e^{-zeta}),   tau = e^{zeta} ~ Gamma(a0, b0)
 * with g[n] in [0, J) the row's group.  The latent is z = [w (D) | b (J) | zeta], P = D + J + 1, the guide mean-field:
 * lam = [m (P) | rho (P)].  From the data one update needs, per draw s,
 *      ell[s]  = sum_n v[n] ( y[n] l[n,s] - A(l[n,s]) )
 *      G[s,d]  = sum_n r[n,s] X[n,d]                         r[n,s] = v[n] ( y[n] - A'(l[n,s]) )
 *      H[s,j]  = sum_{n : g[n] = j} r[n,s]
 * offset and weight are bsc_glm_data_pass_obs's (each may be NULL; a row with v[n] = 0 adds exactly nothing).
 *
 * The group plan.  H is a scatter; it is summed without float atomics in an order the PLAN fixes: the rows in stable
 * order by group (ascending row within a group), each group's run cut into segments of at most BSC_GLM_GROUP_SEG_ROWS
 * rows, a (start, length, group) table and every group's range of segments -- an opaque int32 array of
 * bsc_glm_group_plan_size(B, J) entries (-1: B or J outside the plan's range).  bsc_glm_group_plan builds it from
 * device g[B] into device memory: g is copied down, counting-sorted on the host and the plan copied up, so the call is
 * SYNCHRONOUS like bsc_malloc -- call it when a batch is set, never inside an update.  It is the one place ids are
 * range-checked: an id outside [0, J) is refused with the first offending row named.  *n_segments (may be NULL)
 * receives the segment count.  bsc_glm_group_plan_host is its core on host pointers (no device, no context). */
#define BSC_GLM_GROUP_SEG_ROWS 512
#define BSC_GLM_GROUP_MAX_J 65536
#define BSC_GLM_GROUP_MAX_ROWS ((int64_t)1 << 30)
int64_t bsc_glm_group_plan_size(int64_t B, int32_t J);
int bsc_glm_group_plan_host(const int32_t* g, int64_t B, int32_t J, int32_t* plan, int32_t* n_segments);
int bsc_glm_group_plan(bsc_ctx* ctx, const int32_t* g, int64_t B, int32_t J, int32_t* plan, int32_t* n_segments);

/* The pass.  Bz holds the intercept draws in float32 as [ceil(S / 8)][J][8] -- chunk of eight draws, group, draw slot;
 * unused slots are zero -- so that one launch (eight draws) gathers Bz[chunk][g[n]][slot] through a descriptor of
 * exactly J * 32 bytes: no id can read outside the table.  Outputs float64: ell [S], G [S, D], H [S, J]; a group
 * without rows gets exactly 0.  Per chunk of eight draws: the pass kernel (it also leaves every residual in the
 * workspace, 32 bytes per row), the float64 slab reduction, one wave per plan segment summing its rows' residuals in
 * float64, and the groups' segments added in segment order.  Every order of summation depends on the plan alone:
 * results are reproducible bit for bit.  With Bz = 0, ell and G are bit-identical to bsc_glm_data_pass_obs on the same
 * inputs.
 * The envelope is bsc_glm_data_pass_obs's, and 1 <= J <= BSC_GLM_GROUP_MAX_J, B <= BSC_GLM_GROUP_MAX_ROWS; g int32,
 * contiguous; plan the one built for this g, B and J (a plan whose header names another B or J is not read: H comes
 * back NaN).  The 16-row MFMA kernel (D == 256) is taken when y, g and the set ones of offset and weight are 16-byte
 * aligned, else the 8-row kernel.  The workspace (bsc_glm_group_workspace_bytes(ctx, B, J): slab, residuals, segment
 * sums) grows on demand -- synchronously; bsc_ctx_reserve it first to keep updates asynchronous. */
int64_t bsc_glm_group_workspace_bytes(bsc_ctx* ctx, int64_t B, int32_t J);
int bsc_glm_data_pass_groups(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y,
                             const float* offset, const float* weight, const int32_t* g, const int32_t* plan, int64_t B,
                             int32_t D, int32_t J, const float* W, const float* Bz, int32_t S, double* ell, double* G,
                             double* H);

/* The finish, two launches.  stats = [ell (S) | G (S*D) | H (S*J)] as the pass and the all-reduce leave them (NULL is
 * refused); eps in bsc_blr_noise's [S, (P-1)+1] layout (the last column is zeta's noise); W [S, D] and Bz (the layout
 * above) the float32-rounded draws the pass read; zeta_s = m_zeta + e^{rho_zeta} eps_s,P-1 in float64:
 *     g_w    = scale G_s - prior_precision w_s
 *     g_b    = scale H_s - e^{zeta_s} b_s
 *     g_zeta = J/2 + a0 - e^{zeta_s} (b0 + 1/2 sum_j b_sj^2)
 *     ELBO   = mean_s [scale ell_s + log p(z_s)] + sum rho + P/2 (1 + log 2 pi)
 *     d/d m  = mean_s g_s,     d/d rho_i = mean_s g_si eps_si e^{rho_i} + 1
 * (log p(z) with every normaliser: at prior_precision = 1 it is the log-prior of the score-function route,
 * bsc_logreg_bbvi_*), then Adam ascent step t (bsc_adam_ascent's form; lam_in is not modified, m1 and m2 in place)
 * and, when the *_next buffers are set (all or none), W_next [S, D] and Bz_next (chunked, unused slots zeroed) from
 * eps_next; eps_next_ready = 0 draws the noise of next_step into eps_next first.  lam_in != lam_out; the *_next buffers
 * must not alias the current ones.  Requires 1 <= S <= 64, 1 <= J <= BSC_GLM_GROUP_MAX_J, t >= 1 and
 * prior_precision, a0, b0, scale > 0.  Fixed-order sums, no atomics. */
int bsc_glm_hier_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                        double* m2, const double* eps, const float* W, const float* Bz, int32_t D, int32_t J, int32_t S,
                        double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                        double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                        int32_t eps_next_ready, float* W_next, float* Bz_next, double* elbo, double* grad);

/* ---- negative-binomial regression with a learned dispersion on the same pass (csrc/bsc_glm_nb.hip) ----------------
 *
 *      y_n ~ NegBin(mean mu_n = exp(l_n), dispersion phi),   Var y_n = mu_n + mu_n^2 / phi,   l[n,s] = sum_d X[n,d] W[s,d] + o[n]
 *      w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0):  log p(tau) = a0 log b0 - lnGamma(a0) + a0 tau - b0 e^tau
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  One dispersion draw rides
 * with every weight draw: logphi[s] = tau_s, float32 [S], any 4-byte alignment.  With u = l - tau_s, phi_s = e^{tau_s}
 * (float32 expf of the value read), sp = softplus and sg = sigmoid in bsc_glm_data_pass's stable forms -- the
 * log-density is the logistic link at a shifted logit and is finite for EVERY finite l, which the Poisson link is not --
 *      ell[s]  = sum_n v[n] ( dlnGamma(y[n], phi_s) + y[n] u - (y[n] + phi_s) sp(u) )      dlnGamma(y, phi) = lnGamma(y + phi) - lnGamma(phi)
 *      G[s,d]  = sum_n r[n,s] X[n,d]             r[n,s] = v[n] ( y[n] - (y[n] + phi_s) sg(u) )                  (= d / d l)
 *      T[s]    = sum_n v[n] ( phi_s dpsi(y[n], phi_s) - phi_s sp(u) ) - sum_n r[n,s]          dpsi(y, phi) = psi(y + phi) - psi(phi)
 * (T[s] = d ell[s] / d tau_s; ell leaves the constant -sum_n v[n] lnGamma(y[n] + 1) out, as the Poisson link does.)
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select); y >= 0, not necessarily an integer; both
 * differences are exactly 0 at y = 0.  They are evaluated in float32 per (row, draw), csrc/bsc_special_f32.h: for a whole
 * y <= 8 as the product and the sum they are, log prod_{i<y} (phi_s + i) and sum_{i<y} 1 / (phi_s + i); otherwise from a
 * shift of y + phi_s up to >= 8 and three asymptotic terms, against lnGamma(phi_s) and psi(phi_s) made once per launch
 * in float64.
 * ACCURACY ENVELOPE: tau in [-2.5, 5] (phi in [0.08, 148]).  Above it T's terms cancel (phi dpsi - phi sp - r -> 0 as
 * phi -> infinity) beyond what float32 holds, and lnGamma(y + phi) - lnGamma(phi) loses its digits to lnGamma(phi);
 * past tau = 10 the eight-factor product overflows.
 * The envelope and its refusals are bsc_glm_data_pass_obs's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); logphi == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics. */
int bsc_glm_nb_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                         const float* weight, int64_t B, int32_t D, const float* W, const float* logphi, int32_t S,
                         double* ell, double* G, double* T);

/* The finish, two launches.  stats = [ell (S) | G (S*D) | T (S)] as the pass and the all-reduce leave them (NULL is
 * refused); eps in bsc_blr_noise's [S, D+1] layout, column D (tau's noise, Philox stream 1) READ here; W [S, D] and
 * logphi [S] the float32 draws the pass read -- tau_s enters as that float32 value, exactly as w_s does:
 *     g_w    = scale G_s - prior_precision w_s
 *     g_tau  = scale T_s + a0 - b0 e^{tau_s}
 *     ELBO   = mean_s [ scale ell_s - prior_precision/2 |w_s|^2 + log p(tau_s) ] + D/2 log(prior_precision / 2 pi)
 *              + sum rho + P/2 (1 + log 2 pi)
 *     d/d m  = mean_s g_s,     d/d rho_i = mean_s g_si eps_si e^{rho_i} + 1
 * then Adam ascent step t (bsc_adam_ascent's form; lam_in is not modified, m1 and m2 in place) and, when the *_next
 * buffers are set (all or none), W_next [S, D] and logphi_next [S] from eps_next, rounded to float32;
 * eps_next_ready = 0 draws the noise of next_step into eps_next first.  lam_in != lam_out; the *_next buffers must not
 * alias the current ones.  Requires 1 <= S <= 64, t >= 1 and prior_precision, a0, b0, scale > 0.  Fixed-order sums, no
 * atomics. */
int bsc_glm_nb_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                      const double* eps, const float* W, const float* logphi, int32_t D, int32_t S, double scale,
                      double prior_precision, double a0, double b0, int64_t t, double lr, double beta1, double beta2,
                      double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                      float* W_next, float* logphi_next, double* elbo, double* grad);

/* ---- Gamma regression (log link) with a learned shape on the same pass (csrc/bsc_glm_gamma.hip) --------------------
 *
 *      y_n ~ Gamma(shape alpha, rate alpha / mu_n),   y_n > 0,   E y_n = mu_n = exp(l_n),   Var y_n = mu_n^2 / alpha
 *      l[n,s] = sum_d X[n,d] W[s,d] + o[n],   w ~ N(0, I / prior_precision),   alpha = e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  One shape draw rides with
 * every weight draw: logshape[s] = tau_s, float32 [S], any 4-byte alignment; alpha_s = e^{tau_s} (float32 expf of the
 * value read).  With ly = log y, c_a(alpha) = alpha log alpha - lnGamma(alpha), c_1(alpha) = log alpha + 1 - psi(alpha)
 * (both made once per launch in float64 from alpha_s and rounded to float32):
 *      log p(y | l, alpha) = c_a + alpha (ly - l - y e^{-l}) - ly             (the FULL density: nothing is left out)
 *      ell[s]  = sum_n v[n] log p(y[n] | l[n,s], alpha_s)
 *      G[s,d]  = sum_n r[n,s] X[n,d]             r[n,s] = v[n] alpha_s ( y[n] e^{-l[n,s]} - 1 )               (= d / d l)
 *      T[s]    = sum_n v[n] alpha_s ( c_1 + ly[n] - l[n,s] - y[n] e^{-l[n,s]} )                  (= d ell[s] / d tau_s)
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * y = 1, l = 0 whatever it held, as the rows past B are, and log 0 is never formed).  The exponential is taken as the
 * product y e^{-l}, exp and log at full float32 accuracy.
 * y IS NOT CHECKED ON THE DEVICE: a kept row with y <= 0 or a non-finite y makes ell and T of every draw NaN or
 * infinite (bayesic_amd/svi/glm_gamma.py checks y where a batch is set).
 * OVERFLOW: exp is NOT clamped, as for the Poisson link (a clamp would change the gradient silently): the outputs are
 * finite while e^{-l} and y e^{-l} stay below the float32 maximum (l > -88 at y = 1).
 * ACCURACY ENVELOPE: tau in [-2.5, 5] (alpha in [0.08, 148]); there a plain float32 evaluation stays within 1e-6 of
 * sum_n v ( |c_a| + alpha (|ly - l| + y e^{-l}) + |ly| + 1 ) for ell, of sum_n v ( alpha (|c_1| + |ly - l| + y e^{-l}) + 1 )
 * for T and of max |G|.  Above it c_1 -> 1 + 1 / (2 alpha) and T's terms cancel beyond what float32 holds.
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); logshape == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics. */
int bsc_glm_gamma_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                            const float* weight, int64_t B, int32_t D, const float* W, const float* logshape,
                            int32_t S, double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with logshape in the place of logphi -- the prior on e^tau has the same form, the
 * likelihood enters through ell, G and T alone, and both entry points run one body (csrc/bsc_meanfield.h), so the same
 * arguments give the same bits:
 *     g_w = scale G_s - prior_precision w_s,     g_tau = scale T_s + a0 - b0 e^{tau_s}
 *     ELBO = mean_s [ scale ell_s - prior_precision/2 |w_s|^2 + log p(tau_s) ] + D/2 log(prior_precision / 2 pi)
 *            + sum rho + P/2 (1 + log 2 pi)
 * stats = [ell (S) | G (S*D) | T (S)]; checks, next draws and requirements as there. */
int bsc_glm_gamma_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                         double* m2, const double* eps, const float* W, const float* logshape, int32_t D, int32_t S,
                         double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                         double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                         int32_t eps_next_ready, float* W_next, float* logshape_next, double* elbo, double* grad);

/* ---- Beta regression (logit link) with a learned precision on the same pass (csrc/bsc_glm_beta.hip) ----------------
 *
 *      y_n ~ Beta(a_n, b_n),   0 < y_n < 1,   a_n = m_n phi,   b_n = (1 - m_n) phi
 *      m_n = sigmoid(l_n),   E y_n = m_n,   Var y_n = m_n (1 - m_n) / (1 + phi)
 *      l[n,s] = sum_d X[n,d] W[s,d] + o[n],   w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  One precision draw rides
 * with every weight draw: logprec[s] = tau_s, float32 [S], any 4-byte alignment; phi_s = e^{tau_s} (float32 expf of the
 * value read); lnGamma(phi_s) and psi(phi_s) are made once per launch in float64 and rounded.  With ly = log y and
 * l1y = log1p(-y):
 *      log p(y | l, phi) = lnGamma(phi) - lnGamma(a) - lnGamma(b) + (a - 1) ly + (b - 1) l1y   (the FULL density)
 *      ell[s]  = sum_n v[n] log p(y[n] | l[n,s], phi_s)
 *      G[s,d]  = sum_n r[n,s] X[n,d]       r[n,s] = v[n] phi_s m (1 - m) ( (ly - l1y) - psi(a) + psi(b) )       (= d / d l)
 *      T[s]    = sum_n v[n] phi_s ( psi(phi_s) + m (ly - psi(a)) + (1 - m)(l1y - psi(b)) )          (= d ell[s] / d tau_s)
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * y = 1/2, l = 0 whatever it held, as the rows past B are).  m and 1 - m come each from the stable logistic form
 * (e / (1 + e) and 1 / (1 + e), e = exp(-|l|)), never 1 - m by subtraction; lnGamma and psi at a and b are float32, for
 * any positive argument: the argument is shifted up to at least 8 by ONE product of at most eight factors carried with
 * its derivative, then three asymptotic terms (lnGamma = Stirling - log P, psi = asymptotic - P' / P).
 * y IS NOT CHECKED ON THE DEVICE: a kept row with y <= 0, y >= 1 or a non-finite y makes ell and T of every draw NaN or
 * infinite (bayesic_amd/svi/glm_beta.py checks y where a batch is set, AFTER rounding to float32).
 * OVERFLOW: nothing is clamped.  The outputs are finite while m phi, (1 - m) phi and their reciprocals are normal float32
 * values: |l| <= 80 at tau in [-2, 5] (psi(a) ~ -1 / a reaches 4e35 there and is multiplied by m first).
 * ACCURACY ENVELOPE: tau in [-2, 5] (phi in [0.135, 148]), |l| <= 80; there a plain float32 evaluation stays within
 * 1e-6 of  sum_n v ( |lnGamma phi| + S(a) + S(b) + |log min(a, 1)| + |log min(b, 1)| + (a + 1)|ly| + (b + 1)|l1y| + 1 ),
 * S(x) = max(|lnGamma(max(x, 8))|, 17) the shifted Stirling term, for ell, of  sum_n v ( phi (|psi phi| + m (|ly| +
 * |psi a|) + (1 - m)(|l1y| + |psi b|)) + 1 )  for T and of max |G|.  T cancels from its terms' size (2e3 per row at
 * tau = 5) down to O(1): above the envelope float32 does not hold the difference.
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); logprec == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics. */
int bsc_glm_beta_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                           const float* weight, int64_t B, int32_t D, const float* W, const float* logprec, int32_t S,
                           double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with logprec in the place of logphi -- the prior on e^tau has the same form, the
 * likelihood enters through ell, G and T alone, and both entry points run one body (csrc/bsc_meanfield.h), so the same
 * arguments give the same bits.  stats = [ell (S) | G (S*D) | T (S)]; checks, next draws and requirements as there.
 * A full-covariance guide finishes with bsc_glm_scalar_fullrank_update. */
int bsc_glm_beta_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                        double* m2, const double* eps, const float* W, const float* logprec, int32_t D, int32_t S,
                        double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                        double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                        int32_t eps_next_ready, float* W_next, float* logprec_next, double* elbo, double* grad);

/* ---- Weibull survival regression with right censoring and a learned shape on the same pass (csrc/bsc_glm_weibull.hip)
 *
 *      t_n ~ Weibull(shape k, scale e^{l_n}),   l[n,s] = sum_d X[n,d] W[s,d] + o[n]   (accelerated failure time)
 *      w ~ N(0, I / prior_precision),   k = e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  One shape draw rides with
 * every weight draw: logshape[s] = tau_s, float32 [S], any 4-byte alignment; k_s = e^{tau_s} (float32 expf of the value
 * read).  l is the log SCALE, not the log mean: E t = e^l Gamma(1 + 1/k), Var t = e^{2l} (Gamma(1 + 2/k) -
 * Gamma(1 + 1/k)^2).
 * ENCODING: the censoring flag of a row is the SIGN of y (a duration is positive, so the sign is free and the pass reads
 * no new vector):  y[n] > 0 is an event seen at y[n];  y[n] < 0 is right-censored at -y[n] (the event is later);
 * 0, NaN and +-infinity are invalid.  With delta = (y > 0), t = |y|, ly = log t and z = k (ly - l):
 *      log f(t) = tau + z - ly - e^z        log S(t) = -e^z              (the FULL density: nothing is left out)
 *      ell[s]  = sum_n v[n] ( delta[n] (tau_s + z[n,s] - ly[n]) - e^{z[n,s]} )
 *      G[s,d]  = sum_n r[n,s] X[n,d]             r[n,s] = v[n] k_s ( e^{z[n,s]} - delta[n] )                   (= d / d l)
 *      T[s]    = sum_n v[n] ( delta[n] (1 + z[n,s]) - z[n,s] e^{z[n,s]} )                        (= d ell[s] / d tau_s)
 * At k = 1 with every row an event ell and G are bsc_glm_gamma_data_pass's at alpha = 1 (T is not).
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * t = 1, l = 0, delta = 0 whatever it held -- 0 and NaN included -- as the rows past B are).
 * y IS NOT CHECKED ON THE DEVICE: a kept row with y = 0 or a non-finite y makes ell and T of every draw NaN or infinite
 * (bayesic_amd/svi/glm_weibull.py checks time and event where a batch is set).
 * OVERFLOW: exp is NOT clamped, as for the Poisson and Gamma links (a clamp would change the gradient silently): the
 * outputs are finite while z = k (log t - l) stays below about 88 (e^z and z e^z below the float32 maximum).
 * ACCURACY ENVELOPE: tau in [-2, 4] (k in [0.14, 55]).  z is rounded to float32 before the exponential, which costs
 * |z| eps of e^z, and z inherits the rounding of k, ly and l: with c = |z| + k (|ly| + sum_d |x_d w_d| + |o|) a plain
 * float32 evaluation stays within 1e-6 of sum_n v ( delta (|tau| + |z| + |ly| + c) + (1 + c) e^z + 1 ) for ell, of
 * sum_n v ( delta (1 + |z| + c) + (|z| + (1 + |z|) c) e^z + 1 ) for T and of sum_n v k ( (1 + c) e^z + delta ) |x_d| for
 * G[., d].
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); logshape == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics. */
int bsc_glm_weibull_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                              const float* weight, int64_t B, int32_t D, const float* W, const float* logshape,
                              int32_t S, double* ell, double* G, double* T);

/* bsc_glm_weibull_data_pass with INTERVAL and LEFT censoring (csrc/bsc_glm_weibull_interval.hip): one more per-row
 * vector, upper [B] float32 (contiguous, 4-byte aligned), next to the signed y.
 * ENCODING:  upper[n] == 0              the row is exactly what y[n] says above (an event, or right-censored)
 *            upper[n] >  0, y[n] < 0    interval-censored: the event lies in (a, b] = (-y[n], upper[n]];  b > a is required
 *            upper[n] <  0              left-censored: the event is at or before b = -upper[n]; the magnitude of y[n] is
 *                                       NOT read on such a row (bayesic_amd/svi/glm_weibull.py stores y[n] = upper[n])
 * so a vector of zeros is bsc_glm_weibull_data_pass's model, and the rows past B read upper = 0 through the descriptor.
 * With la = log a, d = log b - la, z_a = k (la - l), E_a = e^{z_a}, Delta = E_b - E_a formed as E_a expm1(k d) (a narrow
 * interval does not cancel) and E_b = E_a + Delta, an interval row adds, times v[n],
 *      ell:  log P = -E_a + log(-expm1(-Delta))                       (= log(S(a) - S(b)): nothing is left out)
 *      r:    k ( E_a - Delta / expm1(Delta) )                         (= d / d l;  Delta / expm1(Delta) lies in (0, 1))
 *      T:    -z_a E_a + ( z_a Delta + k d E_b ) / expm1(Delta)         (= d / d tau)
 * and a left-censored row the same with E_a = 0, z_a E_a = 0 and Delta = E_b = e^{k (log b - l)}:
 *      ell:  log(-expm1(-E_b))        r:  -k E_b / expm1(E_b)        T:  z_b E_b / expm1(E_b)
 * Event rows and right-censored rows keep the expressions above.  1 / expm1(Delta) is formed as e^{-Delta} / (1 -
 * e^{-Delta}), expm1 from the full-accuracy exp and log (Kahan's quotient below 1/2): seven transcendentals per (row,
 * draw) where the pass above has two.
 * OVERFLOW RULE: where Delta >= 103 -- e^{-Delta} is zero in float32 (103 is one denormal step short of it) -- or where
 * e^{k d} or Delta is infinite in float32, the upper end is taken as ABSENT: the row adds the right-censored row's values
 * at a, finite (a left-censored row adds nothing: its probability is 1), by a select on the link's inputs.  upper = 1e30
 * is therefore a valid way to write "no bound".  An interval with k d > 88 is always read this way, whatever z_a.  Apart
 * from that exp is NOT clamped: finite while z_a stays below about 88.  A kept row whose Delta underflows to 0 (z_a below
 * -103) has probability 0 in float32: ell = -infinity, and G and T of that draw are NaN (1 / expm1(0) times 0); such a
 * row is the caller's to keep out, like y = 0 above.
 * A row with v[n] = 0, and every row past B, is evaluated at a = b = 1, l = 0 as an uncensored row of weight 0, whatever y
 * and upper hold there (0, NaN and infinity included), and adds EXACTLY nothing.  y and upper ARE NOT CHECKED ON THE
 * DEVICE (bayesic_amd/svi/glm_weibull.py checks them where a batch is set).
 * ACCURACY ENVELOPE: tau in [-2, 4], as above.  A plain float32 evaluation stays within 1e-6 of the sums of the
 * magnitudes of the terms with the conditioning of z_a, k d and Delta on their rounded inputs (spelled out in
 * tests/_glm_weibull_interval_ref.py), the device within 2e-5.  d = log b - log a is formed as log1p((b - a) / a) where
 * b < 2 a (b - a is exact there), so that a narrow interval keeps its digits.
 * upper == NULL: the kernels of bsc_glm_weibull_data_pass, bit for bit.  The envelope and the refusals are that entry
 * point's; upper must be 4-byte aligned, and counts among the vectors whose 16-byte alignment decides the MFMA route.
 * Outputs, determinism and the slab as there; the finishes are shared (they see ell, G and T alone). */
int bsc_glm_weibull_data_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                       const float* offset, const float* weight, int64_t B, int32_t D, const float* W,
                                       const float* logshape, int32_t S, double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with logshape in the place of logphi -- the prior on e^tau has the same form, the
 * likelihood enters through ell, G and T alone, and the entry points run one body (csrc/bsc_meanfield.h), so the same
 * arguments give the same bits as bsc_glm_nb_update and bsc_glm_gamma_update.  stats = [ell (S) | G (S*D) | T (S)];
 * checks, next draws and requirements as there. */
int bsc_glm_weibull_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                           double* m2, const double* eps, const float* W, const float* logshape, int32_t D, int32_t S,
                           double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                           double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                           double* eps_next, int32_t eps_next_ready, float* W_next, float* logshape_next, double* elbo,
                           double* grad);

/* ---- Log-normal survival regression with right censoring and a learned scale on the same pass
 * (csrc/bsc_glm_lognormal.hip)
 *
 *      t_n ~ LogNormal(location l_n, scale sigma),   l[n,s] = sum_d X[n,d] W[s,d] + o[n]   (accelerated failure time)
 *      w ~ N(0, I / prior_precision),   k = 1 / sigma = e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  tau is the log of the
 * INVERSE scale, so that the prior on e^tau has the form the shared finish knows.  One draw of it rides with every weight
 * draw: loginvscale[s] = tau_s, float32 [S], any 4-byte alignment; k_s = e^{tau_s} (float32 expf of the value read).  l is
 * the location of log t (the log median), not the log mean: E t = e^{l + sigma^2 / 2}, Var t = (e^{sigma^2} - 1)
 * e^{2l + sigma^2}.  The model next to bsc_glm_weibull_data_pass's: its hazard rises and falls where the Weibull one is
 * monotone.
 * ENCODING: bsc_glm_weibull_data_pass's.  The censoring flag of a row is the SIGN of y:  y[n] > 0 is an event seen at
 * y[n];  y[n] < 0 is right-censored at -y[n] (the event is later);  0, NaN and +-infinity are invalid.  With
 * delta = (y > 0), t = |y|, ly = log t, z = k (ly - l), Phi and phi the standard normal distribution function and density
 * and h(z) = phi(z) / Phi(-z) the normal hazard:
 *      log f(t) = tau - ly - z^2 / 2 - log(2 pi) / 2        log S(t) = log Phi(-z)        (the FULL density)
 *      ell[s]  = sum_n v[n] ( delta[n] (tau_s - ly[n] - z[n,s]^2 / 2 - log(2 pi) / 2) + (1 - delta[n]) log Phi(-z[n,s]) )
 *      G[s,d]  = sum_n r[n,s] X[n,d]        r[n,s] = v[n] k_s ( delta[n] z[n,s] + (1 - delta[n]) h(z[n,s]) )     (= d / d l)
 *      T[s]    = sum_n v[n] ( delta[n] (1 - z[n,s]^2) - (1 - delta[n]) z[n,s] h(z[n,s]) )          (= d ell[s] / d tau_s)
 * With every row an event this is the Gaussian regression of log t.
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * t = 1, l = 0, delta = 0 whatever it held -- 0 and NaN included -- as the rows past B are).
 * log Phi(-z) and h(z) are float32, per (row, draw), from ONE scaled complementary error function E = erfcx(|z| / sqrt 2)
 * in (0, 1] (a degree-11 polynomial on the half line, within 2 roundings): for z >= 0, log Phi(-z) = -z^2 / 2 + log(E / 2)
 * and h = sqrt(2 / pi) / E; for z < 0, with q = e^{-z^2 / 2} E / 2, log Phi(-z) = log1p(-q) and h = phi(z) / (1 - q).
 * Neither tail cancels or overflows: log Phi(-60) = -1805.01 with h = 60.02, log Phi(60) = -0 with h = 0.
 * y IS NOT CHECKED ON THE DEVICE: a kept row with y = 0 or a non-finite y makes ell and T of every draw NaN or infinite
 * (bayesic_amd/svi/glm_lognormal.py checks time and event where a batch is set).
 * OVERFLOW: nothing is clamped and nothing needs to be: every term is finite for every finite z whose square is
 * (|z| < 1.8e19); bsc_glm_weibull_data_pass's z < 88 does not apply.
 * ACCURACY ENVELOPE: tau in [-1.5, 4] (sigma from 4.5 down to 0.018; the lower end is the predictive variance's, see
 * bsc_lognormal_predict_pass).  z inherits the rounding of k, ly and l: with c = |z| + k (|ly| + sum_d |x_d w_d| + |o|) a
 * plain float32 evaluation stays within 1e-6 of
 *      sum_n v ( delta (|tau| + |ly| + z^2 / 2 + |z| c + 1) + (1 - delta)(|log Phi(-z)| + h c + 1) )           for ell,
 *      sum_n v ( delta (1 + z^2 + 2 |z| c) + (1 - delta)(|z| h + (h + |z| h |h - z|) c) + 1 )                   for T,
 *      sum_n v k ( delta (|z| + c) + (1 - delta) h (1 + |h - z| c) ) |x_d|                                      for G[., d]
 * (h' = h (h - z)), |z| = 60 in both tails included, and the device within 2e-5.
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); loginvscale == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics.
 * Not built: interval and left censoring (no `upper`), left truncation, random intercepts. */
int bsc_glm_lognormal_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                                const float* weight, int64_t B, int32_t D, const float* W, const float* loginvscale,
                                int32_t S, double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with loginvscale in the place of logphi -- the prior on e^tau = 1 / sigma has the same
 * form, the likelihood enters through ell, G and T alone, and the entry points run one body (csrc/bsc_meanfield.h), so
 * the same arguments give the same bits as bsc_glm_nb_update.  stats = [ell (S) | G (S*D) | T (S)]; checks, next draws
 * and requirements as there.  A full-covariance guide finishes with bsc_glm_scalar_fullrank_update. */
int bsc_glm_lognormal_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                             double* m2, const double* eps, const float* W, const float* loginvscale, int32_t D,
                             int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                             double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                             double* eps_next, int32_t eps_next_ready, float* W_next, float* loginvscale_next,
                             double* elbo, double* grad);

/* ---- Zero-inflated Poisson regression with a learned inflation odds on the same pass (csrc/bsc_glm_zip.hip)
 *
 *      y_n ~ ZIP(pi, mu_n): with probability pi a structural zero, else Poisson(mu_n)
 *      mu_n = e^{l_n},   l[n,s] = sum_d X[n,d] W[s,d] + o[n]          (offset or log exposure, as in the Poisson route)
 *      w ~ N(0, I / prior_precision),   omega = pi / (1 - pi) = e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  tau is the log ODDS of a
 * structural zero, pi = sigmoid(tau), so that the prior on e^tau has the form the shared finish knows.  One draw of it
 * rides with every weight draw: logodds[s] = tau_s, float32 [S], any 4-byte alignment.  Per draw L1 = log1p(omega) =
 * softplus(tau_s) and pi = sigmoid(tau_s) are made once per launch in float64 from the value read and rounded.  With
 * u = tau + mu and the branch of a row chosen by y == 0:
 *                   y == 0                                                   y > 0
 *      log p        max(tau, -mu) + log1p(e^{-|u|}) - L1                      y l - mu - L1
 *      d / d l      -mu sigmoid(-u)                                           y - mu
 *      d / d tau    sigmoid(u) (1 - pi) (1 - e^{-mu})                         -pi
 *      ell[s]  = sum_n v[n] log p        G[s,d] = sum_n r[n,s] X[n,d],  r = v d / d l        T[s] = sum_n v[n] d / d tau
 * The zero branch is log(omega + e^{-mu}) - log1p(omega); softplus(u) - mu is never formed.  sigmoid(-u) is the
 * probability that a zero came from the Poisson part.  sigmoid(u) and sigmoid(-u) each come from the stable logistic
 * form on e^{-|u|}; the tau derivative of a zero row is the product above (= sigmoid(u) - sigmoid(tau), which would cancel
 * at small mu), never negative; 1 - e^{-mu} through expm1.  The positive branch leaves the row constant -lnGamma(y + 1)
 * out, as bsc_glm_data_pass(BSC_GLM_POISSON) and bsc_glm_nb_data_pass do.
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * y = 0, l = 0 whatever it held -- NaN, infinity and negative values included -- as the rows past B are).
 * y IS NOT CHECKED ON THE DEVICE: a kept row with a negative or non-finite y is read as a positive count
 * (bayesic_amd/svi/glm_zip.py checks y finite, >= 0 and whole where a batch is set).
 * OVERFLOW: nothing is clamped, like the Poisson link: every term is finite while e^l is (l <= 88).  At l = +80 a zero
 * row gives exactly log p = tau - L1 (= log pi), d / d l = 0 and d / d tau = 1 - pi; at l = -80 every term is finite (a zero row's
 * log p is -(1 - pi) mu to first order, within a rounding of L1 of 0; a positive row's is y l - L1).
 * ACCURACY: a plain float32 evaluation stays within 1e-6, and the device within 2e-5, of
 *      sum_n v ( |tau| + mu + L1 + |y l| + 1 )          for ell,
 *      sum_n v ( |d / d tau| + pi + 1 )                  for T,
 *      sum_n v ( y + (1 + a) mu r + a mu^2 r (1 - r) [y == 0] ) |x_d|                        for G[., d]
 * (a = sum_d |x_d w_d| + |o| the size of the logit's float32 terms; r = sigmoid(-u) on a zero row and 1 on a positive
 * one, so that mu r is the size of the residual's second term and the rest its conditioning on l) over tau in [-8, 8]
 * and l in [-80, 80].
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); logodds == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics.
 * Not built: covariates on the zero share, a zero-inflated negative binomial, hurdle models, random intercepts. */
int bsc_glm_zip_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                          const float* weight, int64_t B, int32_t D, const float* W, const float* logodds, int32_t S,
                          double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with logodds in the place of logphi -- the prior on e^tau = pi / (1 - pi) has the same
 * form, the likelihood enters through ell, G and T alone, and the entry points run one body (csrc/bsc_meanfield.h), so
 * the same arguments give the same bits as bsc_glm_nb_update.  stats = [ell (S) | G (S*D) | T (S)]; checks, next draws
 * and requirements as there.  A full-covariance guide finishes with bsc_glm_scalar_fullrank_update. */
int bsc_glm_zip_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                       double* m2, const double* eps, const float* W, const float* logodds, int32_t D, int32_t S,
                       double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                       double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                       int32_t eps_next_ready, float* W_next, float* logodds_next, double* elbo, double* grad);

/* ---- Student-t robust regression with a learned scale and fixed degrees of freedom on the same pass
 * (csrc/bsc_glm_studentt.hip)
 *
 *      y_n ~ StudentT(df = nu, location l_n, scale sigma),   l[n,s] = sum_d X[n,d] W[s,d] + o[n]
 *      w ~ N(0, I / prior_precision),   k = 1 / sigma = e^tau ~ Gamma(a0, b0),   nu = df > 0 fixed by the caller
 * The latent is z = [w (D) | tau], P = D + 1, the guide mean-field: lam = [m (P) | rho (P)].  tau is the log of the
 * INVERSE scale, as in bsc_glm_lognormal_data_pass, so that the prior on e^tau has the form the shared finish knows.  One
 * draw of it rides with every weight draw: loginvscale[s] = tau_s, float32 [S], any 4-byte alignment; k_s = e^{tau_s}
 * (float32 expf of the value read).  y is any finite float.  With z = k (y - l) and
 * c_nu = lnGamma((nu + 1) / 2) - lnGamma(nu / 2) - log(nu pi) / 2:
 *      log p   = tau + c_nu - ((nu + 1) / 2) log1p(z^2 / nu)                                     (the FULL density)
 *      ell[s]  = sum_n v[n] log p(y[n] | l[n,s], k_s)
 *      G[s,d]  = sum_n r[n,s] X[n,d]        r[n,s] = v[n] k_s (nu + 1) z[n,s] / (nu + z[n,s]^2)                  (= d / d l)
 *      T[s]    = sum_n v[n] nu (1 - z[n,s]^2) / (nu + z[n,s]^2)                              (= d ell[s] / d tau_s)
 * The residual is BOUNDED in z (k (nu + 1) / (2 sqrt nu) at most, at z^2 = nu): one gross outlier cannot move the fit as
 * far as it likes, which it can under the Gaussian likelihood, the limit nu -> infinity of this one.
 * df: the degrees of freedom, finite and > 0 (BSC_ERR_INVALID otherwise, the message naming the entry point); the kernels
 * take it rounded to float32, and c_nu is made once per launch in float64 from the rounded value and added to tau_s there,
 * so the density is normalised for the nu the link uses.  It is read at every call: two calls on one context may differ
 * in it.
 * Outputs float64: ell [S], G [S, D], T [S].  offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0,
 * v = 1; a row with v[n] = 0 adds EXACTLY nothing to ell, G and T, by a select on the link's inputs: it is evaluated at
 * y = 0, l = 0 whatever it held -- NaN and infinity included -- as the rows past B are).
 * log1p(r), r = z^2 / nu, is log(t) r / (t - 1) with t = 1 + r (r itself where t == 1): the quotient undoes the rounding
 * of t, so at nu = 1e6, where r = 1e-6 z^2 and ((nu + 1) / 2) log1p(r) = z^2 / 2, every digit is kept.
 * y IS NOT CHECKED ON THE DEVICE: a kept row with a non-finite y makes ell, G and T of every draw NaN
 * (bayesic_amd/svi/glm_studentt.py checks y where a batch is set).
 * OVERFLOW: nothing is clamped and nothing needs to be: every term is finite while z^2 is (|z| < 1.8e19).
 * ACCURACY: z inherits the rounding of k, y and l: with a = sum_d |x_d w_d| + |o| and c = |z| + k (|y| + a) a plain
 * float32 evaluation stays within 1e-6, and the device within 2e-5, of
 *      sum_n v ( |tau| + |c_nu| + ((nu + 1) / 2) log1p(z^2 / nu) + (nu + 1) |z| c / (nu + z^2) + 1 )              for ell,
 *      sum_n v ( nu |1 - z^2| / (nu + z^2) + 2 nu (nu + 1) |z| c / (nu + z^2)^2 + 1 )                             for T,
 *      sum_n v k (nu + 1) ( |z| + c |nu - z^2| / (nu + z^2) ) / (nu + z^2) |x_d|                                 for G[., d]
 * (each derivative's size times c) over tau in [-3, 5], nu from 1 to 1e6 and |z| from 1e-3 to 1e4 and beyond.  Where the
 * data are many sigma away from 0 (k |y| large against |z|) the term in c is the whole bound: y - l cancels.
 * The envelope and its refusals are bsc_glm_nb_data_pass's (D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64 with eight draws
 * and their eight tau per launch, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26); loginvscale == NULL is
 * refused.  The 16-row MFMA kernel (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned,
 * else the 8-row kernel.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block partials of
 * 8 * 256 + 16 floats (ell and T behind G), fixed-order float64 finish, no float atomics.
 * Not built: a learned nu, random intercepts, a one-call pass + finish form. */
int bsc_glm_studentt_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                               const float* weight, int64_t B, int32_t D, const float* W, const float* loginvscale,
                               int32_t S, double df, double* ell, double* G, double* T);

/* The finish: bsc_glm_nb_update with loginvscale in the place of logphi -- the prior on e^tau = 1 / sigma has the same
 * form, the likelihood enters through ell, G and T alone, and the entry points run one body (csrc/bsc_meanfield.h), so
 * the same arguments give the same bits as bsc_glm_nb_update.  The finish never sees nu.  stats = [ell (S) | G (S*D) |
 * T (S)]; checks, next draws and requirements as there.  A full-covariance guide finishes with
 * bsc_glm_scalar_fullrank_update. */
int bsc_glm_studentt_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, const float* loginvscale, int32_t D,
                            int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                            double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                            double* eps_next, int32_t eps_next_ready, float* W_next, float* loginvscale_next,
                            double* elbo, double* grad);

/* The finish of bsc_glm_update for a FULL-COVARIANCE Gaussian guide (csrc/bsc_glm_full.hip; full-rank ADVI, Kucukelbir
 * et al.): q(w) = N(mu, L L^T) over w in R^D (no scalar latent: P = D), L lower-triangular with L_ii = e^{rho_i}.
 *     lam = [mu (D) | L packed row-major, lower triangle incl. the diagonal (D(D+1)/2)]
 * row i of L starts at lam[D + i(i+1)/2] and its diagonal slot holds rho_i (33 152 doubles at D = 256): the layout of
 * bsc_blr_fullrank_update with P = D; m1, m2 and grad have lam's layout.  Same model, scale and prior_precision (tau)
 * as bsc_glm_update; per update, with eps_s in bsc_blr_noise's [S, D+1] layout (column D is not read) and W_s the
 * float32-rounded draws the pass read:
 *     g_s  = scale G_s - tau W_s
 *     ELBO = mean_s [scale ell_s - tau/2 |w_s|^2] + D/2 log(tau / 2 pi) + sum_i rho_i + D/2 (1 + log 2 pi)
 *     d / d mu = mean_s g_s,   d / d L_ij = mean_s g_si eps_sj (j < i),   d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
 * then Adam ascent on every entry (bsc_glm_update's hyper-parameters and bias correction; lam_in is not modified) and,
 * when the *_next buffers are set, the next draw w'_s = mu' + L' eps'_s rounded to float32 into W_next [S, D].
 * eps_next_ready = 0: the noise of next_step is drawn into eps_next first (one bsc_blr_noise launch).  With every
 * off-diagonal entry zero the ELBO, the mu / rho gradients and their Adam step equal bsc_glm_update's on the same
 * stats and noise.
 * stats = [ell (S) | G (S*D)] as bsc_glm_data_pass and the all-reduce leave them (NULL is refused: pending pass
 * partials are not read).  One launch of D / 2 workgroups, workgroup k owning rows k and D - 1 - k of L; fixed-order
 * sums, no atomics: reproducible bit for bit.  The caller double-buffers lam and the draws: lam_in != lam_out, and
 * *_next (both set or both NULL) must not alias eps / W.
 * Requires D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64, t >= 1, prior_precision > 0, scale > 0. */
int bsc_glm_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, int32_t D, int32_t S, double scale,
                            double prior_precision, int64_t t, double lr, double beta1, double beta2, double adam_eps,
                            uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                            double* elbo, double* grad);

/* The finish of bsc_glm_nb_update / bsc_glm_gamma_update / bsc_glm_weibull_update for a FULL-COVARIANCE Gaussian guide
 * (csrc/bsc_glm_scalar_full.hip): q(z) = N(mu, L L^T) over z = [w (D) | tau], P = D + 1, L lower-triangular with
 * L_ii = e^{rho_i}.
 *     lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal (P(P+1)/2)]
 * row i of L starts at lam[P + i(i+1)/2] and its diagonal slot holds rho_i (33 410 doubles at D = 256): the layout of
 * bsc_blr_fullrank_update; m1, m2 and grad have lam's layout.  ONE entry point for the three families: the likelihood
 * enters through stats = [ell (S) | G (S*D) | T (S)] alone (NULL is refused), as the pass of any of them and the
 * all-reduce leave them.  Arguments and their order are bsc_glm_nb_update's; logscalar [S] is the float32 tau_s the
 * pass read (logphi, logshape), eps in bsc_blr_noise's [S, D+1] layout with EVERY column read, W the float32 draws:
 *     g_si = scale G_si - prior_precision W_si  (i < D),     g_sD = scale T_s + a0 - b0 e^{tau_s}
 *     ELBO = mean_s [ scale ell_s - prior_precision/2 |w_s|^2 + a0 tau_s - b0 e^{tau_s} ]
 *            + D/2 log(prior_precision / 2 pi) + a0 log b0 - lnGamma(a0) + sum_i rho_i + P/2 (1 + log 2 pi)
 *            (the mean-field finishes' quantity)
 *     d / d mu = mean_s g_s,   d / d L_ij = mean_s g_si eps_sj (j < i),
 *     d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
 * then Adam ascent on every entry (lam_in is not modified, m1 and m2 in place) and, when the *_next buffers are set
 * (all or none), the next draw z'_s = mu' + L' eps'_s rounded to float32 into W_next [S, D] and logscalar_next [S].
 * eps_next_ready = 0: the noise of next_step is drawn into eps_next first (one bsc_blr_noise launch).  With every
 * off-diagonal entry zero the ELBO, the mu / rho gradients and their Adam step equal bsc_glm_nb_update's on the same
 * stats and noise (rtol 1e-12: two sums run in another order).
 * One launch of D / 2 + 1 workgroups, workgroup k owning rows k and D - k of L (row D / 2 alone); fixed-order sums, no
 * atomics: reproducible bit for bit.  lam_in != lam_out, and *_next must not alias eps / W / logscalar.
 * Requires D % 4 == 0, 4 <= D <= 256, 1 <= S <= 64, t >= 1 and prior_precision, a0, b0, scale > 0. */
int bsc_glm_scalar_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                                   double* m2, const double* eps, const float* W, const float* logscalar, int32_t D,
                                   int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t,
                                   double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                                   uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                                   float* logscalar_next, double* elbo, double* grad);

/* ---- posterior predictive and held-out log density (csrc/bsc_predict.hip; ABSENT in the reference) ---------
 *
 * One streaming pass over X[B,D] (row-major, leading dimension ldx floats) for S draws W[S,D] of a fitted q.  With
 * l[n,s] = sum_d X[n,d] W[s,d], per draw
 *      family                   mu(l)      v(l)             log p(y | l)
 *      BSC_PREDICT_GAUSSIAN     l          exp(logvar[s])   -1/2 (logvar[s] + log 2 pi) - 1/2 exp(-logvar[s]) (y - l)^2
 *      BSC_PREDICT_LOGISTIC     sigmoid    mu (1 - mu)      y l - softplus(l)        (stable: finite at l = +-80)
 *      BSC_PREDICT_POISSON      exp(l)     mu               y l - exp(l) - lnGamma(y + 1)     (exp not clamped)
 * and per row (each output may be NULL; float32 [B])
 *      mean[n] = 1/S sum_s mu(l[n,s])
 *      var[n]  = 1/S sum_s v(l[n,s]) + 1/S sum_s (mu(l[n,s]) - mean[n])^2      (squares taken about the mean)
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s]) - log S                       (maximum subtracted; needs y)
 *      lpd_sum = sum_n lpd[n]                                                   (float64 [1]; needs y)
 * The Poisson constant lnGamma(y + 1) IS included (bsc_glm_data_pass leaves it out of ell): a held-out score is
 * compared across models.  X is read once for every S.  Draws come from bayesic_amd/svi/predict.py (Philox stream 2;
 * training uses streams 0 and 1).
 * Argument errors (BSC_ERR_INVALID): unknown family, a NULL X (B > 0) or W, no output requested, lpd or lpd_sum
 * without y, the Gaussian family without logvar.  Outside the envelope (BSC_ERR_UNSUPPORTED, outputs untouched):
 * D % 4 != 0 or D outside [4, 256], S outside [1, 64], X or W not 16-byte aligned, ldx < D, ldx % 4 != 0,
 * ldx >= 2^26.  y is contiguous with any 4-byte alignment.  B = 0 writes lpd_sum = 0 and nothing else.
 * Deterministic: fixed partition, float64 block partials of lpd in the workspace (pending pass partials of
 * bsc_blr_data_pass_partial are dropped), fixed-order float64 finish, no float atomics. */
#define BSC_PREDICT_GAUSSIAN 0
#define BSC_PREDICT_LOGISTIC 1
#define BSC_PREDICT_POISSON 2
int bsc_predict_pass(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                     const float* W, const float* logvar, int32_t S, float* mean, float* var, float* lpd,
                     double* lpd_sum);

/* bsc_predict_pass with a per-row offset o[B] (csrc/bsc_predict_offset.hip; float32, contiguous, any 4-byte
 * alignment) for the logistic and the Poisson family: l[n,s] = sum_d X[n,d] W[s,d] + o[n], everything else as above
 * (a model fitted with bsc_glm_data_pass_obs's offset predicts with the same one: o[n] = log exposure[n] gives the
 * expected COUNT of row n, not its rate).  offset == NULL: bsc_predict_pass, bit for bit.  BSC_PREDICT_GAUSSIAN with
 * a non-NULL offset is BSC_ERR_INVALID.  Row weights need no pass of their own: a weighted score is sum_n v[n] lpd[n]
 * over the lpd vector. */
int bsc_predict_pass_offset(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                            const float* offset, int64_t B, int32_t D, const float* W, const float* logvar, int32_t S,
                            float* mean, float* var, float* lpd, double* lpd_sum);

/* The predictive of the negative-binomial model (csrc/bsc_glm_nb.hip: bsc_predict_pass's kernel with a fourth family
 * that only this entry point reaches; bsc_predict_pass and bsc_predict_pass_offset refuse it).  Per draw, with
 * phi_s = exp(logphi[s]) and l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset may be NULL):
 *      mu = exp(l)    v = mu + mu^2 / phi_s    log p(y | l, phi_s) = the full log-pmf, -lnGamma(y + 1) included
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s (mu + mu^2 / phi_s) + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], phi_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * lpd comes from the softplus form (bsc_glm_nb_data_pass) and is finite for every finite l.  exp is NOT clamped, as for
 * the Poisson family: mean stops being finite at l > 88 and var at l > 44 (mu^2 overflows float32).  Outputs, refusals,
 * envelope and determinism are bsc_predict_pass_offset's; logphi == NULL is BSC_ERR_INVALID.  Accuracy envelope of
 * lpd: logphi in [-2.5, 5]. */
int bsc_nb_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                        int32_t D, const float* W, const float* logphi, int32_t S, float* mean, float* var, float* lpd,
                        double* lpd_sum);

/* The predictive of the Gamma model (csrc/bsc_glm_gamma.hip: bsc_predict_pass's kernel with a fifth family that only
 * this entry point reaches).  Per draw, with alpha_s = exp(logshape[s]) and l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset
 * may be NULL):
 *      mu = exp(l)    v = mu^2 / alpha_s    log p(y | l, alpha_s) = c_a + alpha_s (log y - l - y e^{-l}) - log y
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s mu^2 / alpha_s + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], alpha_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * The density is bsc_glm_gamma_data_pass's, complete.  exp is NOT clamped: mean stops being finite at l > 88, var at
 * l > 44, lpd where y e^{-l} overflows; y > 0 is not checked here.  Outputs, refusals, envelope and determinism are
 * bsc_nb_predict_pass's; logshape == NULL is BSC_ERR_INVALID.  Accuracy envelope of lpd: logshape in [-2.5, 5]. */
int bsc_gamma_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                           int32_t D, const float* W, const float* logshape, int32_t S, float* mean, float* var,
                           float* lpd, double* lpd_sum);

/* The predictive of the Beta model (csrc/bsc_glm_beta.hip: bsc_predict_pass's kernel with an eighth family that only
 * this entry point reaches).  Per draw, with phi_s = exp(logprec[s]), l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset may be
 * NULL), m = sigmoid(l), a = m phi_s and b = (1 - m) phi_s:
 *      mu = m    v = m (1 - m) / (1 + phi_s)
 *      log p(y | l, phi_s) = lnGamma(phi_s) - lnGamma(a) - lnGamma(b) + (a - 1) log y + (b - 1) log1p(-y)
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s v + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], phi_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * The density is bsc_glm_beta_data_pass's, complete, in its forms; lnGamma(phi_s) and 1 / (1 + phi_s) are made once per
 * launch in float64.  mean and var are finite for every finite l; 0 < y < 1 is not checked here.  Outputs, refusals,
 * envelope and determinism are bsc_nb_predict_pass's; logprec == NULL is BSC_ERR_INVALID.  Accuracy envelope of lpd:
 * logprec in [-2, 5], |l| <= 80. */
int bsc_beta_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                          int32_t D, const float* W, const float* logprec, int32_t S, float* mean, float* var,
                          float* lpd, double* lpd_sum);

/* The predictive of the Weibull survival model (csrc/bsc_glm_weibull.hip: bsc_predict_pass's kernel with a sixth family
 * that only this entry point reaches).  y carries bsc_glm_weibull_data_pass's encoding: y[n] > 0 an event at y[n],
 * y[n] < 0 right-censored at -y[n].  Per draw, with k_s = exp(logshape[s]), l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset
 * may be NULL), t = |y| and z = k_s (log t - l):
 *      mu = e^l Gamma(1 + 1/k_s)        v = e^{2l} ( Gamma(1 + 2/k_s) - Gamma(1 + 1/k_s)^2 )
 *      log p(y | l, k_s) = tau_s + z - log t - e^z   (y > 0: the density)        = -e^z   (y < 0: the log survival)
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s v + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], k_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * The lpd of a censored row is therefore the log of the posterior-predictive survival probability at that time, and a
 * batch with every row censored at t_n gives log S(t_n | x_n).  Both special values are made once per launch in float64
 * and rounded.  exp is NOT clamped: mean stops being finite at l > 88, var at l > 44, lpd where z > 88; y = 0 is not
 * checked here.  FLOAT32 ENVELOPE OF THE MOMENTS: Gamma(1 + 2/k) overflows float32 near k = 0.06; accuracy envelope
 * logshape in [-2, 4].  Outputs, refusals, envelope and determinism are bsc_nb_predict_pass's; logshape == NULL is
 * BSC_ERR_INVALID. */
int bsc_weibull_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                             int32_t D, const float* W, const float* logshape, int32_t S, float* mean, float* var,
                             float* lpd, double* lpd_sum);

/* bsc_weibull_predict_pass with bsc_glm_weibull_data_pass_interval's upper [B] (csrc/bsc_glm_weibull_interval.hip): the
 * same encoding, forms and overflow rule.  mean and var do not depend on the row's kind.  For an interval or left-censored
 * row log p(y | l, k_s) = -E_a + log(-expm1(-Delta)) is the log of the row's PROBABILITY under draw s, so lpd[n] is the log
 * of the draw average of that probability (the same log-mean-exp).  upper == NULL: bsc_weibull_predict_pass, bit for bit.
 * upper must be 4-byte aligned; everything else as there. */
int bsc_weibull_predict_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                      const float* offset, int64_t B, int32_t D, const float* W, const float* logshape,
                                      int32_t S, float* mean, float* var, float* lpd, double* lpd_sum);

/* The predictive of the log-normal survival model (csrc/bsc_glm_lognormal.hip: bsc_predict_pass's kernel with a family
 * that only this entry point reaches).  y carries bsc_glm_lognormal_data_pass's encoding: y[n] > 0 an event at y[n],
 * y[n] < 0 right-censored at -y[n].  Per draw, with k_s = exp(loginvscale[s]), sigma_s = 1 / k_s, l[n,s] =
 * sum_d X[n,d] W[s,d] + o[n] (offset may be NULL), t = |y| and z = k_s (log t - l), the three outputs are
 *      mu = e^l e^{sigma_s^2 / 2}        v = e^{2l} (e^{sigma_s^2} - 1) e^{sigma_s^2}
 *      log p(y | l, k_s) = tau_s - log t - z^2 / 2 - log(2 pi) / 2   (y > 0: the density)
 *                        = log Phi(-z)                                (y < 0: the log survival)
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s v + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], k_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * The lpd of a censored row is therefore the log of the posterior-predictive survival probability at that time, and a
 * batch with every row censored at t_n gives log S(t_n | x_n).  log Phi(-z) is the training pass's, in its forms.  Both
 * moment factors are made once per launch in float64 from tau_s itself and rounded.  exp is NOT clamped: mean stops being
 * finite at l + sigma^2 / 2 > 88, var at 2 l + 2 sigma^2 > 88; y = 0 is not checked here.  FLOAT32 ENVELOPE OF THE
 * MOMENTS: the variance factor ~ e^{2 sigma^2} overflows float32 at sigma^2 = 44.4 (tau = -1.90; sigma^2 = 54.6 at
 * tau = -2); accuracy envelope loginvscale in [-1.5, 4], where the factor is 2.8e17 at most.  Outputs, refusals, envelope
 * and determinism are bsc_nb_predict_pass's; loginvscale == NULL is BSC_ERR_INVALID. */
int bsc_lognormal_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                               int64_t B, int32_t D, const float* W, const float* loginvscale, int32_t S, float* mean,
                               float* var, float* lpd, double* lpd_sum);

/* The predictive of the zero-inflated Poisson model (csrc/bsc_glm_zip.hip: bsc_predict_pass's kernel with a family that
 * only this entry point reaches).  Per draw, with pi_s = sigmoid(logodds[s]), L1_s = softplus(logodds[s]) (both made once
 * per launch in float64 and rounded), l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset may be NULL) and mu = e^l, the three
 * outputs are
 *      m = (1 - pi_s) mu        v = (1 - pi_s) mu (1 + pi_s mu)
 *      log p(y | l, tau_s) = max(tau_s, -mu) + log1p(e^{-|tau_s + mu|}) - L1_s     (y == 0: log(pi + (1 - pi) e^{-mu}))
 *                          = y l - mu - L1_s - lnGamma(y + 1)                      (y > 0)
 *      mean[n] = 1/S sum_s m,     var[n] = 1/S sum_s v + 1/S sum_s (m - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], tau_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * log p in the training pass's forms; lnGamma(y + 1) is taken off once per row after the log-mean-exp (lnGamma(1) = 0
 * keeps the zero rows right).  A batch with y = 0 in every row gives the log of the predictive P(y = 0 | x).  exp is NOT
 * clamped: mean stops being finite at l > 88, var at 2 l > 88; lpd is finite for |l| <= 80.  y is not checked here.
 * Outputs, refusals, envelope and determinism are bsc_nb_predict_pass's; logodds == NULL is BSC_ERR_INVALID. */
int bsc_zip_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                         int32_t D, const float* W, const float* logodds, int32_t S, float* mean, float* var,
                         float* lpd, double* lpd_sum);

/* The predictive of the Student-t model (csrc/bsc_glm_studentt.hip: bsc_predict_pass's kernel with a family that only
 * this entry point reaches).  Per draw, with k_s = exp(loginvscale[s]), nu = df (bsc_glm_studentt_data_pass's: finite and
 * > 0, rounded to float32), l[n,s] = sum_d X[n,d] W[s,d] + o[n] (offset may be NULL) and z = k_s (y - l), the three
 * outputs are
 *      mu = l        v = nu / ((nu - 2) k_s^2)  for nu > 2,   +infinity for nu <= 2
 *      log p(y | l, k_s) = tau_s + c_nu - ((nu + 1) / 2) log1p(z^2 / nu)
 *      mean[n] = 1/S sum_s mu,     var[n] = 1/S sum_s v + 1/S sum_s (mu - mean[n])^2
 *      lpd[n]  = logsumexp_s log p(y[n] | l[n,s], k_s) - log S,     lpd_sum = sum_n lpd[n]     (float64 [1])
 * mu is the LOCATION: the mean of the distribution for nu > 1 and its median for every nu (at nu <= 1 the distribution
 * has no mean and `mean` is the draw average of the median).  var is +infinity in every row at nu <= 2, exactly.  tau_s +
 * c_nu and v are made once per launch in float64 and rounded; log p is the training pass's, in its forms.  Nothing is
 * clamped; y is not checked here.  Outputs, refusals, envelope and determinism are bsc_nb_predict_pass's;
 * loginvscale == NULL and a df that is not finite and > 0 are BSC_ERR_INVALID. */
int bsc_studentt_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                              int64_t B, int32_t D, const float* W, const float* loginvscale, int32_t S, double df,
                              float* mean, float* var, float* lpd, double* lpd_sum);

/* The predictive of the random-intercept model (csrc/bsc_predict_group.hip: bsc_predict_pass_offset's kernel with a
 * per-draw, per-group intercept; bsc_glm_data_pass_groups is its training pass):
 *      l[n,s] = sum_d X[n,d] W[s,d] + Bt[row(groups[n]), s] + o[n]          (offset may be NULL: o = 0)
 * family BSC_PREDICT_LOGISTIC or BSC_PREDICT_POISSON, everything after l as bsc_predict_pass.  groups int32 [B],
 * contiguous, any 4-byte alignment.  Bt float32 [J + 1][ldb], the draws CONTIGUOUS: Bt[j, s] = b_s[j] for the J groups
 * of training, and row J the draws of a group that was NOT seen in training, b_new,s ~ N(0, e^{-zeta_s}), which the id
 * -1 selects: row(-1) = J, row(j) = j.  (bsc_glm_data_pass_groups' Bz [chunk][J][8] is the same numbers in the
 * training pass's order.)  Columns S .. ldb - 1 are not used.
 * IDS ARE TRUSTED HERE -- bsc_group_ids_check is the range check, once per batch.  They cannot touch memory all the
 * same: the gather goes through a descriptor of exactly (J + 1) ldb 4 bytes, and an id outside [-1, J) reads an
 * intercept of 0 for every draw.
 * Argument errors (BSC_ERR_INVALID) as bsc_predict_pass.  Outside the envelope (BSC_ERR_UNSUPPORTED, nothing is
 * launched, outputs untouched): bsc_predict_pass's, and a family other than the two above, groups or Bt NULL, J outside
 * [1, BSC_GLM_GROUP_MAX_J], ldb < S, ldb % 4 != 0, ldb > 8192, Bt not 16-byte aligned, groups or offset not 4-byte
 * aligned.  Asynchronous and allocation-free once the workspace holds lpd_sum's block partials (bsc_ctx_reserve).
 * Deterministic like bsc_predict_pass: no float atomics.  With Bt = 0 every output is bit-identical to
 * bsc_predict_pass_offset on the same inputs. */
int bsc_predict_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                            const float* offset, const int32_t* groups, int64_t B, int32_t D, int32_t J, const float* W,
                            const float* Bt, int32_t ldb, int32_t S, float* mean, float* var, float* lpd,
                            double* lpd_sum);

/* The range check of a predictive batch's ids: every groups[n] in [0, J), or in [-1, J) with allow_new != 0.  One small
 * kernel finds the first offending row; the call then SYNCHRONISES (like bsc_glm_group_plan, which checks the ids of a
 * training batch) -- call it once per batch, never inside an update.  BSC_ERR_INVALID with
 * "row <n> has group id <id> outside [-1,<J>)" (or "[0,<J>)").  Uses 8 bytes of the workspace (pending pass partials of
 * bsc_blr_data_pass_partial are dropped). */
int bsc_group_ids_check(bsc_ctx* ctx, const int32_t* groups, int64_t B, int32_t J, int32_t allow_new);

/* ---- random intercepts for the families with a learned scalar (csrc/bsc_glm_scalar_group.hip,
 *      csrc/bsc_predict_scalar_group.hip; ABSENT in the reference) ------------------------------------------------------
 *
 * family F = BSC_SCALAR_NEGBIN (bsc_glm_nb_data_pass's density), BSC_SCALAR_GAMMA (bsc_glm_gamma_data_pass's) or
 * BSC_SCALAR_WEIBULL (bsc_glm_weibull_data_pass's, right censoring in the sign of y), with its scalar e^tau:
 *      l[n,s] = sum_d X[n,d] W[s,d] + Bz[g[n], s] + o[n]             y[n] ~ F(l[n,s], e^{tau_s})
 *      w ~ N(0, I / prior_precision),  b_j | zeta ~ N(0, e^{-zeta}),  e^zeta ~ Gamma(group_a0, group_b0),
 *      e^tau ~ Gamma(a0, b0)
 * The latent is z = [w (D) | b (J) | zeta | tau], P = D + J + 2, the guide mean-field: lam = [m (P) | rho (P)].  The
 * intercept enters through l alone: ell, the residual r = d ell / d l and T are the family's own forms at that l.
 * From the data one update needs stats = [ell (S) | G (S*D) | H (S*J) | T (S)], H[s,j] = sum_{n : g[n] = j} r[n,s],
 * T[s] = d ell[s] / d tau_s.
 *
 * The pass.  The plan is bsc_glm_group_plan's, Bz [ceil(S / 8)][J][8] and H bsc_glm_data_pass_groups', logtau [S] and T
 * the family's pass's; every order of summation depends on the plan alone, no float atomics.  With Bz = 0, ell, G and T
 * are bit-identical to the family's own pass on the same inputs.  The envelope and the refusals are
 * bsc_glm_data_pass_groups' and the family's pass's, and a family outside the three codes is refused.  The 16-row MFMA
 * kernel (D == 256) is taken when y, g and the set ones of offset and weight are 16-byte aligned, else the 8-row
 * kernel.  The workspace (bsc_glm_scalar_group_workspace_bytes: the slab with T's eight floats per workgroup, residuals,
 * segment sums) grows on demand -- synchronously; bsc_ctx_reserve it first. */
#define BSC_SCALAR_NEGBIN 0
#define BSC_SCALAR_GAMMA 1
#define BSC_SCALAR_WEIBULL 2
int64_t bsc_glm_scalar_group_workspace_bytes(bsc_ctx* ctx, int64_t B, int32_t J);
int bsc_glm_scalar_data_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                                    const float* offset, const float* weight, const int32_t* g, const int32_t* plan,
                                    int64_t B, int32_t D, int32_t J, const float* W, const float* Bz,
                                    const float* logtau, int32_t S, double* ell, double* G, double* H, double* T);

/* The finish of all three families (it sees the statistics, never the likelihood), two launches.  eps in
 * bsc_blr_noise's [S, (P-1)+1] layout: columns 0 .. P-2 (w, b, zeta) from stream 0, column P-1 (tau) from stream 1.
 * W, Bz and logtau are the float32 draws the pass read; zeta_s = m_zeta + e^{rho_zeta} eps_s,P-2 in float64:
 *     log p(z) = c0 - prec/2 |w|^2 + J/2 zeta - e^zeta/2 |b|^2 + group_a0 zeta - group_b0 e^zeta + a0 tau - b0 e^tau
 *     g_w    = scale G_s - prior_precision w_s            g_b   = scale H_s - e^{zeta_s} b_s
 *     g_zeta = J/2 + group_a0 - e^{zeta_s} (group_b0 + 1/2 sum_j b_sj^2)       g_tau = scale T_s + a0 - b0 e^{tau_s}
 * ELBO, d/d m, d/d rho and Adam as bsc_glm_hier_update.  When the *_next buffers are set (all or none), W_next,
 * Bz_next (chunked, unused slots zeroed) and logtau_next [S] are made from eps_next; eps_next_ready = 0 draws the noise
 * of next_step into eps_next first (bsc_blr_noise(P - 1)).  Requires 1 <= S <= 64, 1 <= J <= BSC_GLM_GROUP_MAX_J,
 * t >= 1 and prior_precision, a0, b0, group_a0, group_b0, scale > 0.  Fixed-order sums, no atomics. */
int bsc_glm_scalar_hier_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                               double* m2, const double* eps, const float* W, const float* Bz, const float* logtau,
                               int32_t D, int32_t J, int32_t S, double scale, double prior_precision, double a0,
                               double b0, double group_a0, double group_b0, int64_t t, double lr, double beta1,
                               double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                               int32_t eps_next_ready, float* W_next, float* Bz_next, float* logtau_next, double* elbo,
                               double* grad);

/* The predictive: bsc_predict_pass_groups' table Bt [J + 1][ldb] (row J for id -1) and envelope, the family's
 * bsc_nb_predict_pass / bsc_gamma_predict_pass / bsc_weibull_predict_pass link and per-draw scalar logtau [S] (not
 * NULL, 4-byte aligned).  With Bt = 0 every output is bit-identical to the family's own predictive pass. */
int bsc_scalar_predict_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                                   const float* offset, const int32_t* groups, int64_t B, int32_t D, int32_t J,
                                   const float* W, const float* Bt, int32_t ldb, const float* logtau, int32_t S,
                                   float* mean, float* var, float* lpd, double* lpd_sum);

/* ---- multi-class softmax regression (csrc/bsc_softmax.hip; ABSENT in the reference) ------------------------
 *
 * Labels y[n] in {0 .. K-1} (int32), weights W[S,K,D] (S draws of a K x D matrix, flattened parameter p = k D + d)
 * under w ~ N(0, I / prior_precision) on all K D entries.  One streaming pass over X[B,D] (row-major, leading
 * dimension ldx floats) and y[B] per group of floor(16 / K) draws:
 *      l[n,s,k]  = sum_d X[n,d] W[s,k,d],      lse[n,s] = logsumexp_k l[n,s,k]      (maximum subtracted)
 *      ell[s]    = sum_n ( l[n,s,y[n]] - lse[n,s] )                           (float64 out, [S])
 *      G[s,k,d]  = sum_n ( 1[y[n] = k] - softmax_k(l[n,s,:]) ) X[n,d]          (float64 out, [S,K,D])
 * A row whose label is outside [0, K) is skipped entirely (nothing in ell, nothing in G); the label is only compared
 * with class indices, never used as an address, so any int32 value is memory-safe.  [ell | G] is the stats vector of
 * bsc_glm_update / bsc_glm_fullrank_update called with D := K D.
 * Envelope (BSC_ERR_INVALID with a message naming the quantity, outputs untouched): 2 <= K <= 16, D % 4 == 0,
 * 4 <= D <= 256, 1 <= S <= 64, X and W 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26, non-NULL ell and G.
 * y is contiguous with any 4-byte alignment.  B = 0 gives zeros.  Deterministic: fixed partition, float32 block
 * partials in the workspace (pending pass partials of bsc_blr_data_pass_partial are dropped), fixed-order float64
 * reduction, no float atomics. */
int bsc_softmax_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, int64_t B, int32_t D, int32_t K,
                          const float* W, int32_t S, double* ell, double* G);

/* Posterior predictive of the softmax model for S draws W[S,K,D] of a fitted q; X is read once for every S.  Per row
 * (each output may be NULL)
 *      prob[n,k] = 1/S sum_s softmax_k(l[n,s,:])                                          (float32 [B,K])
 *      lpd[n]    = logsumexp_s ( l[n,s,y[n]] - lse[n,s] ) - log S                         (float32 [B]; needs y)
 *      lpd_sum   = sum_n lpd[n]                                                           (float64 [1]; needs y)
 * A row whose label is outside [0, K) gets lpd[n] = 0 and adds nothing to lpd_sum; prob is written for every row.
 * Argument errors (BSC_ERR_INVALID, outputs untouched): the envelope of bsc_softmax_data_pass, no output requested,
 * lpd or lpd_sum without y.  B = 0 writes lpd_sum = 0 and nothing else.  Deterministic: float64 block partials of
 * lpd in the workspace (pending pass partials are dropped), fixed-order finish, no float atomics. */
int bsc_softmax_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, int64_t B, int32_t D,
                             int32_t K, const float* W, int32_t S, float* prob, float* lpd, double* lpd_sum);

/* ---- ordinal (cumulative-logit, proportional-odds) regression with learned cutpoints (csrc/bsc_glm_ordinal.hip;
 *      ABSENT in the reference) ---------------------------------------------------------------------------------
 *
 * Labels y[n] in {0 .. K-1} (int32), 2 <= K <= 8, in their ORDER.  eta[n,s] = sum_d X[n,d] w[s,d] + o[n], cutpoints
 * c_0 < .. < c_{K-2} per draw:
 *      P(y <= k) = sigmoid(c_k - eta),     P(y = k) = sigmoid(c_k - eta) - sigmoid(c_{k-1} - eta)   (c_{-1} = -inf,
 *      c_{K-1} = +inf)
 * in the unconstrained coordinates theta_0 = c_0, theta_j = log(c_j - c_{j-1}) (j >= 1), so every draw is ordered.  The
 * latent is z = [w (D) | theta (K - 1)], P = D + K - 1, under z ~ N(0, I / prior_precision); there is no intercept: the
 * cutpoints are the intercepts.
 * Z: the draws, float32 [S, ldz] with ldz >= P, weights in columns 0 .. D-1 and theta in columns D .. P-1, 4-BYTE
 * aligned (bsc_glm_update's W_next [S, P] as it stands; the kernels read the draws once per launch with 4-byte loads).
 * With a = c_{y-1} - eta, b = c_y - eta, U = [y < K-1], L = [y > 0], g = c_y - c_{y-1}, sp the stable softplus:
 *      log p            = -U sp(-b) - L sp(a) + U L log(-expm1(-g))
 *      r = d log p / d eta  = L sigmoid(a) - U sigmoid(-b)
 *      d log p / d c_y      = U (sigmoid(-b) + L / expm1(g)),      d log p / d c_{y-1} = -L (sigmoid(a) + U / expm1(g))
 *      ell[s]       = sum_n v[n] log p                              (float64 out, [S])
 *      G[s,d]       = sum_n v[n] r[n,s] X[n,d]      (d < D)         (float64 out, [S, P])
 *      G[s,D]       = sum_j H_j[s],   G[s,D+i] = e^{theta_i} sum_{j >= i} H_j[s]  (i >= 1),   H_j = d ell[s] / d c_j
 * [ell | G] is the stats vector of bsc_glm_update / bsc_glm_fullrank_update called with D := P.  The cutpoints are the
 * float32 roundings of the float64 cumulative sum of the float32 theta read, g the float32 difference of those;
 * log(-expm1(-g)) and 1 / expm1(g) are made once per launch in float64 and rounded.  ACCURACY ENVELOPE: theta_j in
 * [-3, 1.5] for j >= 1 (gaps 0.05 .. 4.5), |eta - c| <= 30.
 * offset and weight are bsc_glm_data_pass_obs's (each may be NULL: o = 0, v = 1).  A row is dropped -- adds EXACTLY
 * nothing -- when v[n] = 0 or y[n] is outside [0, K), by a select on the link's inputs; the label that indexes the
 * (draw, class) table is inside it for every int32 value.
 * Envelope (BSC_ERR_INVALID with a message naming the quantity, outputs untouched): 2 <= K <= 8, D % 4 == 0,
 * 4 <= D <= 256, 1 <= S <= 64 (eight draws per launch), X 16-byte aligned, ldx >= D, ldx % 4 == 0, ldx < 2^26,
 * ldz >= D + K - 1, ldz < 2^26, y, offset, weight and Z 4-byte aligned, non-NULL ell and G.  The 16-row MFMA kernel
 * (D == 256) is taken when y and the set ones of offset and weight are 16-byte aligned, else the 8-row kernel.  B = 0 gives
 * zeros.  Deterministic: fixed partition, float32 block partials of 8 * 256 + 8 + 7 * 8 floats (ell and the H_j behind
 * G), fixed-order float64 finish, no float atomics. */
int bsc_glm_ordinal_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, const float* offset,
                              const float* weight, int64_t B, int32_t D, int32_t K, const float* Z, int64_t ldz,
                              int32_t S, double* ell, double* G);

/* The predictive of the ordinal model (csrc/bsc_glm_ordinal.hip: bsc_predict_pass's kernel with a seventh family that
 * only this entry point reaches) for S <= 64 draws Z [S, ldz] as above; offset may be NULL.  Per row (each output may be
 * NULL)
 *      prob[n,k] = 1/S sum_s P(y = k | eta[n,s], c_s)                                     (float32 [B, K])
 *      lpd[n]    = logsumexp_s log p(y[n] | eta[n,s], c_s) - log S                        (float32 [B]; needs y)
 *      lpd_sum   = sum_n lpd[n]                                                           (float64 [1]; needs y)
 * prob comes from the differences of the cumulative sigmoids, which telescope (the K entries of a row add up to 1 to
 * rounding); log p from the form above, which does not cancel.  A row whose label is outside [0, K) gets lpd[n] = 0 and
 * adds nothing to lpd_sum; prob is written for every row.  Refusals: K, Z's alignment, ldz, null pointers, no output
 * requested and lpd or lpd_sum without y are BSC_ERR_INVALID; D, S, ldx and X's alignment are bsc_predict_pass's
 * (BSC_ERR_UNSUPPORTED).  B = 0 writes lpd_sum = 0 and nothing else.  Deterministic as bsc_predict_pass. */
int bsc_ordinal_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const int32_t* y, const float* offset,
                             int64_t B, int32_t D, int32_t K, const float* Z, int64_t ldz, int32_t S, float* prob,
                             float* lpd, double* lpd_sum);

/* ---- parameter updates --------------------------------------------------- */

/* Adam ascent on a flat float64 vector; t is the 1-based step count. */
int bsc_adam_ascent(bsc_ctx* ctx, double* lam, const double* grad, double* m1,
                    double* m2, int64_t n, int64_t t, double lr, double beta1,
                    double beta2, double eps);

/* SVI natural-gradient / VMP step (README.md:36,75-77; Hoffman et al. [4]):
 *   eta <- (1-rho) eta + rho (eta0 + scale * message),  all float64[n]. */
int bsc_natgrad_update(bsc_ctx* ctx, double* eta, const double* eta0,
                       const double* message, int64_t n, double scale, double rho);

/* Dirichlet expectation out[r,c] = exp(digamma(lam[r,c]) - digamma(sum_c lam[r,c]))
 * (float32 in/out, float64 inside) and the float32 form of the natural-gradient
 * step with a scalar prior, eta <- (1-rho) eta + rho (eta0 + scale * message):
 * the K x V global parameter of the LDA-style Dirichlet-Multinomial model
 * (BASELINE config 4; its sufficient statistics are the two contractions
 * Bt * dot(Th.T, C / dot(Th, Bt)) evaluated through bsc_gemm_strided_batched). */
int bsc_dirichlet_expectation(bsc_ctx* ctx, const float* lam, int64_t rows, int64_t cols,
                              int64_t ld, float* out);
int bsc_natgrad_update_f32(bsc_ctx* ctx, float* eta, float eta0, const float* message, int64_t n,
                           float scale, float rho);

/* Expectation of a Categorical node: out[r, :] = softmax(in[r, :]) over the LAST axis and, when lse
 * is not NULL, lse[r] = log sum_c exp in[r, c] (the responsibilities of a mixture's discrete latent
 * and the bound's normaliser; README.md:43 -- in the derived mean-field engine the data-sized
 * assignments stay on the device).  float32, rows ld_in / ld_out elements apart, cols <= 1024. */
int bsc_softmax_rows(bsc_ctx* ctx, const float* in, int64_t rows, int64_t cols, int64_t ld_in, float* out,
                     int64_t ld_out, float* lse);

/* The same expectation when the logits are a tall-skinny product that nothing else needs:
 *   L = alpha * A . B,  R = softmax_rows(L),  lse[r] = log sum_c exp L[r, c],  cross[r] = sum_c R[r, c] L[r, c]
 * with A [rows, K] (unit column stride, rows lda apart), B [K, N] (strides ldbk, ldbn), R [rows, N]
 * (rows ldr apart) -- features(x_n) . coefficients of a mixture with exponential-family components
 * (README.md:43; alpha = the 1 / (N / B) of a local latent under mini-batch scaling, README.md:69-79).  One pass: A is read once and R written once; the logits never reach memory (as two
 * launches they are written, read and written again).  `cross` (may be NULL) is what the factor's
 * entropy sum_r (lse[r] - cross[r]) needs in place of the logits.  float32; K <= 64 and a multiple of
 * 8, N <= 64 and a multiple of 4, A and R 16-byte aligned, lda % 4 == ldr % 4 == 0, lda < 2^25 (a tile's 32 rows
 * are addressed through 32-bit byte offsets; BSC_ERR_INVALID beyond); a K or N outside these is
 * BSC_ERR_UNSUPPORTED (callers then take bsc_gemm_strided_batched + bsc_softmax_rows, as they do for such a view). */
int bsc_gemm_softmax_rows(bsc_ctx* ctx, const float* A, int64_t lda, int64_t rows, int32_t K,
                          const float* B, int64_t ldbk, int64_t ldbn, int32_t N, float alpha, float* R,
                          int64_t ldr, float* lse, float* cross);

/* ... and the statistics every neighbour of that latent asks for, in the same pass:
 *   stats[c, f] = sum_r R[r, c] A[r, f]          (float32 [N, K], rows ldst apart),   lse_sum[0] = sum_r lse[r]
 * -- R^T . A with A = [T_1(x) | T_2(x) | .. | 1] the feature matrix the logits were formed from: the
 * responsibility-weighted sufficient statistics of a mixture with exponential-family components (statistics
 * of iid draws add up, bayesic/distribution/base.py:329-332; marginalisation by summation README.md:43,72) and,
 * through the ones column, the responsibilities' column sums.  The tile's responsibilities go from the softmax
 * registers through wave-private LDS into the backward MFMAs; R (may be NULL) is written only when something
 * else reads it.  csrc/bsc_mog.hip's E-step for any feature matrix of up to 64 columns; float64 fixed-order
 * finish.  `bias` (may be NULL; N values ldbn apart): L = alpha * (A . B + bias) -- the feature matrix's ones
 * column taken out of the product; its statistic, the column sums sum_r R[r, c], is then written to
 * stats[c, K] (ldst >= K + 1, K <= 56).  Same limits as bsc_gemm_softmax_rows otherwise. */
int bsc_gemm_softmax_stats(bsc_ctx* ctx, const float* A, int64_t lda, int64_t rows, int32_t K,
                           const float* B, int64_t ldbk, int64_t ldbn, int32_t N, float alpha, const float* bias,
                           float* R, int64_t ldr, float* stats, int64_t ldst, double* lse_sum);

/* Fixed-gamma local step of the LDA-style Dirichlet-Multinomial model (BASELINE
 * config 4): sstats[k,v] = Bt[k,v] * sum_d Th[d,k] C[d,v] / (sum_k' Th[d,k'] Bt[k',v]),
 * the algebra expression Bt * dot(Th.T, C / dot(Th, Bt)) (lowered by
 * bayesic/algebra.py:553-765 to two _tensordot GEMMs around a division) in ONE pass
 * over the count matrix C[docs, V]: neither docs x V intermediate is written.
 * Th[docs, K] = exp(E[log theta]), Bt[K, V] = exp(E[log beta]) (bsc_dirichlet_expectation);
 * all float32, row-major with leading dimensions in elements; fp32 MFMA.
 * K must be 32, 64, 96 or 128 (else BSC_ERR_UNSUPPORTED -- the executor path is general). */
int bsc_lda_sstats(bsc_ctx* ctx, const float* C, int64_t ldc, int64_t docs, int64_t V, int32_t K,
                   const float* Th, int64_t ldth, const float* Bt, int64_t ldb, float* sstats,
                   int64_t ldo);

/* The same statistic from SPARSE counts in compressed-sparse-column form (column v =
 * word v: colptr[V+1] offsets into rowidx (document ids) / vals (counts)): one pass over
 * the nonzeros, no atomics, fixed summation order.  Real bag-of-words data is ~1 % dense
 * (SURVEY.md 8(f) rank 4); explicit zeros contribute nothing.  Same K limits. */
int bsc_lda_sstats_csc(bsc_ctx* ctx, const int64_t* colptr, const int32_t* rowidx, const float* vals,
                       int64_t docs, int64_t V, int32_t K, const float* Th, int64_t ldth,
                       const float* Bt, int64_t ldb, float* sstats, int64_t ldo);

/* The evidence lower bound of the same model (ABSENT in the reference; README.md:30-37, mini-batch
 * form README.md:69-79; Hoffman, Blei, Bach 2010 eq. 7 with the per-word assignments at their
 * optimum; oracle.svi.lda_elbo):
 *   ELBO = scale * [ sum_dv C_dv log(phinorm_dv) - sum_d KL(Dir(gamma_d) || Dir(alpha)) ]
 *          - sum_k KL(Dir(lambda_k) || Dir(eta)),          phinorm = Th Bt.
 * bsc_lda_sstats_bound / bsc_lda_sstats_csc_bound are the statistic kernels above that ALSO return
 * ll[0] = sum_dv C_dv log(phinorm_dv) (float64, device): phinorm exists only in their registers, so
 * the sum is taken there -- a v_log_f32 and an fma per element, float32 per-wave partials, added in
 * float64 in a fixed order; no extra pass over C.
 * bsc_dirichlet_expectation_bound is bsc_dirichlet_expectation that also returns
 * bound[0] = sum_r -KL(Dir(lam_r) || Dir(prior)) (symmetric scalar prior; float64, fixed order), from
 * the digamma values it computes anyway plus one lnGamma per element (both factors' terms: rows =
 * topics for lambda, rows = documents for gamma).
 * bsc_natgrad_update_f32_elbo is bsc_natgrad_update_f32 that first writes
 * elbo[0] = scale * (ll[0] + local_bound[0]) + global_bound[0]: the bound at the lambda the step
 * starts from (ll and local_bound all-reduced when data-parallel). */
int bsc_lda_sstats_bound(bsc_ctx* ctx, const float* C, int64_t ldc, int64_t docs, int64_t V, int32_t K,
                         const float* Th, int64_t ldth, const float* Bt, int64_t ldb, float* sstats,
                         int64_t ldo, double* ll);
int bsc_lda_sstats_csc_bound(bsc_ctx* ctx, const int64_t* colptr, const int32_t* rowidx, const float* vals,
                             int64_t docs, int64_t V, int32_t K, const float* Th, int64_t ldth,
                             const float* Bt, int64_t ldb, float* sstats, int64_t ldo, double* ll);
int bsc_dirichlet_expectation_bound(bsc_ctx* ctx, const float* lam, int64_t rows, int64_t cols, int64_t ld,
                                    double prior, float* out, double* bound);
int bsc_natgrad_update_f32_elbo(bsc_ctx* ctx, float* eta, float eta0, const float* message, int64_t n,
                                float scale, float rho, const double* ll, const double* local_bound,
                                const double* global_bound, double* elbo);
/* The same step on a [rows, cols] block: eta with leading dimension ld_eta, the message with ld_msg -- the
 * piece of lambda [K, V] that one column range of the statistic, staged contiguously for its collective,
 * belongs to.  elbo != NULL: elbo[0] = scale * (ll[0] + .. + ll[n_ll - 1] + local_bound[0]) + global_bound[0]
 * first (one words' term per piece).  The same arithmetic per element as bsc_natgrad_update_f32.
 * bsc_lda_sstats_round_columns: the columns of ONE whole round of the persistent statistic kernel on this
 * context (128 per resident workgroup); a statistic taken in ranges that start at multiples of it is
 * bit-identical to the statistic taken in one call (every column block then has the schedule it has there). */
int bsc_natgrad_update_f32_2d(bsc_ctx* ctx, float* eta, int64_t ld_eta, float eta0, const float* message,
                              int64_t ld_msg, int64_t rows, int64_t cols, float scale, float rho, const double* ll,
                              int32_t n_ll, const double* local_bound, const double* global_bound, double* elbo);
int bsc_lda_sstats_round_columns(bsc_ctx* ctx, int32_t K, int64_t* host_cols);

/* ---- summed sufficient statistics of iid draws ---------------------------
 * ExpFamIndependentObservations.sufficient_statistics,
 * bayesic/distribution/base.py:328-332; Normal t(x)=(x,x^2),
 * bayesic/distribution/core.py:16-17.
 * stats[0]=n, stats[1]=sum x, stats[2]=sum x^2 (float64). */
int bsc_suffstats_normal(bsc_ctx* ctx, const float* x, int64_t n, double* stats);

/* ---- mixture of Gaussians: discrete latent marginalised by summation ------
 * (ABSENT in reference; README.md:43,72; statistics per
 * bayesic/distribution/base.py:329-332).  For every row of X[N,D]:
 *     logit_k = c[k] + sum_d (Wmat[k,d] x_d + Wmat[k,D+d] x_d^2)
 *     r_k     = softmax_k(logit)
 * and, summed over rows in float64 (fixed order):
 *     stats[k] = [sum r_k | sum r_k x (D) | sum r_k x^2 (D)]   ([K, 1+2D])
 *     lse[0]   = sum_n logsumexp_k(logit_nk)
 * Both contractions run on fp32 MFMA.  Limits: D <= 16, K <= 64 (one tile); X 4-byte aligned, D <= ldx < 2^25
 * (a tile's 32 rows are addressed through 32-bit byte offsets). */
int bsc_mog_estep(bsc_ctx* ctx, const float* X, int64_t ldx, int64_t N, int32_t D, int32_t K,
                  const float* Wmat, const float* c, double* stats, double* lse);

/* Responsibility-weighted second moments (full-covariance mixture statistic
 * sum_n r_nk x_n x_n^T; t(x) = (x, x x^T) of bayesic/distribution/core.py:41-44 summed over
 * the iid axis, bayesic/distribution/base.py:329-332):
 *     out[k,d,e] = scale * sum_n R[n,k] X[n,d] Y[n,e]          (float32 [K, D, E], contiguous)
 * in ONE pass over R[N,K], X[N,D], Y[N,E] (row-major, leading dimensions in floats).  The
 * reference lowers this einsum to a _tensordot over a materialised K x D x N product
 * (bayesic/algebra.py:632-636).  Y == X (same pointer, ld and extent) computes only d <= e and
 * mirrors.  fp32 MFMA, float64 fixed-order finish.  Limits: K <= 64, D, E <= 32, all
 * multiples of 4, 16-byte aligned operands, ld % 4 == 0 (else BSC_ERR_UNSUPPORTED -- the
 * executor then takes the general route). */
int bsc_weighted_outer(bsc_ctx* ctx, const float* R, int64_t ldr, const float* X, int64_t ldx,
                       const float* Y, int64_t ldy, int64_t N, int32_t K, int32_t D, int32_t E,
                       double scale, float* out);

/* Mean-field global parameters of the mixture: Dirichlet over weights and a
 * Normal-Gamma per (component, column), as one natural-parameter vector
 *   eta = [alpha-1 (K) | kappa*m (K*D) | kappa (K*D) | 2a-1 (K*D) | 2b+kappa*m^2 (K*D)].
 * bsc_mog_expected_params writes the float32 logit coefficients Wmat [K, 2D] and
 * c [K] (expectations under q; digamma in float64).  bsc_mog_natgrad applies
 *   eta <- (1-rho) eta + rho (eta0 + scale * message(stats))
 * (README.md:36,75-77) straight from the [K, 1+2D] statistics. */
int bsc_mog_expected_params(bsc_ctx* ctx, const double* eta, int32_t K, int32_t D, float* Wmat,
                            float* c);
int bsc_mog_natgrad(bsc_ctx* ctx, double* eta, const double* eta0, const double* stats, int32_t K,
                    int32_t D, double scale, double rho);

/* The evidence lower bound of the mixture (ABSENT in the reference; README.md:30-37 "maximise a
 * lower bound on the model evidence", mini-batch form README.md:69-79; every factor decomposed as
 * bayesic/distribution/base.py:47-69).  With the assignments marginalised by summation
 * (README.md:43,72) the bound at q(theta) = eta is
 *     ELBO = scale * sum_n logsumexp_k(logit_nk) + bound,
 *     bound = E_q[log p(pi,mu,tau)] - E_q[log q(pi,mu,tau)] = sum_factors <eta0-eta, E_q[T]> - A(eta0) + A(eta)
 * (oracle.svi.mog_elbo / mog_global_bound).  bsc_mog_log_normalizer writes A(eta) (one float64, device):
 * called once with the prior's eta0, it gives the constant `prior_A` of the model.
 * bsc_mog_expected_params_bound is bsc_mog_expected_params that also writes `bound` (one float64,
 * device) from the same digamma / log values; bsc_mog_natgrad_elbo is bsc_mog_natgrad that first writes
 * elbo[0] = scale * lse[0] + bound[0] (lse: what bsc_mog_estep returned for THIS eta, all-reduced
 * when data-parallel) -- the bound at the parameters the step starts from.  No extra launch, no
 * extra pass.  K <= 1024. */
int bsc_mog_log_normalizer(bsc_ctx* ctx, const double* eta, int32_t K, int32_t D, double* A_out);
int bsc_mog_expected_params_bound(bsc_ctx* ctx, const double* eta, const double* eta0, const double* prior_A,
                                  int32_t K, int32_t D, float* Wmat, float* c, double* bound);
int bsc_mog_natgrad_elbo(bsc_ctx* ctx, double* eta, const double* eta0, const double* stats, int32_t K,
                         int32_t D, double scale, double rho, const double* lse, const double* bound,
                         double* elbo);

/* The exact posterior predictive of the fitted mixture under the mean-field q (ABSENT in the reference;
 * README.md:43,72 -- marginalise the discrete latent by summation -- for a NEW row, with the Dirichlet and the
 * Normal-Gamma factors integrated out in closed form).  With (alpha [K], m, kappa, a, b [K, D]) read from eta as
 * above, the predictive is a mixture of products of Student-t laws,
 *     p(x*) = sum_k alpha_k / sum(alpha) prod_d St(x_d; location m_kd, scale^2 = b_kd (kappa_kd + 1) / (a_kd kappa_kd),
 *                                                   dof 2 a_kd),
 *     logit_k(x) = c_k - sum_d h_kd log1p(q_kd (x_d - m_kd)^2),
 *         h_kd = a_kd + 1/2,   q_kd = kappa_kd / (2 b_kd (kappa_kd + 1)),
 *         c_k  = log alpha_k - log sum(alpha) + sum_d [lnGamma(a_kd + 1/2) - lnGamma(a_kd) + log(q_kd / pi) / 2],
 *     lpd(x)   = logsumexp_k logit_k(x)        (the log posterior-predictive density),
 *     R_k(x)   = exp(logit_k(x) - lpd(x))      (the predictive probability that the row belongs to component k),
 *     label(x) = argmax_k logit_k(x)           (the lowest index among equal float32 maxima).
 * The logit is formed from (x - m)^2, not from the expanded quadratic (which loses digits on data that are not
 * centred), and log1p as log(w) u / (w - 1), w = 1 + u: h ~ N_k / 2 multiplies whatever log(1 + u) would lose.
 *
 * bsc_mog_predictive_params writes the table Pt float32 [K, 3D] = [m | q | h] and c float32 [K]: everything in
 * float64, rounded once.  K <= 1024; the validity of eta is the caller's, as for bsc_mog_expected_params.
 *
 * bsc_mog_predict_pass is ONE pass over X (float32 [N, D], rows ldx apart).  Each of lpd [N], label [N],
 * R [N, K] (rows ldr >= K apart) and lpd_sum [1] may be NULL, not all four.  lpd_sum = sum_n lpd(x_n) in float64 in a
 * fixed order (no float atomics: two runs give the same bits); N = 0 is BSC_OK and gives lpd_sum = 0.  Nothing is
 * written past N rows, and the pass reads no environment variable.  Limits, the fused E-step's: D <= 16 and K <= 64
 * (BSC_ERR_UNSUPPORTED otherwise); X 4-byte aligned, D <= ldx < 2^25. */
int bsc_mog_predictive_params(bsc_ctx* ctx, const double* eta, int32_t K, int32_t D, float* Pt, float* c);
int bsc_mog_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, int64_t N, int32_t D, int32_t K,
                         const float* Pt, const float* c, float* lpd, int32_t* label, float* R, int64_t ldr,
                         double* lpd_sum);

/* ---- black-box VI, score-function gradient with control variate ------------
 * (ABSENT in reference; README.md:52 -> ref [3]; config 5: hierarchical logistic
 * regression y_n ~ Bernoulli(sigmoid(x_n.w + b_{g_n})), z = [w (D) | b (G) | log tau],
 * q(z) = N(mu, diag e^{2 rho}), lam = [mu (P) | rho (P)], P = D+G+1.)
 *
 * bsc_bbvi_sample: z_s = mu + e^rho eps_s (Philox stream 2) -> eps [S,P] f64,
 *   Wz [S,D] f32, Bz [G,S] f32 (transposed), zeta [S] f64.
 * bsc_logreg_bbvi_loglik: ONE pass over X[N,D], y[N] (0/1 as float), g[N] (int32):
 *   ell[s] = sum_n ( y_n l_ns - softplus(l_ns) ),  l_ns = x_n.Wz[s] + Bz[g_n,s]
 *   (float64 out, fixed order).  fp32 MFMA.  Requires S == 64, D % 4 == 0, D <= 256.
 * bsc_bbvi_grad: f_s = scale*ell_s + log p(z_s) - log q(z_s); control variate
 *   a = sum_i Cov(f h_i, h_i) / sum_i Var(h_i); grad = mean_s (f_s - a) h_s with
 *   h_s = [eps/sigma | eps^2 - 1]; elbo = mean_s f_s.  f_out (may be NULL): f [S]. */
int bsc_bbvi_sample(bsc_ctx* ctx, const double* lam, int32_t D, int32_t G, int32_t S, uint64_t seed,
                    uint32_t step, double* eps, float* Wz, float* Bz, double* zeta);
int bsc_logreg_bbvi_loglik(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y,
                           const int32_t* g, int64_t N, int32_t D, int32_t n_groups,
                           const float* Wz, const float* Bz, int32_t S, double* ell);
int bsc_bbvi_grad(bsc_ctx* ctx, const double* lam, const double* eps, const double* ell, int32_t D,
                  int32_t G, int32_t S, double scale, double a0, double b0, double* elbo,
                  double* grad, double* f_out);
/* bsc_bbvi_update: everything after the pass in three launches -- bsc_bbvi_grad's f and
 * control-variate moments, then ONE kernel for the gradient, the Adam ascent step of
 * bsc_adam_ascent (step count t >= 1, in place on lam, m1, m2) and the draws of the NEXT update
 * (bsc_bbvi_sample with `next_step`, from the new lam: eps is overwritten, Wz / Bz / zeta
 * refreshed).  Same results as the three separate calls up to float64 summation order. */
int bsc_bbvi_update(bsc_ctx* ctx, double* lam, double* eps, const double* ell, int32_t D, int32_t G,
                    int32_t S, double scale, double a0, double b0, double* m1, double* m2, int64_t t,
                    double lr, double beta1, double beta2, double eps_adam, uint64_t seed,
                    uint32_t next_step, float* Wz, float* Bz, double* zeta, double* elbo,
                    double* grad, double* f_out);

/* ---- executable primitives of the algebra front end -----------------------
 * The five-op IR that Einsum lowering emits plus element-wise nodes:
 * _sum bayesic/algebra.py:1284-1294, _mul :1297-1309, _dimshuffle :1312-1326 and
 * _diagonal :1398-1414 (both are stride views -- no kernel), _tensordot
 * :1329-1383, elemwise/add :195-233, log/exp/pow/abs_ :1435-1448, eye :236-258.
 * Tensors are (pointer, shape, strides-in-elements); a stride of 0 broadcasts a
 * size-1 axis (the 'x' axes of dimshuffle).  rank <= BSC_MAX_RANK. */

typedef enum bsc_dtype { BSC_F32 = 0, BSC_F64 = 1 } bsc_dtype;

typedef enum bsc_op {
    BSC_OP_ADD = 0, /* n-ary, 1..8 inputs */
    BSC_OP_MUL = 1, /* n-ary, 1..8 inputs */
    BSC_OP_LOG = 2,
    BSC_OP_EXP = 3,
    BSC_OP_POW = 4, /* in0 ** in1 */
    BSC_OP_ABS = 5,
    BSC_OP_COPY = 6, /* materialise a strided view */
    BSC_OP_LGAMMA = 7,  /* log Gamma(x): unary, bsc_map_reduce only (log-normalisers of the */
    BSC_OP_DIGAMMA = 8, /* Gamma / Dirichlet / Wishart nodes and their expectations)        */
    BSC_OP_SCALE = 9    /* x * arg: unary, bsc_map_reduce only -- a per-operand coefficient, so that
                         * (1 - rho) eta + rho m (the damped natural-gradient step, README.md:75-77) is one launch */
} bsc_op;

/* out[i] = op(in_0[i], ..., in_{n-1}[i]) over the index space `shape`;
 * in_strides is [n_in][rank] row-major; `in` is a HOST array of n_in device
 * pointers. */
int bsc_elemwise(bsc_ctx* ctx, int op, int dtype, int rank, const int64_t* host_shape, void* out,
                 const int64_t* host_out_strides, int n_in, const void* const* host_in,
                 const int64_t* host_in_strides);

/* dst = (dst_dtype) src, both strided (dtype conversion + layout change). */
int bsc_convert(bsc_ctx* ctx, int src_dtype, int dst_dtype, int rank, const int64_t* host_shape,
                const void* src, const int64_t* host_src_strides, void* dst,
                const int64_t* host_dst_strides);

/* out[keep...] = sum over red... of in[keep..., red...]; float64 accumulation,
 * fixed summation order (deterministic).  out is contiguous over keep_shape. */
int bsc_sum(bsc_ctx* ctx, int dtype, int rank_keep, const int64_t* host_keep_shape,
            const int64_t* host_in_keep_strides, int rank_red, const int64_t* host_red_shape,
            const int64_t* host_in_red_strides, const void* in, void* out);

/* Fused pointwise map with an optional trailing sum: one pass over the operands
 * for a chain elemwise -> add/_mul -> elemwise -> _sum (bayesic/algebra.py:195-233,
 * 1284-1309, 1435-1448), which the reference leaves to Theano's graph optimiser.
 *   v(keep, red) = post( scale * COMBINE_i pre_i( in_i[keep, red] ) + shift )
 *   out[keep]    = sum over red of v(keep, red)     (rank_red == 0: out[keep] = v(keep))
 * combine is BSC_OP_ADD or BSC_OP_MUL; pre_op[i] and post_op are BSC_OP_COPY, SCALE, LOG,
 * EXP, ABS, LGAMMA, DIGAMMA or POW (x ** arg, arg taken from pre_arg[i] / post_arg).  in_keep_strides
 * is [n_in][rank_keep], in_red_strides [n_in][rank_red] (0 broadcasts); sums
 * accumulate in float64 in a fixed order. */
int bsc_map_reduce(bsc_ctx* ctx, int dtype, int combine, int rank_keep,
                   const int64_t* host_keep_shape, int rank_red, const int64_t* host_red_shape,
                   int n_in, const void* const* host_in, const int64_t* host_in_keep_strides,
                   const int64_t* host_in_red_strides, const int32_t* host_pre_op,
                   const double* host_pre_arg, double scale, double shift, int post_op,
                   double post_arg, void* out, const int64_t* host_out_strides);

/* C[b,m,n] = sum_k A[b,m,k] * B[b,k,n], every stride free (so transposed and
 * broadcast operands cost nothing).  float32 runs on v_mfma_f32_32x32x2_f32 with
 * a deterministic split-K when M*N is small against K (XtX: M=N=256, K=1e6);
 * float64 is a plain VALU kernel. */
int bsc_gemm_strided_batched(bsc_ctx* ctx, int dtype, int64_t batch, int64_t M, int64_t N,
                             int64_t K, const void* A, int64_t sa_b, int64_t sa_m, int64_t sa_k,
                             const void* B, int64_t sb_b, int64_t sb_k, int64_t sb_n, void* C,
                             int64_t sc_b, int64_t sc_m, int64_t sc_n);

/* The same product with its consumer folded into the store (what Theano's graph optimiser would do
 * for `B * dot(X, Y)` and `C / dot(X, Y)`, bayesic/algebra.py:741-765 + 1297-1309):
 *     C[b,m,n] = scale * (sum_k A[b,m,k] B[b,k,n]) ^ power * E[b,m,n],   power = 1 | -1,
 * E strided like C (a stride of 0 broadcasts; E == NULL: no factor).  float32, K > 0. */
int bsc_gemm_epilogue(bsc_ctx* ctx, int dtype, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A,
                      int64_t sa_b, int64_t sa_m, int64_t sa_k, const void* B, int64_t sb_b, int64_t sb_k,
                      int64_t sb_n, void* C, int64_t sc_b, int64_t sc_m, int64_t sc_n, int power, double scale,
                      const void* E, int64_t se_b, int64_t se_m, int64_t se_n);
/* bsc_gemm_epilogue with an element-wise PRODUCER folded into the operand fragments as well:
 *   C = scale * dot(pre_a(A), pre_b(B))^power * E,   pre = 0 none | 1 square | 2 exp | 3 abs   (power 0: no epilogue)
 * -- `_mul` / `elemwise` feeding `_tensordot` (bayesic/algebra.py:741-765, 1297-1309 -> :1347) without the
 * intermediate array: dot(exp(X), Y), dot(X * X, A.T).  Only the persistent stream kernel applies prologues; when the
 * shape takes another path (matrix-vector, skinny, float64, short contractions), or both sides ask for exp (padded
 * zeros would no longer cancel), NOTHING is launched and *handled = 0: the caller materialises the operand and calls
 * bsc_gemm_strided_batched / bsc_gemm_epilogue.  *handled = 1: C is written. */
int bsc_gemm_fused(bsc_ctx* ctx, int dtype, int64_t batch, int64_t M, int64_t N, int64_t K, const void* A, int64_t sa_b,
                   int64_t sa_m, int64_t sa_k, int pre_a, const void* B, int64_t sb_b, int64_t sb_k, int64_t sb_n, int pre_b,
                   void* C, int64_t sc_b, int64_t sc_m, int64_t sc_n, int power, double scale, const void* E, int64_t se_b,
                   int64_t se_m, int64_t se_n, int32_t* handled);

/* Host-only: the schedule the persistent kernels (GEMM, LDA statistic) use for `tiles` tiles of `n_kt`
 * units on `slots` resident workgroups; out = {n_wg, rounds, tail_tiles, sk_stream, sk_q, sk_r} --
 * workgroup w takes tiles w, w + n_wg, ... of `rounds` rounds, then units [u(w), u(w + 1)) of the
 * tail tiles' unit list, u(w) = sk_stream ? w sk_q + min(w, sk_r) : min(w, tail_tiles) n_kt. */
int bsc_stream_plan(int64_t tiles, int32_t n_kt, int64_t slots, int32_t out[6]);

/* out[b] = log det A[b] for symmetric positive-definite A[b] (n x n, strides in
 * elements), by float64 Cholesky -- the T.logdet of MultivariateNormal's
 * log-normaliser, bayesic/distribution/core.py:49-52.  NaN when not SPD. */
int bsc_logdet_spd(bsc_ctx* ctx, int dtype, int64_t batch, int64_t n, const void* A, int64_t s_b,
                   int64_t s_r, int64_t s_c, void* out);

/* out[b] (n x n, contiguous) = the inverse of the symmetric positive-definite A[b] (strides in elements; the mean of
 * the two triangles is taken), by float64 Cholesky; logdet[b] = log det A[b] when logdet is not null.  What turns the
 * natural parameters of a multivariate-normal or Wishart factor (precision, V^-1) into its expectations on the
 * device: the variational-message-passing update of README.md:36 for the (t(x) = (x, x x^T)) family of
 * bayesic/distribution/core.py:41-56, whose host-side form calls numpy.linalg.inv.  NaN when not SPD. */
int bsc_inverse_spd(bsc_ctx* ctx, int dtype, int64_t batch, int64_t n, const void* A, int64_t s_b, int64_t s_r,
                    int64_t s_c, void* out, void* logdet);

/* out[n,n] = identity, contiguous. */
int bsc_eye(bsc_ctx* ctx, int dtype, void* out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* BAYESIC_HIP_H */
