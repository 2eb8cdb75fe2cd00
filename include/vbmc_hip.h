/*
 * vbmc_hip.h -- C ABI of libvbmc_hip.so: the MI355X (gfx950) implementation of
 * PyVBMC's ELBO-evaluation hot path.
 *
 * The reference (acerbilab/pyvbmc) is pure Python and has no FFI; the boundary
 * it offers for this path is a set of Python callables.  Each entry point below
 * names the reference callable whose arithmetic it replaces (paths relative to
 * /root/reference/pyvbmc).  The Python mirror of those callables lives in
 * pyvbmc_amd/ and reaches this library through ctypes only.
 *
 * Conventions
 *   - every pointer argument is CALLER-OWNED HOST memory, contiguous, float64 /
 *     int32 / int64 as typed; the library copies in and out.  No torch types.
 *   - matrices are row-major.  `mu_KxD` is K rows of D means, i.e. exactly
 *     theta[:D*K] / mu.ravel(order="F") of the reference's (D,K) array
 *     (variational_posterior/variational_posterior.py:653-676).
 *   - return value: 0 = ok, <0 = error (VBMC_E_*); text via vbmc_last_error().  One entry point
 *     has a positive "do it again" code (VBMC_W_GP_CHANGED), one a positive "not here" code (VBMC_W_NOT_FUSED).
 *     No C++ exception crosses the boundary.
 *   - a vbmc_ctx owns one device, its HIP streams, device scratch and (optionally)
 *     one RCCL communicator.  A ctx is not thread-safe; distinct ctxs are
 *     independent.
 *   - grad_flags bit0..3 = gradients wrt (mu, sigma, lambda, w), the reference's
 *     4-tuple `grad_flags` (entropy/entmc_vbmc.py:9, entlb_vbmc.py:8).
 *   - all arithmetic is float64.
 */
#ifndef VBMC_HIP_H
#define VBMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vbmc_ctx vbmc_ctx;

enum {
  VBMC_OK = 0,
  VBMC_E_ARG = -1,     /* bad argument / state (e.g. mixture not set)      */
  VBMC_E_HIP = -2,     /* HIP runtime error                                 */
  VBMC_E_RCCL = -3,    /* RCCL error                                        */
  VBMC_E_NODEV = -4,   /* no usable gfx950 device                           */
  VBMC_E_UNSUP = -5,   /* combination the reference raises NotImplemented on */
  VBMC_E_NONFINITE = -6, /* non-finite input where the path needs finite    */
  VBMC_E_NOMEM = -7,    /* host allocation failed (vbmc_mt19937_randn)       */
  VBMC_E_NOTPD = -8,    /* vbmc_gp_posterior / vbmc_gp_append: a pivot of the Cholesky factorisation is not a
                           positive finite number; the GP state installed before the call is unchanged */
  VBMC_W_GP_CHANGED = 1, /* vbmc_neg_elcbo only: the watched GP arrays changed (vbmc_set_gp_watch);
                           the outputs were computed on the GP of the last vbmc_set_gp: discard them,
                           upload the GP again and repeat the call                               */
  VBMC_W_NOT_FUSED = 2   /* vbmc_adam_run_auto: this run does not have the one-launch form (shape, ranks,
                           or a launch that gave up waiting); nothing was done: use vbmc_adam_run in batches.
                           vbmc_mt19937_randn_dev: the request is not the device generator's; the state is
                           untouched: draw with vbmc_mt19937_randn                                        */
};

/* GP mean functions understood by the path
 * (vbmc/variational_optimization.py:1383-1392). */
enum { VBMC_MEAN_ZERO = 0, VBMC_MEAN_CONST = 1, VBMC_MEAN_NEGQUAD = 2 };

/* Source of the standard-normal draws of the Monte-Carlo entropy. */
enum {
  VBMC_EPS_RESIDENT = 0, /* draws uploaded with vbmc_set_eps (parity mode: the
                            reference's np.random.randn stream, entmc_vbmc.py:67) */
  VBMC_EPS_PHILOX = 1    /* Philox4x32-10 + Box-Muller generated on the device, fresh
                            per call from `seed` (throughput mode): by extra blocks
                            of the prep launch, by spare workgroups of the optimiser
                            loop's short launches one iteration ahead, or inside the
                            entropy kernel -- the same values                        */
};

/* ---- library / context ------------------------------------------------- */

/* ABI version of this header (bumped on any signature change). */
int vbmc_abi_version(void);

/* Number of visible HIP devices (0 on a box without a GPU; never fails hard). */
int vbmc_device_count(int* n_out);

/* Create a context on HIP device `device_id`.  Fails with VBMC_E_NODEV when no
 * GPU is present -- there is no CPU fallback behind this ABI.
 * device_id == -1 creates a HOST-ONLY context: it can hold the mixture
 * (vbmc_set_mixture / vbmc_theta_to_mixture) and run the host finalisation
 * (vbmc_entmc_finalize); every entry point that would launch a kernel returns
 * VBMC_E_NODEV on it.  It exists so the sharded reduce->finalise path can be
 * exercised by multi-process CPU tests. */
int vbmc_ctx_create(int device_id, vbmc_ctx** out);
void vbmc_ctx_destroy(vbmc_ctx* ctx);

/* Host placement.  The polled evaluation is a latency chain over PCIe, and on a two-socket host it is 2.5 us (3 %) per
 * evaluation shorter from the device's own NUMA node (csrc/ctx.hip bind_host_thread).  vbmc_ctx_create therefore narrows
 * the CALLING THREAD's CPU affinity to the CPUs local to the device (sysfs local_cpulist of its PCI function) before it
 * allocates its pinned buffers.  It only removes CPUs from the thread's current set and leaves a set alone that is
 * already inside the node or entirely outside it; VBMC_HOST_AFFINITY=0 in the environment disables it.  This reports what
 * happened: *bound_out = 1 when this context narrowed the set, *n_cpus_out = CPUs in the thread's set afterwards
 * (0: the device's CPU list could not be read).  No counterpart in the reference (a NumPy program). */
int vbmc_host_affinity(const vbmc_ctx* ctx, int* bound_out, int* n_cpus_out);

/* Last error text of `ctx` (or of the failed vbmc_ctx_create when ctx==NULL). */
const char* vbmc_last_error(const vbmc_ctx* ctx);

/* Device facts for the bench harness: name (NUL-terminated, truncated to
 * name_len), compute units, max clock kHz, global memory bytes. */
int vbmc_device_info(const vbmc_ctx* ctx, char* name, int name_len, int* cu_count,
                     int* clock_khz, uint64_t* hbm_bytes);

/* Block until everything queued on the ctx has finished (bench bracketing). */
int vbmc_synchronize(vbmc_ctx* ctx);

/* Switch the HIP event pair around the dominant kernels on or off (default: off).
 * A record between two dependent kernels puts a barrier packet into the queue, which
 * costs ~6 us per record on MI355X -- measurement harnesses switch it on for the
 * launches they want timed, production callers leave it off.
 * on = 2 additionally records the pair around gp_predict's variance product (which = 5 below): those two records sit
 * BETWEEN predict's launches and lengthen the interval which = 3 reports by their own ~12 us, so a harness reads
 * which = 3 at on = 1 and which = 5 at on = 2. */
int vbmc_set_timing(vbmc_ctx* ctx, int on);

/* Duration in milliseconds of the most recent TIMED launch (vbmc_set_timing) of the
 * dominant kernel of the given entry point, from HIP events on the ctx's own stream.
 * which: 0 = entmc main kernel, 1 = gp_log_joint, 2 = mixture pdf,
 *        3 = gp_predict (all its launches), 4 = whole last vbmc_neg_elcbo device section,
 *        5 = gp_predict's variance product kernel alone -- recorded at vbmc_set_timing(ctx, 2) ONLY, and that pass runs
 *            the product WITHOUT the finish in its epilogue (three launches where production runs two): it measures
 *            the product kernel, not the production configuration; a predict at level 0 / 1 invalidates the record
 *            (VBMC_E_ARG "no timed launch recorded", never a stale interval).
 *        6 = vbmc_gp_posterior's blocked Cholesky factorisation alone (all its block steps),
 *        7 = vbmc_is_mcmc's launch (all S chains),
 *        8 = vbmc_gp_lml's last chunk: its factorisation and its value / gradient kernels,
 *        9 = vbmc_search_fill's uploads and launches, 10 = vbmc_search_eval's acquisition, noise lookup and mask,
 *        11 = its sort and gather,
 *        12 = vbmc_gp_hyp_sample: all the rounds of the last call (a call that launched nothing leaves no record),
 *        13 = vbmc_search_cmaes: all the rounds of the last call, likewise,
 *        14 = vbmc_gp_hyp_optimize: all the rounds of the last call, likewise,
 *        15 = vbmc_sieve_fill's launch, 16 = vbmc_sieve_eval's scoring launches, 17 = its rank and gather. */
int vbmc_last_kernel_ms(vbmc_ctx* ctx, int which, double* ms_out);

/* Host-side wall-clock breakdown (microseconds) of the most recent vbmc_neg_elcbo:
 * out[0] theta -> mixture + pack upload issue, out[1] kernel launches,
 * out[2] wait for the device, out[3] host finalisation, out[4] total.
 * Profiling aid for bench.py / DESIGN.md; no reference counterpart. */
int vbmc_last_host_us(const vbmc_ctx* ctx, double out[5]);
/* Where the two result blocks of the most recent vbmc_neg_elcbo arrived on the host's clock, microseconds from
 * the call's entry: out[0] the GP sums' completion word (the host finalises G / dG behind it, while the entropy
 * kernel still runs), out[1] the entropy's completion word (or the end of the stream wait); out[2] where the
 * GP sums ran: 0 the prep launch, 1 the finish launch, 2 spare workgroup slots of the entropy launch; out[3]
 * reserved (0).  Profiling aid for bench.py (S > 1 hyper-parameter samples). */
int vbmc_last_step_marks(const vbmc_ctx* ctx, double out[4]);
/* A function the library calls from inside vbmc_neg_elcbo once the evaluation's launches are released (the pack and
 * the go word written, or the launches queued) and before it starts waiting for the device: the caller's own
 * bookkeeping that depends on theta alone -- the reference's vp.set_parameters side effects, which the Python mirror
 * applies from the mu / sigma / lambda / w / eta outputs, already filled at that point -- then runs while the device
 * works instead of between two evaluations.  fn = NULL clears it.  No reference counterpart. */
int vbmc_set_release_callback(vbmc_ctx* ctx, void (*fn)(void*), void* user);

/* Per-context switches for tests and measurements (no reference counterpart).  Each starts
 * from the environment variable in brackets, read when the context is created.
 *   "entmc_kernel" [VBMC_ENTMC_KERNEL=valu -> 1]: 0 = pick the kernel by shape (default),
 *                  1 = always the generic thread-per-row kernel (on-device cross-check)
 *   "entmc_mfma"   1 = shapes the FP64 matrix tile pads little and the wave-split kernel runs one wave per SIMD on
 *                  (D > 10 or K > 80, K within 12 below a multiple of 16: BASELINE config 5) take the matrix-pipe form
 *                  of the entropy kernel (default), 0 = the wave-split kernel everywhere
 *   "gp_ship"      [VBMC_GP_SHIP]: 1 = in the host-driven step whose GP sums run in the prep launch in front of the matrix-pipe entropy
 *                  kernel, their copy to pinned memory and their completion word are issued by a workgroup of the entropy
 *                  launch (default: the prep launch then ends with the sums), 0 = by the prep launch's last GP block
 *   "acq_poll"     [VBMC_ACQ_POLL]: 1 = vbmc_acq_eval with at most 256 points has the CPU write the points into host-writable
 *                  device memory and polls a completion word for the results (default), 0 = copies + stream wait
 *   "adam_fused"   [VBMC_ADAM_FUSED]: 1 = vbmc_adam_run runs a batch of iterations as ONE launch where the shape allows
 *                  (one rank, K <= 64, D <= 24, <= 64 antithetic rows per component, LDS plan fits -- with X^T resident in
 *                  the GP workgroups' LDS, or read from memory where that does not fit; default),
 *                  0 = always four launches per iteration; 2 = test hook (the launch also waits for a workgroup
 *                  that does not exist, must give up by its 20 ms limit, and the batch is redone as four launches)
 *                  3 = the one-launch form with its exchange written as agent-scope release stores / acquire fences
 *                  instead of write-through records and relaxed flags (the documented fallback: the same results bit
 *                  for bit, +5 us per iteration)
 *   "elbo_pregen"  [VBMC_ELBO_PREGEN]: 1 = Philox draws generated ahead of the entropy
 *                  kernel (default), 0 = generated in-line by it; same values either way
 *   "elbo_ahead"   [VBMC_ELBO_AHEAD]: 1 = after a Philox evaluation with seed s the draws of
 *                  seed s+1 are generated speculatively, by spare workgroups of the finish launch,
 *                  while the host finalises (default), 0 = never
 *   "mix_bar"      [VBMC_MIX_BAR]: 1 = in the polled host-driven step the CPU writes the mixture
 *                  pack straight into (fine-grained) device memory and the GP sums ride in spare
 *                  workgroup slots of the entropy launch when they fit (default), 0 = upload kernel,
 *                  GP sums in the prep launch
 *   "predict_dma"  [VBMC_PREDICT_DMA]: 1 = gp_predict's variance product for batches of > 32
 *                  points on Cholesky samples runs in the LDS-direct kernel (default), 0 = the
 *                  plain 64 x 64-tile kernel (cross-check)
 *   "predict_fused" [VBMC_PREDICT_FUSED_FINISH]: gp_predict's third stage (fmu / fs2 from the partial sums)
 *                  in the LDS-direct product kernel's epilogue, by an arrival ticket per 64-point row tile --
 *                  two launches instead of three, bit-identical results: 1 = where the product grid is one
 *                  round of workgroups (default), 2 = always, 0 = never (the finish launch)
 *   "elbo_arm"     [VBMC_ELBO_ARM]: 1 = after a polled Philox evaluation the launches of the next one
 *                  (seed + 1, same shapes) are queued at once and wait on the device for the next
 *                  call's theta (default); any other use of the context cancels them.  Never after an
 *                  evaluation that took more than 1 ms, and the device-side wait is at most 5 ms.
 *   "arm_late_test" / "ident_test": test hooks -- the n-th use of an armed evaluation from now takes
 *                  the late-go recovery path / the n-th identity check of a result block from now
 *                  fails (the evaluation is repeated unarmed); see vbmc_armed_stats
 *   "ws_span"      [VBMC_WS_SPAN]: 1 = the wave-split entropy kernel in span mode (default): every CU's
 *                  first-dispatched workgroup takes "ws_front" per mille of the CU's batches, the second one
 *                  the rest, parts crossing component boundaries, so that all workgroups end together
 *                  (csrc/entropy_args.h WsSpan); 0 = equal chunks per component
 *   "ws_front"     [VBMC_WS_FRONT]: that share (0 = built-in per instantiation); "ws_pad" [VBMC_WS_PAD]:
 *                  batches a component's end is priced at when the parts are cut (-1 = built-in)
 *   "ws_roles"     [VBMC_WS_ROLES]: 1 = which components a wave of the wave-split kernel takes is its role,
 *                  (wave + 2) mod 4 in the second workgroup of a CU and the wave index elsewhere, and a wave's
 *                  loops end behind the ceil((K - role) / 4) components it owns (default); 0 = role = wave and
 *                  every wave runs over all 4 KTMAX table rows.  Bit-identical results either way.
 * The results of an evaluation do not depend on any of these -- except that "ws_span" / "ws_front" /
 * "ws_pad" change how the Monte-Carlo rows are grouped into partial sums, i.e. the last bits of the
 * entropy (<= 1e-15 relative); for given values every evaluation is bit-reproducible.
 * Unknown key -> VBMC_E_ARG. */
int vbmc_set_option(vbmc_ctx* ctx, const char* key, int value);

/* Launch geometry of the most recent Monte-Carlo entropy of this ctx (vbmc_entmc,
 * vbmc_neg_elcbo, the optimiser loop): out[0] = kernel (0 generic, 1 wave-split on equal chunks, 2 small-
 * sample, 3 matrix-pipe form, 4 the fused optimiser loop: no entropy launch of its own, 5 wave-split in span
 * mode), out[1] = 64-row batches per workgroup (the wave-split kernel's batch loop count; span mode: the
 * longest part), out[2] = partial rows (workgroups) per component, out[3] = bit 0: the draws were read from
 * HBM (clear: generated in-line), bit 1: the wave-split kernel ran with "ws_roles".  Lets the parity tests assert which code path they exercised. */
int vbmc_last_entmc_plan(const vbmc_ctx* ctx, int out[4]);

/* Host utility (no device, no ctx): the span-mode partition of the wave-split entropy kernel for cus CUs of
 * which pb have a filler part, front share `front` (per mille), nb batches per component, `pad` slots priced
 * per component end, K components -- part_lo[cus + pb + 1] = first slot of every part of the padded list
 * (part_lo[last] = K (nb + pad)), first_part[K] = the part that holds each component's first batch,
 * *rows_per_component = partial rows per component.  The CPU suite checks the partition's invariants. */
int vbmc_ws_span_layout(int cus, int pb, int front, int nb, int pad, int K, int64_t* part_lo, int* first_part,
                        int* rows_per_component);

/* Host utility (no device, no ctx): a 64-bit checksum over n blocks of doubles,
 * sum_a (sum_i bits(v_ai) * odd_i + len_a) * odd_a mod 2^64 -- any change of a single element changes
 * it.  The Python mirror keys its "is this GP already on the device" test on it (every posterior's
 * alpha and hyp in full: an in-place edit anywhere in them is seen; ~1 us + 0.05 us per KB). */
int vbmc_host_checksum(const double* const* ptrs, const int64_t* lens, int n, uint64_t* out);

/* Watch the HOST arrays the device GP was uploaded from: n blocks of doubles (every posterior's alpha
 * and hyp) whose vbmc_host_checksum was `expected` at upload time.  vbmc_neg_elcbo then recomputes
 * that checksum itself -- after it has released its launches, while the device works and the host
 * would only be polling -- and returns VBMC_W_GP_CHANGED when it differs.  This keeps the caller's
 * "is this GP still the one on the device" test (the reference overwrites GP records in place,
 * active_importance_sampling.py:207-209) off the path between two evaluations of the optimiser.
 * The caller guarantees the blocks stay allocated while the watch is set; n = 0 or the next
 * vbmc_set_gp clears it. */
int vbmc_set_gp_watch(vbmc_ctx* ctx, const double* const* ptrs, const int64_t* lens, int n, uint64_t expected);

/* Counters of the polled host-driven step (vbmc_neg_elcbo) since the context was created:
 * out[0] armed evaluations used, out[1] cancelled, out[2] of those: late go word (recovery path),
 * out[3] result blocks whose identity was checked -- the finish launch publishes, next to the
 * sequence number, the checksum of the mixture pack the device actually read and the Philox seed
 * its launches were planned for, and the host compares both with what it sent -- out[4] checks
 * that failed (the evaluation was repeated), out[5] evaluations whose completion word never came
 * (the armed launches had given up, or a stuck device) and that were repeated. */
int vbmc_armed_stats(const vbmc_ctx* ctx, uint64_t out[6]);

/* The raw (pre-Jacobian) entropy accumulator [H | mu (K x D) | sigma (K) | lambda (D) | w (K)] of
 * the most recent Monte-Carlo vbmc_neg_elcbo of this ctx -- the vector the sharded job all-reduces
 * (additive over disjoint row slices; with a communicator: the sum over the ranks).  n must be
 * 1 + D*K + 2K + D.  VBMC_E_ARG when the last evaluation had none.  Lets the parity tests add up
 * the slices of virtual ranks (row_begin/row_count of vbmc_elbo_opts) on one GPU. */
int vbmc_last_elbo_raw(const vbmc_ctx* ctx, double* out, int n);

/* ---- mixture state: VariationalPosterior attributes --------------------- */

/* Upload the mixture (variational_posterior.py:106-138: mu (D,K), sigma (1,K),
 * lambd (D,1), w (1,K), eta (1,K)).  Values are taken as given (no
 * renormalisation: that is set_parameters' job, see vbmc_theta_to_mixture).
 * Giving the values the device already holds is a no-op (no pack, no upload): pdf,
 * acquisition and sampling calls between two updates of the posterior pay nothing. */
int vbmc_set_mixture(vbmc_ctx* ctx, int D, int K, const double* mu_KxD,
                     const double* sigma_K, const double* lambd_D, const double* w_K,
                     const double* eta_K);

/* The same with the means in the reference's own layout, mu (D,K) row-major -- the array a VariationalPosterior
 * holds -- so that a caller in front of every pdf / acquisition call passes its attribute arrays as they are. */
int vbmc_set_mixture_dk(vbmc_ctx* ctx, int D, int K, const double* mu_DxK,
                        const double* sigma_K, const double* lambd_D, const double* w_K,
                        const double* eta_K);

/* Host-side restatement of VariationalPosterior.set_parameters (raw_flag=True)
 * (variational_posterior.py:680-759) for the fused objective: theta ->
 * (mu, sigma, lambd, w) with exp, softmax (max-shifted), lambda renormalised to
 * unit RMS, plus eta = theta[-K:] - max (variational_optimization.py:1082-1085).
 * optimize_mask bit0..3 = optimize_{mu,sigma,lambd,weights}; blocks whose bit is
 * clear are absent from theta and the current ctx mixture values are kept.
 * Outputs (each nullable) receive the new attribute values. */
int vbmc_theta_to_mixture(vbmc_ctx* ctx, const double* theta, int n_theta,
                          int optimize_mask, double* mu_KxD, double* sigma_K,
                          double* lambd_D, double* w_K, double* eta_K);

/* ---- a3: VariationalPosterior.pdf / log_pdf in the transformed space ---- */

/* y[n] = sum_k w_k N(x_n; mu_k, sigma_k^2 diag(lambda^2))  (df = +/-inf or 0),
 * multivariate-t (df > 0) or product-of-univariate-t (df < 0) tails
 * (variational_posterior.py:441-529); log_flag: log with 0 -> -inf (:531-541);
 * grad_flag: dy (n x D), for log_flag dy/y (:464-469,532-533).  grad with finite
 * non-zero df -> VBMC_E_UNSUP (the reference raises NotImplementedError :499,527).
 * Bounds masking / Jacobian of orig_flag=True stay on the host (parameter
 * transformer), as in the reference they are separate pre/post steps. */
int vbmc_mixture_pdf(vbmc_ctx* ctx, int64_t n, const double* x_nxD, int log_flag,
                     int grad_flag, double df, double* y_n, double* dy_nxD);

/* ---- a6: entropy/entmc_vbmc.py:6-134 ------------------------------------ */

/* Make the antithetic half-draws resident in HBM: eps_half is [K][n_half][D]
 * (for component j the rows the reference draws with randn(Ns//2, D),
 * entmc_vbmc.py:64-68).  `row_begin,row_count` select the slice of each
 * component's rows this ctx will process (sharding); pass 0,n_half
 * for the whole job. */
int vbmc_set_eps(vbmc_ctx* ctx, int K, int64_t n_half, int D, const double* eps_half,
                 int64_t row_begin, int64_t row_count);

/* The reference's draw stream on the host cores (no device, no ctx): the next `n` values
 * np.random.randn would return from NumPy's legacy global state -- MT19937 words, 53-bit
 * uniforms, polar method (the eps of entmc_vbmc.py:67) -- bit for bit, with the state advanced
 * exactly as NumPy would leave it.  `key[624], pos, has_gauss, gauss` are the fields of
 * np.random.get_state(legacy=True) (in/out).  n_threads <= 0: all host cores (at most 64).
 * The MT19937 recurrence runs on one thread; the polar method's attempts, each a pure
 * function of its word position, on all of them (csrc/host_randn.hip). */
int vbmc_mt19937_randn(uint32_t* key, int* pos, int* has_gauss, double* gauss, double* out,
                       int64_t n, int n_threads);

/* The same stream generated on the DEVICE (csrc/device_randn.hip: MT19937 with a GF(2) jump-ahead per workgroup, the
 * polar method's attempts as position-pure work items, a prefix sum over the accepted pairs) and copied to `out`.
 * Words, accept / reject decisions and the state handed back are bit-identical to np.random.randn's; the VALUES use a
 * double-double logarithm on the device and about 0.1 % of them differ from NumPy's (glibc's log) by 1-3 units in the
 * last place (neither logarithm is correctly rounded everywhere; histogram in the source).  What vbmc_set_eps_numpy
 * uses (without the copy) when the context holds all rows.  The caller's state is written only on success.  Returns
 * VBMC_W_NOT_FUSED, state untouched, when the request is not this path's (more than 8e8 words, or fewer accepted
 * attempts than pairs inside the 6-sigma word margin: ~1e-9 per call) -- draw with vbmc_mt19937_randn then.
 * Reference: entropy/entmc_vbmc.py:64-68. */
int vbmc_mt19937_randn_dev(vbmc_ctx* ctx, uint32_t* key, int* pos, int* has_gauss, double* gauss, double* out,
                           int64_t n);
/* *window_reused = 1 when the context's last device pass (vbmc_mt19937_randn_dev / vbmc_set_eps_numpy) found the 33 blocks
 * behind its incoming state in the word sequence of the pass before -- a caller that keeps drawing from the stream where
 * the last call left it -- and did not have to compute them (csrc/device_randn.hip). */
int vbmc_randn_dev_info(const vbmc_ctx* ctx, int* window_reused);
/* Host twins of that jump for the CPU tests: the MT19937 block that starts n_words (>= 1) words after key_in[0], by the
 * polynomial t^(n_words-1) mod the characteristic polynomial (found by Berlekamp-Massey, csrc/mt_jump.h); and the
 * polynomials t^(m stride - 1), m = 1 .. count, as [count][624] words. */
int vbmc_mt_jump_host(const uint32_t* key_in, uint64_t n_words, uint32_t* key_out);
int vbmc_mt_jump_polys(uint64_t stride_words, int count, uint32_t* out);

/* vbmc_mt19937_randn + vbmc_set_eps in one call: the next K*n_half*D values of NumPy's legacy
 * stream (= np.random.randn(n_half, D) for j = 0..K-1, the reference's draw order) are generated
 * into a pinned buffer the ctx keeps and rows [row_begin, +row_count) of every component are
 * uploaded as the resident draws.  The generator state advances by the whole job's values on
 * every rank.
 * WHICH GENERATOR RUNS, and what that means for parity: a single-rank context that holds all rows and asks for
 * >= 65 536 values draws ON THE DEVICE (vbmc_mt19937_randn_dev: state, words and accept / reject decisions
 * bit-identical to NumPy, ~0.1 % of the values 1-3 ulp off); a row shard, a multi-rank context, a smaller request, or
 * the device pass answering VBMC_W_NOT_FUSED draws on the host cores (vbmc_mt19937_randn: every value bit-identical).
 * F and dF computed from the two therefore agree to ~1e-15 relative, not bit for bit.  Strict parity switch:
 * vbmc_set_option(ctx, "randn_device", 0) or VBMC_RANDN_DEVICE=0 in the environment -- always the host generator.
 * The caller's state is written only when the draw succeeded. */
int vbmc_set_eps_numpy(vbmc_ctx* ctx, uint32_t* key, int* pos, int* has_gauss, double* gauss, int K,
                       int64_t n_half, int D, int64_t row_begin, int64_t row_count, int n_threads);

/* Monte-Carlo entropy and its reparameterisation gradient.
 *   ns_per_comp : the reference's (even-rounded) Ns = 2*n_half.
 *   eps_mode    : VBMC_EPS_RESIDENT or VBMC_EPS_PHILOX (`seed` used by the latter).
 *   row_begin,row_count : the antithetic-pair rows of every component this ctx
 *                 evaluates (0,n_half = all); the normaliser stays ns_per_comp.
 *   H, dH       : as the reference returns them -- dH packs only the enabled
 *                 blocks [mu 'F' | sigma | lambda | w] (entmc_vbmc.py:48-51,132),
 *                 Jacobians applied when jacobian_flag (entmc_vbmc.py:114-130).
 *   raw_out     : nullable; receives the un-Jacobianed accumulator vector
 *                 [H | mu (K blocks of D) | sigma (K) | lambda (D) | w (K)]
 *                 (length 1+D*K+2K+D) -- the vector the all-reduce sums.
 * If the ctx has a communicator (vbmc_comm_init) the raw vector is summed over
 * ranks with ONE ncclAllReduce before finalisation. */
int vbmc_entmc(vbmc_ctx* ctx, int64_t ns_per_comp, int eps_mode, uint64_t seed,
               int64_t row_begin, int64_t row_count, int grad_flags, int jacobian_flag,
               double* H, double* dH, double* raw_out);

/* The draws of VBMC_EPS_PHILOX mode themselves: out[K][row_count][D] = the standard normals the
 * entropy kernels use for rows [row_begin, +row_count) of every component of a job with n_half
 * antithetic pairs per component (counter-based: Philox4x32-10 keyed by seed on (global row, block),
 * four normals per block; csrc/philox.h, restated by oracle/philox_ref.py).  Generated by the same
 * kernel code as inside an evaluation.  For parity and distribution tests; no reference counterpart
 * (the reference draws np.random.randn, entropy/entmc_vbmc.py:64-68). */
int vbmc_philox_normals(vbmc_ctx* ctx, int K, int64_t n_half, int D, uint64_t seed, int64_t row_begin,
                        int64_t row_count, double* out);

/* Finalise a raw accumulator vector on the host (Jacobians + packing,
 * entmc_vbmc.py:114-132) with the ctx's current mixture: what every rank does
 * after the all-reduce.  Exposed so the sharded path can be tested without a GPU
 * collective. */
int vbmc_entmc_finalize(vbmc_ctx* ctx, const double* raw, int grad_flags,
                        int jacobian_flag, double* H, double* dH);

/* ---- a7: entropy/entlb_vbmc.py:6-180 ------------------------------------- */
int vbmc_entlb(vbmc_ctx* ctx, int grad_flags, int jacobian_flag, double* H, double* dH);

/* ---- GP posterior state: what gpyreg hands the path (a11) --------------- */

/* X (N x D); per GP sample s: hyp (P doubles: [log ell (D), log sf, noise (1),
 * mean (0 | 1 | 1+2D)]), alpha (N), L (N x N), L_chol, sn2_eff = 1/sW[0]^2
 * (variational_optimization.py:1394-1398), sW (N) and sn2_mult for predict. */
int vbmc_set_gp(vbmc_ctx* ctx, int N, int D, int S, int P, int mean_kind,
                const double* X_NxD, const double* hyp_SxP, const double* alpha_SxN,
                const double* L_SxNxN, const int32_t* L_chol_S, const double* sW_SxN,
                const double* sn2_mult_S);

/* The same state BUILT on the device.  Replaces pyvbmc_amd/gp.py GP._posterior (gpyreg's posterior, SURVEY
 * Appendix A "Posterior"; gpyreg is not part of the reference tree) followed by vbmc_set_gp: per sample
 *   A = K(X, X) / sl + diag(sn2 / sn2_div),  U^T U = A (upper Cholesky),  alpha = U^-1 U^-T (y - m(X)) / sl,
 * with sl = sn2_div (sn2_mult = 1), sW = 1 / sqrt(sl), L = U, L_chol = 1.  The noise scalars are the caller's: sn2
 * (S x N, noise variance per point) and sn2_div (S, its minimum).  Afterwards the context's GP state is what
 * vbmc_set_gp would have left for those records, and y and sn2 stay on the device for vbmc_gp_append.  alpha_SxN and
 * L_SxNxN are nullable: only what is asked for is copied back.  VBMC_E_UNSUP when a sample has sn2_div < 1e-6 (the
 * non-Cholesky branch stays on the host), VBMC_E_ARG on bad shapes, VBMC_E_NOTPD when a sample does not factorise --
 * the state installed before is then unchanged.  FP64, fixed summation order: bit-reproducible. */
int vbmc_gp_posterior(vbmc_ctx* ctx, int N, int D, int S, int P, int mean_kind, const double* X_NxD,
                      const double* y_N, const double* sn2_SxN, const double* sn2_div_S, const double* hyp_SxP,
                      double* alpha_SxN, double* L_SxNxN);

/* One more training point (x, y) for the posterior vbmc_gp_posterior (or an earlier append) installed, in O(S N^2):
 * what gpyreg's gp.update(xnew, ynew, compute_posterior=True) does after every acquired point
 * (vbmc/active_sample.py:584), which gp.py answers with a full GP._posterior.  With k = K(X, x) / sl, l = U^-T k,
 * d = sqrt(sf^2 / sl + sn2 / sn2_div - l.l):  U' = [[U, l], [0, d]],  U'^-1 = [[U^-1, -U^-1 l / d], [0, 1 / d]].
 * Constant noise only: VBMC_E_UNSUP when the resident state has per-point noise, VBMC_E_ARG when it was not built
 * on the device, VBMC_E_NOTPD (state unchanged) when d^2 is not positive and finite.  Outputs nullable, of the
 * N + 1 points. */
int vbmc_gp_append(vbmc_ctx* ctx, const double* x_D, double y, double* alpha_SxN1, double* L_SxN1xN1);

/* The same append under per-point noise: sn2_new_S is, per sample, the new point's total noise variance (the noise
 * function at the new point, a user-provided s2 included).  The resident state may have constant or per-point noise,
 * but must be device-built (VBMC_E_ARG otherwise).  Applies while sn2_new_S[s] >= sl[s] for every s -- the new point
 * then leaves sn2_div, the scale of the factor, as it is; VBMC_E_UNSUP otherwise (the caller rebuilds with
 * vbmc_gp_posterior).  The new state's sn2 is the old rows plus the new entry; vbmc_gp_append applies to it afterwards
 * only if the old state had constant noise and every new entry equals sl.  Errors and outputs as vbmc_gp_append. */
int vbmc_gp_append_noisy(vbmc_ctx* ctx, const double* x_D, double y, const double* sn2_new_S, double* alpha_SxN1,
                         double* L_SxN1xN1);

/* Copy the resident posterior out: alpha (S x N) and L (S x N x N), both nullable. */
int vbmc_gp_fetch(vbmc_ctx* ctx, double* alpha_SxN, double* L_SxNxN);

/* Log marginal likelihood of the training data and its gradient for B hyper-parameter candidates: the objective of GP
 * hyper-parameter fitting (gpyreg's; not part of the reference tree -- the textbook formula).  Per candidate, with C =
 * K + diag(sn2) = sl A, U^T U = A, r = y - m(X), alpha = C^-1 r and sl = sn2_div as in vbmc_gp_posterior:
 *   lml = -1/2 r.alpha - sum_i log U_ii - N/2 log(2 pi sl),
 *   dlml/dtheta = -1/2 tr((C^-1 - alpha alpha^T) dC/dtheta) for [log ell (D), log sf, log sn], alpha . dm/dtheta for the
 * mean's parameters, in the layout of hyp.  dsn2_B: d sn2 / d log sn per candidate, the caller's (2 exp(2 hyp_noise)
 * under constant additive noise, 0 without it); priors are the caller's too.  Candidates are factorised in chunks whose
 * factor state stays under 1 GiB (vbmc_set_option "gp_lml_chunk" forces a chunk size); the GP the context holds is not
 * touched.  want_grad = 0: the value alone (dlml_BxP may then be null).  A candidate that is not positive definite or
 * whose results are not finite gets status_B = 1, lml = -inf and a NaN gradient row; the call still returns VBMC_OK and
 * the other candidates are what they would be without it.  VBMC_E_UNSUP when a candidate has sn2_div < 1e-6, D > 32 or
 * one candidate's state exceeds the cap; VBMC_E_ARG on bad shapes.  FP64, fixed summation order: bit-reproducible, and
 * a candidate's results do not depend on the chunking. */
int vbmc_gp_lml(vbmc_ctx* ctx, int N, int D, int B, int P, int mean_kind, const double* X_NxD, const double* y_N,
                const double* sn2_BxN, const double* sn2_div_B, const double* dsn2_B, const double* hyp_BxP, int want_grad,
                double* lml_B, double* dlml_BxP, int32_t* status_B);

/* GP hyper-parameter sampling: C slice-sampling chains over f(h) = lml(h) + log p(h), advanced in lockstep so that every
 * evaluation round is one batch of C candidates for vbmc_gp_lml's kernels (csrc/gp_hyp.hip; gpyreg's sampler, priors and
 * stream are not part of the reference tree -- these are this library's own, stated in NumPy by tests/slice_host.py and
 * pyvbmc_amd/gp.py).
 *   lml: what vbmc_gp_lml returns for the row h under sn2_n = exp(2 h[D+1]) + s2_n (s2_N nullable: no user-provided
 *   noise) and sn2_div = min_n sn2_n, from the same kernels; the exponential is taken on the device.  A candidate that
 *   does not factorise or whose value is not finite has f = -inf: it lies outside every slice and is never an error.
 *   log p(h) = sum_p t_p (p ascending); t_p = 0 where prior_sigma_P[p] is NaN, else with z = (h_p - mu_p) / sigma_p
 *   t_p = -1/2 log(2 pi) - log sigma - 1/2 z^2 where prior_df_P[p] is +inf, and the Student-t density's
 *   lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 log(pi nu) - log sigma - (nu+1)/2 log(1 + z^2/nu) otherwise.
 * Sampler: Neal's coordinate-wise slice sampler as tests/slice_host.py states it (level, then interval; stepping out at
 * most 32 evaluations a side, at most 64 shrink proposals; x0 clipped into [lb, ub]; burn_in + n thin sweeps, a sample
 * kept every thin-th sweep after burn_in).  Draw i of chain c is the 53-bit uniform of Philox block (i_lo, i_hi, c, 6)
 * under `seed`.  A round is one advance launch (workgroup = chain: the chain's state machine consumes the value of the
 * round before and writes its next candidate into the factorisation's inputs), then the factorisation and the value
 * kernels on the staged state; the GP the context holds is not touched.  Chains beyond one chunk (vbmc_gp_lml's plan,
 * vbmc_set_option "gp_lml_chunk") are processed chunk by chunk inside a round; the host reads back one count of
 * unfinished chains every vbmc_set_option "gp_hyp_rounds" rounds (default 4; a test hook).  X, y, s2 go up once.
 * Outputs: hyp_CxnxP the kept samples, logpost_Cxn their f, logprior_Cxn their log p, stats_Cx4 = [evaluations, draws,
 * step-out caps hit, shrink caps hit] per chain; invalid_C[c] = 1 when f(x0[c]) is not finite -- that chain's outputs
 * are zeros and the others are what they would be without it.  A chain's outputs depend on (data, x0[c], widths, bounds,
 * priors, n, thin, burn_in, seed, c) alone: not on C, the chunking or the rounds per read.
 * VBMC_E_UNSUP, before any launch: D > 32, one candidate's factor state exceeds the cap, or
 * exp(2 lb[D+1]) + min s2 < 1e-6 (the non-Cholesky branch stays on the host).  VBMC_E_ARG: bad shapes, bounds that are
 * not finite or lb > ub, widths <= 0, a prior with sigma <= 0 or df <= 0, n < 1, thin < 1, burn_in < 0. */
int vbmc_gp_hyp_sample(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                       const double* s2_N, int C, const double* x0_CxP, const double* widths_P, const double* lb_P,
                       const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P, const double* prior_df_P,
                       int n, int thin, int burn_in, uint64_t seed, double* hyp_CxnxP, double* logpost_Cxn,
                       double* logprior_Cxn, int64_t* stats_Cx4, int32_t* invalid_C);

/* GP hyper-parameter optimisation: R quasi-Newton runs over phi(h) = -(lml(h) + log p(h)) inside [lb, ub], advanced in
 * lockstep so that every evaluation round is one batch of R trial points for vbmc_gp_lml's factorisation, value and
 * gradient kernels (csrc/gp_opt.hip).  lml, log p and the data and prior arguments are vbmc_gp_hyp_sample's; the
 * derivative with respect to the noise parameter is that of constant additive noise.  The optimiser is this library's
 * own limited-memory BFGS with a projected gradient and a backtracking search, stated in NumPy by tests/gp_opt_host.py
 * and pyvbmc_amd/gp.py (it is not SciPy's L-BFGS-B), with g = grad phi:
 *   x0 clipped into the box; phi(x0) not finite: the run is invalid.  Bound set B = {p : (x_p <= lb_p and g_p > 0) or
 *   (x_p >= ub_p and g_p < 0) or lb_p = ub_p}, pg = g with the entries in B set to 0.  An iteration stops the run on
 *   max |pg| <= tol_g (stop reason 1), then on the iteration count reaching max_iter (2); else d = -H pg by the two-loop
 *   recursion over the stored pairs, oldest to newest, initial scaling s.y / y.y of the newest pair, entries in B set to
 *   0; g.d >= 0 or no pairs: the history is dropped and d = -pg.  Trial points x_t = clip(x + t d, lb, ub), t = 1 with
 *   pairs and min(1, 1 / sum |pg|) without, accepted when phi(x_t) is finite and phi(x_t) <= phi(x) + 1e-4 g.(x_t - x),
 *   else t <- t / 2, at most 30 times (then stop reason 4); a trial that does not factorise is a rejection.  After an
 *   accepted step the pair s = x_t - x, y = g_t - g is stored when s.y > 1e-10 |s| |y| (over the oldest when m are held),
 *   and the run stops on phi_old - phi_new <= tol_f max(1, |phi_new|) (3).  Every trial is one value+gradient evaluation.
 * A round is one advance launch (workgroup = run, one wave), then the factorisation and the value and gradient kernels on
 * the staged state; the GP the context holds is not touched.  Runs beyond one chunk (vbmc_set_option "gp_lml_chunk") are
 * processed chunk by chunk inside a round; the host reads back one count of unfinished runs every vbmc_set_option
 * "gp_opt_rounds" rounds (default 4); at most 2 + 31 max_iter rounds are queued, and runs unfinished then are
 * VBMC_E_HIP.  X, y, s2 go up once, the results come back in one copy.
 * Outputs: hyp_RxP the final points, logpost_R = lml + log p there, grad_RxP its gradient there, stats_Rx4 = [iterations,
 * evaluations, history resets, stop reason]; invalid_R[r] = 1 when phi(x0[r]) is not finite -- that run's outputs are
 * zeros and the others are what they would be without it.  trace_cap > 0 (at most max_iter + 1): trace_iter
 * [R][trace_cap][3 P + 3], row i = [x (P), phi, g (P), d (P), pairs held, 1 when d = -pg] of iteration i (the row of the
 * point a run ends at has d = 0), and trace_eval [R][1 + 31 trace_cap][4], row e = [iteration, t, phi_trial, accepted] of
 * evaluation e (row 0 the start's); rows not reached are zeros.  trace_cap = 0: both may be null.  A run's outputs
 * depend on (data, x0[r], bounds, priors, max_iter, m, tol_g, tol_f) alone: not on R, the chunking, the rounds per read
 * or the trace.
 * VBMC_E_UNSUP, before any launch: D > 32, one candidate's factor state exceeds the cap, or
 * exp(2 lb[D+1]) + min s2 < 1e-6.  VBMC_E_ARG: bad shapes, bounds that are not finite or lb > ub (lb = ub fixes the
 * parameter), a prior with sigma <= 0 or df <= 0, max_iter < 0, m outside [1, 16], a negative tolerance. */
int vbmc_gp_hyp_optimize(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                         const double* s2_N, int R, const double* x0_RxP, const double* lb_P, const double* ub_P,
                         const double* prior_mu_P, const double* prior_sigma_P, const double* prior_df_P, int max_iter, int m,
                         double tol_g, double tol_f, int trace_cap, double* hyp_RxP, double* logpost_R, double* grad_RxP,
                         int64_t* stats_Rx4, int32_t* invalid_R, double* trace_iter, double* trace_eval);

/* The GP hyper-parameter fit as ONE call: design, scoring and ranking of the candidates, vbmc_gp_hyp_optimize's runs from
 * the best of them, vbmc_gp_hyp_sample's chains from the optimum and vbmc_gp_posterior's build at the samples, on one
 * stream with the hand-overs done by kernels (csrc/gp_fit.hip).  X, y, s2 and the arrays below go up once in one block;
 * the host reads the two lockstep drivers' counts of unfinished runs and nothing else; the results come back in one copy.
 * pyvbmc_amd/gp.py states the stages in NumPy (GP.fit(optimizer="fused", device=False)).  lml, log p, the data and the
 * prior arguments are vbmc_gp_hyp_sample's.
 *   1 design    B = H + init_N candidates: the H rows of hyp0 clipped into [lb, ub], then init_N drawn rows, coordinate p
 *               of drawn row j = clip(dlb_p + (dub_p - dlb_p) u, dlb_p, dub_p) with u the 53-bit uniform of words 0, 1 of
 *               Philox block (p, 0, j, 10) under `seed`, no contraction.  [dlb, dub] inside [lb, ub] is the design box.
 *   2 score     every candidate factorised (value only, in vbmc_gp_lml's chunks); score = lml + sum_p t_p, exactly what
 *               vbmc_gp_hyp_optimize computes at a start; a candidate that is not finite or not positive definite, or a
 *               score that is not finite, gives -inf, never an error.  Ranked by score descending, ties to the lower
 *               index; the first R = min(opts_N, B) are the optimiser's starts (starts_R), one without a finite score an
 *               invalid run.
 *   3 optimise  (opts_N > 0) vbmc_gp_hyp_optimize's rounds from those starts (max_iter, m, tol_g, tol_f as there, no
 *               trace).  The optimum: the best candidate and its score, replaced by the first run of greatest finite log
 *               posterior where that is strictly greater.
 *   4 sample    (n_samples > 0) vbmc_gp_hyp_sample's rounds: n_samples chains from the optimum under the same `seed`
 *               (stream 6; the design's is stream 10), one kept sample each after burn_in + thin sweeps.
 *   5 install   S = n_samples samples (n_samples = 0: S = 1, the optimum) are built as vbmc_gp_posterior builds them, read
 *               from device memory, and left installed in the context exactly as that entry leaves its state; alpha_SxN,
 *               L_SxNxN are downloaded only where given.
 * Outputs (nullable except best_P, best_logpost, hyp_SxP, noise_S, status): cand_BxP, score_B; starts_R; the optimiser's
 * opt_hyp_RxP, opt_logpost_R, opt_stats_Rx4, opt_invalid_R; best_P and best_logpost, the optimum; hyp_SxP the installed
 * samples, with logpost_S, logprior_S, stats_Sx4 of the chains (n_samples = 0: logpost_S[0] = best_logpost);
 * noise_S[s] = exp(2 hyp[s][D+1]) as the device formed it (sn2 = noise + s2, sn2_div = noise + min s2: the inputs that
 * make vbmc_gp_posterior reproduce the installed state bit for bit); *status: bit 0 = no candidate has a finite score.
 * Contracts: every refusal happens before any launch, every VBMC_E_ARG before every VBMC_E_UNSUP, through the check the
 * two lockstep entries share: theirs, plus VBMC_E_ARG for dlb / dub outside [lb, ub] or dlb > dub (init_N > 0),
 * H + init_N < 1, negative counts.  "No candidate has a finite score" comes with VBMC_OK and the status bit; then, and on
 * any error, the installed GP is what it was.  The results depend on (data, hyp0, boxes, priors, options, seed) alone:
 * not on the chunking (vbmc_set_option "gp_lml_chunk") or on the rounds per read ("gp_opt_rounds", "gp_hyp_rounds").
 * vbmc_last_kernel_ms 12 and 14 report the chains' and the optimiser's rounds of the last call. */
int vbmc_gp_fit(vbmc_ctx* ctx, int N, int D, int P, int mean_kind, const double* X_NxD, const double* y_N,
                const double* s2_N, int H, const double* hyp0_HxP, int init_N, const double* dlb_P, const double* dub_P,
                const double* lb_P, const double* ub_P, const double* prior_mu_P, const double* prior_sigma_P,
                const double* prior_df_P, int opts_N, int max_iter, int m, double tol_g, double tol_f, int n_samples,
                const double* widths_P, int thin, int burn_in, uint64_t seed, double* cand_BxP, double* score_B,
                int32_t* starts_R, double* opt_hyp_RxP, double* opt_logpost_R, int64_t* opt_stats_Rx4,
                int32_t* opt_invalid_R, double* best_P, double* best_logpost, double* hyp_SxP, double* logpost_S,
                double* logprior_S, int64_t* stats_Sx4, double* noise_S, int32_t* status, double* alpha_SxN,
                double* L_SxNxN);

/* ---- a8: vbmc/variational_optimization.py:1238-1606 _gp_log_joint ------- */

/* G, dG (enabled blocks; sigma/lambda/w blocks only under jacobian_flag,
 * :1528-1546), and when compute_var: varG, var_ss (:1578-1596), I_sk (S x K),
 * J_sjk (S x K x K).  avg_flag as the reference (:1578).  Outputs nullable.
 * With avg_flag=0 or S==1 semantics: G_out/dG_out hold per-sample values laid
 * out [S] and [n_dG][S] like the reference's arrays.  compute_var with any
 * gradient -> VBMC_E_UNSUP (reference raises :1303-1307); compute_var==2 too. */
int vbmc_gp_log_joint(vbmc_ctx* ctx, int grad_flags, int avg_flag, int jacobian_flag,
                      int compute_var, double* G, double* dG, double* varG,
                      double* var_ss, double* I_SxK, double* J_SxKxK);

/* ---- a12: gpyreg GP.predict (third party) ------------ */

/* Per sample: fmu = m(x*) + K*^T alpha; fs2 = max(0, sf^2 - ||L^-T (sW o K*)||^2)
 * (L_chol) or max(0, sf^2 + diag(K*^T L K*)).  separate_samples: outputs (M x S)
 * row-major; else (M): mean over s and mean_s fs2 + var_s(fmu, ddof=1)
 * (the law restated at acquisition_functions/abstract_acq_fcn.py:82-97).
 * add_noise: adds exp(2 hyp_noise)*sn2_mult to the variance. */
int vbmc_gp_predict(vbmc_ctx* ctx, int64_t M, const double* xs_MxD, int add_noise,
                    int separate_samples, double* fmu, double* fs2);

/* ---- a9: the fused objective _neg_elcbo (:991-1235) ---------------------- */

typedef struct {
  /* inputs */
  int64_t ns_per_comp;  /* reference `Ns` (per component); 0 -> entlb           */
  int eps_mode;         /* VBMC_EPS_*                                            */
  uint64_t seed;        /* Philox seed                                           */
  int compute_grad;     /* reference compute_grad                                */
  int optimize_mask;    /* bit0..3 = vp.optimize_{mu,sigma,lambd,weights}        */
  int64_t row_begin;    /* antithetic-pair rows of every component evaluated by  */
  int64_t row_count;    /* this ctx; row_count < 0 -> the rank's even share       */
  /* soft bounds (theta_bnd), all nullable together (:1195-1229)                 */
  const double* bnd_lb; /* length n_bnd                                          */
  const double* bnd_ub;
  int n_bnd;
  double tol_con;
  double weight_threshold;
  double weight_penalty;
} vbmc_elbo_opts;

/* One evaluation of F = -G - H (+ bound / weight penalties) and dF with a single
 * device round trip: theta -> mixture (vbmc_theta_to_mixture), G/dG kernel,
 * entropy kernels, optional all-reduce, host finalisation.  theta's eta tail is
 * max-shifted IN PLACE like the reference does to its caller (:1082-1085).
 * Outputs: F, dF (n_theta; untouched if !compute_grad), G, H; mixture outputs as
 * in vbmc_theta_to_mixture (nullable). */
int vbmc_neg_elcbo(vbmc_ctx* ctx, double* theta, int n_theta, const vbmc_elbo_opts* opts,
                   double* F, double* dF, double* G, double* H, double* mu_KxD,
                   double* sigma_K, double* lambd_D, double* w_K, double* eta_K);

/* The same call with its twelve arguments in ONE block (no reference counterpart: the reference's call is a Python call).
 * A ctypes foreign call converts every argument on every call -- 1.8 us for the thirteen of vbmc_neg_elcbo against 0.3 us for
 * two, on the path between two evaluations of a polled step -- so a binding that keeps its buffers fills the block once
 * and passes its address.  Fields exactly as vbmc_neg_elcbo's parameters. */
typedef struct vbmc_elbo_call {
  double* theta;
  int n_theta;
  const vbmc_elbo_opts* opts;
  double* F;
  double* dF;
  double* G;
  double* H;
  double* mu_KxD;
  double* sigma_K;
  double* lambd_D;
  double* w_K;
  double* eta_K;
} vbmc_elbo_call;
int vbmc_neg_elcbo_call(vbmc_ctx* ctx, const vbmc_elbo_call* c);

/* ---- the sieve's batch of candidate evaluations ---------- */

/* B candidate parameter vectors (rows of thetas_BxN) through the call _sieve makes per
 * candidate (vbmc/variational_optimization.py:775-787): Ns = 0 (lower-bound entropy), no
 * gradient, soft bounds as in `opts`; F_B[b] = -G_b - H_b + bound losses.  opts->ns_per_comp
 * must be 0 and opts->compute_grad 0 (VBMC_E_UNSUP otherwise).  Unlike vbmc_neg_elcbo this
 * neither changes the ctx mixture nor touches the theta rows.  G_B / H_B nullable.  Everything per
 * candidate -- theta -> mixture -> pack, the GP sums, the entropy, G, the bound losses -- runs on the
 * device (four launches for the whole batch); VBMC_E_NONFINITE names the first non-finite candidate. */
int vbmc_neg_elcbo_batch(vbmc_ctx* ctx, const double* thetas_BxN, int B, int n_theta,
                         const vbmc_elbo_opts* opts, double* F_B, double* G_B, double* H_B);

/* ---- the stochastic optimiser's loop, device resident ---- */

/* minimize_adam (vbmc/minimize_adam.py:8-146) specialised to the objective PyVBMC gives it,
 * vb_train_mc_fun = _neg_elcbo(theta, gp, vp0, beta, ns_ent_K, compute_grad=True,
 * theta_bnd=...) (vbmc/variational_optimization.py:238-249).  theta, the Adam moments and
 * the mixture stay on the device; one iteration is four kernel launches and no
 * synchronisation -- or, at the sample counts optimize_vp really uses (ns_ent = 100 K^(2/3) in total,
 * option_configs/advanced_vbmc_options.ini:43), a whole vbmc_adam_run is ONE launch of resident workgroups
 * that exchange their results once per iteration (option "adam_fused").  The early-stopping decision (minimize_adam.py:107-140) stays with the
 * caller, who sees y_tab / x_tab after every vbmc_adam_run -- the reference only tests it
 * every 20 iterations.
 *
 * vbmc_adam_begin: theta0[n_theta] start point (not modified); `opts` as for vbmc_neg_elcbo
 *   (ns_per_comp even and > 0, compute_grad set; with VBMC_EPS_PHILOX iteration i draws
 *   from seed + i; with VBMC_EPS_RESIDENT every iteration reuses the resident draws);
 *   lb/ub[n_theta] the optional box of minimize_adam (both NULL = unbounded); max_iter and
 *   master_* as in the reference.  Non-optimised blocks keep the ctx mixture's values.
 * vbmc_adam_run: the next n_iters iterations.  y_tab_out[n_iters] = objective values
 *   (minimize_adam's y_tab slice), x_tab_out[n_iters][n_theta] = iterates after each update
 *   (rows; the reference stores them as columns), G_out/H_out[n_iters] the two terms of the
 *   objective.  All nullable.  VBMC_E_NONFINITE if an iterate became non-finite.  (If a workgroup of the
 *   one-launch form does not publish its results within 20 ms, the launch gives up with the state of the start
 *   of the batch intact and this call runs the batch -- and the rest of the run -- as four launches per iteration.)
 * vbmc_adam_end: ends the run; the ctx mixture becomes that of the last iterate (outputs as
 *   in vbmc_theta_to_mixture, nullable; theta_out = last x with its eta tail max-shifted).
 * Between begin and end no other entry point of the same ctx may be called. */
int vbmc_adam_begin(vbmc_ctx* ctx, const double* theta0, int n_theta, const vbmc_elbo_opts* opts,
                    const double* lb, const double* ub, int max_iter, double master_min,
                    double master_max, double master_decay);
/* vbmc_adam_run_auto: the rest of the optimisation -- up to max_iters iterations -- in ONE call, where the run has the
 *   one-launch form (option "adam_fused") and has not run an iteration yet (the kernel's stopping rule needs the
 *   mean iterate of the previous batch, which it collects itself from iteration 0 on): the workgroups apply
 *   minimize_adam's stopping rule themselves (minimize_adam.py:107-140: every 20 iterations from the 40th on, the
 *   slope of a straight-line fit through the last 20 objective values against its standard error and tol_fun, and
 *   the distance between the mean iterates of the last two batches) and *n_done returns how many iterations ran;
 *   outputs as vbmc_adam_run for those.  Returns VBMC_W_NOT_FUSED (and does nothing) otherwise. */
int vbmc_adam_run_auto(vbmc_ctx* ctx, int max_iters, double tol_fun, int* n_done, double* y_tab_out,
                       double* x_tab_out, double* G_out, double* H_out);
int vbmc_adam_run(vbmc_ctx* ctx, int n_iters, double* y_tab_out, double* x_tab_out,
                  double* G_out, double* H_out);
int vbmc_adam_end(vbmc_ctx* ctx, double* theta_out, double* mu_KxD, double* sigma_K,
                  double* lambd_D, double* w_K, double* eta_K, int* iterations);

/* ---- acquisition evaluation, pairwise distances -- */

/* Closed-form acquisition functions of the reference. */
enum {
  VBMC_ACQ_STD = 0,     /* AcqFcn        acquisition_functions/acq_fcn.py:38-45          */
  VBMC_ACQ_LOG = 1,     /* AcqFcnLog     acquisition_functions/acq_fcn_log.py:43-52      */
  VBMC_ACQ_VANILLA = 2, /* AcqFcnVanilla acquisition_functions/acq_fcn_vanilla.py:38-42  */
  VBMC_ACQ_NOISY = 3    /* AcqFcnNoisy   acquisition_functions/acq_fcn_noisy.py:33-41    */
};

/* The device part of AbstractAcqFcn.__call__ (acquisition_functions/abstract_acq_fcn.py:
 * 80-131) for M points in transformed space: gp.predict(separate_samples=True) with the GP
 * of vbmc_set_gp, f_bar / var_tot over the hyper-parameter samples (:82-97), the density of
 * the ctx mixture (vp.pdf(Xs, orig_flag=False[, log_flag=True])), the formula selected by
 * `kind` with y_max = function_logger.y_max, the variance regularisation (:112-128; off when
 * tol_gp_var <= 0) and the clamp at -realmax (:130-131).  sn2_M: per-point observation noise,
 * VBMC_ACQ_NOISY only.  Integer-variable rounding (:77-79) and the hard-bound mask
 * (:133-139) involve the caller's parameter transformer and stay on the host.
 * f_bar_M / var_tot_M nullable. */
int vbmc_acq_eval(vbmc_ctx* ctx, int64_t M, const double* xs_MxD, int kind, double y_max,
                  double tol_gp_var, const double* sn2_M, double* acq_M, double* f_bar_M,
                  double* var_tot_M);

/* The importance-sampled acquisition functions for noisy targets, AcqFcnVIQR
 * (acquisition_functions/acq_fcn_viqr.py:30-160) and AcqFcnIMIQR (acq_fcn_imiqr.py:29-177).
 *
 * vbmc_acq_is_set uploads, once per active-sampling round, what the reference keeps in
 * optim_state["active_importance_sampling"] (vbmc/active_importance_sampling.py:262-306) for the
 * GP of vbmc_set_gp (S samples, N points): the importance points Xa (Na x D, or S x Na x D with
 * per_sample_xa -- IMIQR after MCMC), C_tmp[s] = (K+Sigma)^-1 K(X, Xa) resp. L K(X, Xa) (S x N x Na;
 * for IMIQR, which stores K_Xa_X instead, the caller forms it the same way), the predictive
 * variances f_s2 at Xa (Na x S as the reference stores them) and ln_weights (S x Na; NULL = VIQR's
 * constant weights).
 * vbmc_acq_is_eval evaluates the acquisition at M points of the transformed space: predictive
 * variance at the points, posterior cross-covariance with Xa, tau2 = C^2 / (f_s2 + sn2), s_pred,
 * log-sum-exp over Xa and over the GP samples; sn2_M = observation noise at the points
 * (_estimate_observation_noise), u = norm.ppf(quantile).  Integer rounding and the hard-bound mask
 * stay on the host, as for vbmc_acq_eval. */
int vbmc_acq_is_set(vbmc_ctx* ctx, int64_t Na, const double* Xa, int per_sample_xa,
                    const double* Ctmp_SxNxNa, const double* fs2a_NaxS, const double* lnw_SxNa);
int vbmc_acq_is_eval(vbmc_ctx* ctx, int64_t M, const double* xs_MxD, const double* sn2_M, double u,
                     double* acq_M, double* var_tot_M /* nullable: for the variance regularisation */);

/* Preparing that state on the device: vbmc/active_importance_sampling.py, for the GP of vbmc_set_gp.
 *
 * vbmc_is_proposal is active_sample_proposal_pdf (:317-390) for Na points of the transformed space:
 * gp.predict(Xa, separate_samples=True) (:351); the log density of the smoothed posterior -- the mixture
 * (K2, mu2, sigma2, lambd2, w2), e.g. the 4 K components step 1 builds (:126-137) -- plus log w_vp (:361-366);
 * the box-uniform mixture around the training points, half-widths rect_delta_D, strict inequalities (:372-378);
 * their max-shifted log-sum-exp and ln_w = ln_y - l_pdf (:380-388), ln_y = f_mu when ln_y_is_fmu (IMIQR's
 * is_log_base) else 0 (VIQR's).  w_vp = 0: no mixture needed (NULLs); w_vp = 1: no boxes (rect_delta_D NULL),
 * ln_w = ln_y - lpdf directly.  Outputs lnw_NaxS and fs2_NaxS, (Na, S) as the reference returns them.
 * *invalid_out = 1 when some point lies in no box and has zero density: the reference raises
 * ValueError("Invalid value.") there (:381-382).  D <= 32 (VBMC_E_UNSUP above).
 *
 * vbmc_is_box_sample draws n_box box-uniform proposals (:164-168) from the Philox stream 5 of csrc/sample.hip:
 * sample n picks training point floor(u N) and adds (2 u_d - 1) rect_delta_d in every dimension.
 *
 * vbmc_acq_is_build is vbmc_acq_is_set with step 3 (:264-308) done on the device: from Xa (Na x D, or
 * S x Na x D with per_sample_xa), f_s2 (Na x S) and ln_weights (S x Na, NULL for VIQR) it forms, per GP sample,
 * K_Xa_X[s] = k_s(Xa, X) (:287) and C_tmp[s] = (L'L)^-1 K(X, Xa) / sn2_eff (:294-304, two products against
 * the resident L^-1) or L K(X, Xa) (:306), straight into the resident state vbmc_acq_is_eval reads.
 * K_out_SxNaxN / C_out_SxNxNa (nullable) receive copies, as the reference's dict holds them. */
int vbmc_is_proposal(vbmc_ctx* ctx, int64_t Na, const double* Xa_NaxD, int K2, const double* mu2_KxD,
                     const double* sigma2_K, const double* lambd2_D, const double* w2_K, double w_vp,
                     const double* rect_delta_D, int ln_y_is_fmu, double* lnw_NaxS, double* fs2_NaxS,
                     int* invalid_out);
int vbmc_is_box_sample(vbmc_ctx* ctx, int64_t n_box, uint64_t seed, const double* rect_delta_D, double* x_NboxxD);
int vbmc_acq_is_build(vbmc_ctx* ctx, int64_t Na, const double* Xa, int per_sample_xa, const double* fs2a_NaxS,
                      const double* lnw_SxNa, double* K_out_SxNaxN, double* C_out_SxNxNa);

/* The MCMC chains of step 2 (vbmc/active_importance_sampling.py:195-262) for the GP of vbmc_set_gp, all S of them in one
 * launch (csrc/acq_is_mcmc.hip): chain s samples the acquisition's is_log_full over gp.predict(add_noise=True) of the
 * one-sample GP s (:205-250),
 *     f(x) = [ln_y_fmu ? f_mu(x) : 0] + u_q f_s + log1p(-exp(-2 u_q f_s)),   f_s = sqrt(f_s2(x) + sn2 sn2_mult),
 * from x0_SxD[s] clipped into [lb_D, ub_D], with interval widths widths_D, and keeps n samples, one every `thin` sweeps
 * after `burn_in` sweeps (:211-249).  The sampler is this library's own (gpyreg's is not part of the reference tree):
 * Neal's coordinate-wise slice sampler, stepping out at most 32 evaluations a side and shrinking at most 64 times, on
 * the Philox stream 6 of csrc/sample.hip with key `seed` -- tests/slice_host.py states it in NumPy.
 * Outputs: X_SxnxD the kept points, logp_Sxn f at them, fmu_nxS / fs2_nxS the predictive mean and the noise-free
 * variance at them (what the reference's second predict, :254, returns), stats_Sx4 per chain the evaluations of f, the
 * draws consumed, and how often the step-out / the shrink cap ended a loop.  *invalid = 1 when f is not finite at some
 * chain's start: that chain writes nothing (the caller raises the reference's ValueError("Invalid value.")).
 * D <= 32 and N small enough for the chain's LDS (VBMC_E_UNSUP before anything is launched); n, thin >= 1, burn_in >= 0. */
int vbmc_is_mcmc(vbmc_ctx* ctx, int ln_y_fmu, double u_q, const double* x0_SxD, const double* widths_D,
                 const double* lb_D, const double* ub_D, int n, int thin, int burn_in, uint64_t seed,
                 double* X_SxnxD, double* logp_Sxn, double* fmu_nxS, double* fs2_nxS,
                 int64_t* stats_Sx4 /* evaluations, draws, step-out caps, shrink caps */, int* invalid);

/* AbstractAcqFcn._sq_dist (acquisition_functions/abstract_acq_fcn.py:195-222):
 * c[i][j] = max(|a_i - mu|^2 + |b_j - mu|^2 - 2 (a_i - mu).(b_j - mu), 0), mu the common
 * mean the reference subtracts first.  argmin_n (nullable) = np.argmin(c, axis=1), the
 * nearest-neighbour lookup of _estimate_observation_noise (:244-252); c_nxm nullable when
 * only the argmin is wanted.  D <= 32. */
int vbmc_sq_dist(vbmc_ctx* ctx, int64_t n, int64_t m, int D, const double* a_nxD,
                 const double* b_mxD, double* c_nxm, int64_t* argmin_n);

/* ---- the acquisition search of active_sample ------------- *
 *
 * vbmc/active_sample.py:310-349, 647-837: a set of M search points (transformed space) is drawn, scored with the
 * acquisition function and ranked.  The set stays in the context between the calls below: what goes in are the
 * bounds and a few D x D factors, what comes back is the ranked set.
 *
 * vbmc_search_fill fills the set from n_src sources, in order (M = the sum of their rows; D <= 32, M <= 2^20,
 * VBMC_E_UNSUP above, before anything is drawn):
 *   VBMC_SRC_COPY       data = rows x D host points, already in transformed space (the search cache, :716-722)
 *   VBMC_SRC_TRANSFORM  data = rows x D host points of the original space, put through the slot-0 transformer
 *                       (the cache rows x_orig, :706); without a transformer (use_xf = 0) they are copied
 *   VBMC_SRC_MIXTURE    rows balanced draws of the ctx mixture with `df`, as vbmc_mixture_sample_t draws them with
 *                       key `seed` (unshuffled; :728-730, :829)
 *   VBMC_SRC_AFFINE     data = [mean D | A D x D]: row r = z_r A + mean, z_r the standard normals of Philox stream 7
 *                       (csrc/sample.hip) at counter (r, pair) under key `seed` (:736-738, :782-784; the caller passes
 *                       as A the factor np.random.multivariate_normal forms of the covariance, sqrt(s)[:, None] * v of
 *                       its SVD -- pyvbmc_amd/active_search.py mvn_factor, which sets singular values below
 *                       s.max() * D * eps to zero first)
 *   VBMC_SRC_BOX        data = [lb D | ub D]: row r = z_r o (ub - lb) + lb, the same normals (:806-809)
 * Every row is then clamped to [lb_search_D, ub_search_D] (:836; both NULL: no clamp) and, when integer_bits is not
 * 0 (bit d = dimension d is an integer variable), rounded as AbstractAcqFcn._real2int does (abstract_acq_fcn.py:
 * 149-193): inverse transform, rint (half to even), forward transform, the integer columns replaced.  use_xf: 1 = the
 * slot-0 transformer applies (it must be set for D), 0 = the identity.  X_out_MxD (nullable) receives the set.
 * vbmc_search_put is the fill of one VBMC_SRC_COPY source without a clamp: host-drawn points become the set.
 *
 * vbmc_search_eval scores and ranks the set.  kind: VBMC_ACQ_STD .. VBMC_ACQ_NOISY as vbmc_acq_eval, or VBMC_ACQ_IS,
 * the importance-sampled acquisition of vbmc_acq_is_eval on the resident importance state (u = norm.ppf(quantile); the
 * variance regularisation and the clamp of abstract_acq_fcn.py:110-131 applied here too).  VBMC_ACQ_NOISY and
 * VBMC_ACQ_IS take the observation noise of every point from the nearest training input
 * (_estimate_observation_noise, :224-256): n_noise rows X_rescaled_NxD, sn2_new_N and length_scale_D, the set divided
 * by the length scale on the device (the lookup runs over the whole set in one pass: 2 M ceil(n_noise / 64) <= 2^28,
 * VBMC_E_UNSUP above).  Then +inf where the inverse-transformed point (use_xf as above) lies outside
 * [lb_eps_orig_D, ub_eps_orig_D] (:133-139), and the stable ascending order of (value, row), NaN last -- what
 * np.argsort(kind="stable") gives.  Outputs, each nullable: acq_M in set order, order_M, the set in that order. */
enum { VBMC_SRC_COPY = 0, VBMC_SRC_TRANSFORM = 1, VBMC_SRC_MIXTURE = 2, VBMC_SRC_AFFINE = 3, VBMC_SRC_BOX = 4 };
enum { VBMC_ACQ_IS = 4 };
typedef struct vbmc_search_source {
  int kind;
  int64_t rows;
  const double* data;
  double df;     /* VBMC_SRC_MIXTURE: degrees of freedom (+inf or 0: Gaussian) */
  uint64_t seed; /* key of the source's draws */
} vbmc_search_source;
int vbmc_search_fill(vbmc_ctx* ctx, int D, int n_src, const vbmc_search_source* src, const double* lb_search_D,
                     const double* ub_search_D, uint32_t integer_bits, int use_xf, double* X_out_MxD);
int vbmc_search_put(vbmc_ctx* ctx, int64_t M, int D, const double* X_MxD, uint32_t integer_bits, int use_xf);
int vbmc_search_eval(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                     const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                     const double* lb_eps_orig_D, const double* ub_eps_orig_D, double* acq_M, int64_t* order_M,
                     double* X_sorted_MxD);

/* ---- the local optimisation of the acquisition search: CMA-ES ------------- *
 *
 * vbmc/active_sample.py:355-423 with search_optimizer = "cmaes" (the reference's default): from the best ranked search
 * point the acquisition function is minimised in the box [lb_D, ub_D] (:366-375) by `cma.fmin` with tolfun (:377-380),
 * maxfevals = search_max_fun_evals and the initial step max(sqrt(diag Sigma)) (:383-389), thousands of single-point
 * acquisition calls from a Python optimiser.  vbmc_search_cmaes runs R such optimisations in lockstep on the device
 * (R = 1 is the reference's; with R > 1 a caller starts from the R best ranked points): every generation of all runs is
 * one batch of R lambda rows through the scoring launches of vbmc_search_eval.  The optimiser is this library's own
 * (csrc/cmaes.hip states it; there is no stream to be bit-compatible with: `cma` is a third-party package): a
 * (mu/mu_w, lambda)-CMA-ES with an explicit covariance whose Cholesky factor is recomputed every generation, candidates
 * clipped to the box, normals from Philox stream 8 under the key seed + (r + 1) 0x9E3779B97F4A7C15 of run r.  The
 * reference wraps its call in cma.NoiseHandler; the acquisition functions are deterministic, so there is no noise
 * handling here.  Every candidate is evaluated with its integer columns rounded as vbmc_search_fill rounds them
 * (abstract_acq_fcn.py:77-79, 149-193) and masked by the hard bounds (:133-139, +inf), while the unrounded point drives
 * the optimiser; the rounded point is what becomes the best.  The start itself is evaluated first (f0_R, one row).
 *
 * The scoring arguments (kind .. ub_eps_orig_D) are vbmc_search_eval's.  opts: lambda (0 = 4 + floor(3 ln D)),
 * max_fevals (the start counts), tol_fun, tol_x (<= 0: 1e-11 sigma0), seed.  Outputs, each nullable: the best evaluated
 * point and its value, the start's value, and the final mean, step size and covariance of every run; stats_Rx4 =
 * {generations, evaluations, stop reason, generation of the best (0: the start)}, stop reason 1 tolfun, 2 tolx,
 * 3 maxfevals, 4 condition (of the Cholesky factor), 5 invalid (a generation without a finite value).
 * Refused before anything is launched: VBMC_E_UNSUP for D > 32, D = 1 (the reference switches to Nelder-Mead there),
 * lambda > 64, R lambda above the search set's row cap (2^20); VBMC_E_ARG for R < 1, lambda < 4, sigma0 <= 0, a box that
 * is not finite or has lb > ub, a start outside the box, max_fevals < 1 + lambda, GP or mixture not set, a missing noise
 * table for the kinds that need it.  The host queues vbmc_set_option "cmaes_rounds" rounds (default 8) between two reads
 * of the count of runs not yet stopped.  The resident search set, the installed GP and the mixture are left as they are. */
typedef struct vbmc_cmaes_opts {
  int lambda;
  int64_t max_fevals;
  double tol_fun;
  double tol_x;
  uint64_t seed;
} vbmc_cmaes_opts;
int vbmc_search_cmaes(vbmc_ctx* ctx, int kind, double y_max, double tol_gp_var, double u, int64_t n_noise,
                      const double* X_rescaled_NxD, const double* sn2_new_N, const double* length_scale_D, int use_xf,
                      const double* lb_eps_orig_D, const double* ub_eps_orig_D, int R, const double* x0_RxD,
                      const double* sigma0_R, const double* lb_D, const double* ub_D, uint32_t integer_bits,
                      const vbmc_cmaes_opts* opts, double* x_best_RxD, double* f_best_R, double* f0_R, double* mean_RxD,
                      double* sigma_R, double* C_RxDxD, int64_t* stats_Rx4);

/* ---- the sieve of optimize_vp: candidates drawn, scored, ranked ----------- *
 *
 * vbmc/variational_optimization.py:660-810 (_sieve) builds init_N candidate posteriors with _vb_init (:813-988), scores
 * each with a value-only, lower-bound-entropy _neg_elcbo (:775-787) and sorts them (:789-792).  The context keeps one
 * resident set of candidate thetas (B x n_theta: the raw parameters get_parameters returns for a candidate,
 * variational_posterior.py:642-676, the eta tail max-shifted as _neg_elcbo leaves it, :1082-1085); between the calls
 * below the candidates exist only in device memory.
 *
 * vbmc_sieve_fill replaces _vb_init's loop (:882-986) and the get_parameters of :776.  The set is n1 candidates of type
 * 1 (the old parameters mu0 / sigma0 / lambd0 / w0 of K components; K_new - K components spawned next to old ones,
 * :898-914), n2 of type 2 (start mu2 / sigma2, :862-875: the caller orders y_star and makes the single sigma0 draw) and
 * n3 of type 3 (means gathered from X_star, sigma from their variance, :926-943; v3 = mean_d var(X_star[:, d], ddof=1) is
 * used instead when K == 1), in this order; lambd_s_D is the normalised std(X_star) form of lambd (:920-921, :946-947)
 * that types 2 and 3 take with optimize_lambd.  Candidate 0 of types 1 and 2 is left without jitter (:895-896, :917-918).
 * The draws: Z_BxS / I_BxKn are the host's (NumPy's stream; slot layout and index columns: csrc/sieve.hip), or, with
 * Z_BxS NULL, every draw is made on the device from Philox under `seed`, counter (candidate, slot) (streams 10-12 of
 * csrc/sample.hip's list).  thetas_out_BxN (nullable) receives the set.
 * Covered, VBMC_E_UNSUP otherwise, before anything is queued: D <= 32, K_new <= 128, optimize_sigma on, K_new >= K,
 * K_new > K only with optimize_mu, B <= 2^20, N_star within the generator's LDS (Philox type 3: about 3 700 points at
 * K_new D = 4 096).
 *
 * vbmc_sieve_put makes the rows of a host matrix the resident set (a caller's own candidates).
 *
 * vbmc_sieve_eval replaces the loop :775-787 and the sort :789-792: the scoring launches of vbmc_neg_elcbo_batch on the
 * resident set (the ctx mixture supplies D, K = K_new and the blocks that are not optimised; opts as there), then the
 * stable ascending order of F, NaN last (np.argsort(kind="stable")).  A candidate with a value that is not finite
 * scores NaN -- it is dropped by the order, not an error.  Outputs, each nullable: F, G, H in set order, the order, and
 * the thetas in rank order; one download. */
typedef struct vbmc_sieve_fill_args {
  int D, K, K_new, optimize_mask;
  int64_t n1, n2, n3;
  const double* mu0_KxD;
  const double* sigma0_K;
  const double* lambd0_D;
  const double* w0_K;
  const double* mu2_KnxD;  /* n2 > 0 */
  const double* sigma2_Kn; /* n2 > 0 */
  const double* lambd_s_D; /* n2 + n3 > 0 and optimize_lambd */
  int64_t N_star;
  const double* X_star_NxD; /* n3 > 0 and optimize_mu */
  double v3;
  const double* Z_BxS; /* host draws, or NULL: Philox under seed */
  int n_slot;          /* S = (K_new - K)(D + 2) + 3 K_new + D K_new + D */
  const int32_t* I_BxKn;
  uint64_t seed;
} vbmc_sieve_fill_args;
int vbmc_sieve_fill(vbmc_ctx* ctx, const vbmc_sieve_fill_args* args, double* thetas_out_BxN);
int vbmc_sieve_put(vbmc_ctx* ctx, int64_t B, int n_theta, const double* thetas_BxN);
int vbmc_sieve_eval(vbmc_ctx* ctx, const vbmc_elbo_opts* opts, double* F_B, double* G_B, double* H_B, int64_t* order_B,
                    double* thetas_sorted_BxN);

/* ---- the last stage of optimize_vp: full ELCBO and the pruning trials ------ *
 *
 * After the optimiser, vbmc/variational_optimization.py evaluates the full ELCBO with variance and per-component terms
 * (_eval_full_elcbo, :428-499: _neg_elcbo with compute_var and separate_K) and evaluates it again for every pruning
 * trial, on the posterior with one component removed (:322-378).  Removing a component leaves mu, sigma, lambd of the
 * others as they are and rescales their weights, so a trial's G, varG and var_ss are a re-weighting of the I_sk (S x K)
 * and J_sjk (S x K x K) of the first evaluation (:1578-1596); only the Monte-Carlo entropy is new.
 *
 * The context owns one RECORD: S, K0, I_sk and J_sjk at stride K0 in device memory of its own (later scratch use does
 * not touch it), the current mixture, and the alive list -- the columns of the record the current mixture's components
 * stand for, 0..K0-1 at first.
 *
 * vbmc_elcbo_full replaces one _eval_full_elcbo (:474-485 with :1080-1183): theta -> mixture (vbmc_theta_to_mixture),
 * the GP sums and, with compute_var, the variance launches of vbmc_gp_log_joint, the value-only entropy launches
 * (ns_per_comp > 0: Monte Carlo as vbmc_entmc, draws by eps_mode / seed; 0: the lower bound as vbmc_entlb), then the
 * re-weighting kernel; one stream wait.  out = nelbo, G, H, varF, varG, varH, var_ss (:1179-1183, :1578-1596; varH = 0
 * as there).  I_SxK, J_SxKxK nullable.  compute_var = 0 (skip_elbo_variance): no J in the record, variances 0.
 * theta's eta tail is max-shifted in place (:1082-1085).
 *
 * vbmc_elcbo_prune_trial evaluates the record's mixture without the component at position `drop` of the alive list
 * (:335-350): delete, get_parameters (variational_posterior.py:642-676), set_parameters (:720-756) -- the softmax of
 * the remaining log weights with max shift, the lambd / sigma renormalisation; the result becomes the context's mixture
 * (host copy included).  Entropy launches at K' = K_alive - 1, G / varG / var_ss from the re-weighting kernel over the
 * record.  No GP kernel is launched; seven doubles come down after one wait.  drop = -1 removes nothing: the record's
 * mixture as it is, evaluated from the record (after vbmc_elcbo_put: the values of the installed arrays).
 *
 * vbmc_elcbo_prune_accept makes the last trial's alive list and mixture the record's (:365-376).
 *
 * vbmc_elcbo_put installs a record from host arrays with the context's current mixture (K0 components) as its mixture;
 * J_SxK0xK0 NULL = a record without variance.
 *
 * vbmc_elcbo_record_info: info = S, K0, K_alive, launches of the GP expected log joint (its sums, its variance) queued
 * on this context since the record was made, stream waits of this context since then; alive_K0 (nullable) receives the
 * K_alive alive columns.
 *
 * The re-weighting kernel (csrc/elcbo_full.hip) restates the host loop of vbmc_gp_log_joint (csrc/api_gp.hip, :1578-1596):
 * upper triangle j <= k, both clamps at np.spacing(1).  D <= 32, K <= 128, else VBMC_E_UNSUP. */
int vbmc_elcbo_full(vbmc_ctx* ctx, double* theta, int n_theta, int optimize_mask, int64_t ns_per_comp, int eps_mode,
                    uint64_t seed, int compute_var, double out[7], double* I_SxK, double* J_SxKxK);
int vbmc_elcbo_prune_trial(vbmc_ctx* ctx, int drop, int64_t ns_per_comp, int eps_mode, uint64_t seed, double out[7]);
int vbmc_elcbo_prune_accept(vbmc_ctx* ctx);
int vbmc_elcbo_put(vbmc_ctx* ctx, int S, int K0, const double* I_SxK0, const double* J_SxK0xK0);
int vbmc_elcbo_record_info(const vbmc_ctx* ctx, int64_t info[5], int32_t* alive_K0);

/* ---- sampling and its Monte-Carlo consumers -------------- */

/* VariationalPosterior.sample in transformed space, Gaussian components
 * (variational_posterior/variational_posterior.py:241-363 with orig_flag=False, df=inf):
 * x_n = mu_i + (lambda o z_n) sigma_i, i from the weights (np.random.choice, :316-319) or, with
 * balance_flag, split exactly by floor(w N) plus remainder draws (:296-313).  Draws come from
 * the counter-based Philox generator keyed by (seed, n) -- not NumPy's stream -- so sample n
 * is reproducible on its own; unlike the reference the balanced samples are NOT shuffled
 * (grouped by component).  x_NxD / comp_N nullable. */
int vbmc_mixture_sample(vbmc_ctx* ctx, int64_t N, uint64_t seed, int balance_flag, double* x_NxD,
                        int32_t* comp_N);
/* The same with multivariate Student-t tails of `df` degrees of freedom (:329-340, :345-353):
 * x_n = mu_i + lambda o z_n * t_n * sigma_i with t_n = (df/2) / sqrt(G_n), G_n ~ Gamma(df/2, scale
 * df/2) (Marsaglia-Tsang on Philox stream 4, one variate per sample).  df = +inf or 0: Gaussian
 * (vbmc_mixture_sample); df < 0 -> VBMC_E_ARG (numpy's gamma raises on a negative shape too). */
int vbmc_mixture_sample_t(vbmc_ctx* ctx, int64_t N, uint64_t seed, int balance_flag, double df,
                          double* x_NxD, int32_t* comp_N);

/* VariationalPosterior.kl_div, Monte-Carlo branch (gauss_flag=False, :1107-1126), between
 * the ctx mixture (vp1) and a second mixture over the same D: N balanced samples of each
 * (seed, seed+1), both densities, the reference's zero-density replacement rules, and
 * kl_out = max(0, [KL(vp1||vp2), KL(vp2||vp1)]).  Evaluated in transformed space, which equals
 * the reference's original-space value when both posteriors share one parameter transformer
 * (the Jacobians cancel in log q2 - log q1). */
int vbmc_kl_div_mc(vbmc_ctx* ctx, int64_t N, uint64_t seed, int K2, const double* mu2_KxD,
                   const double* sigma2_K, const double* lambd2_D, const double* w2_K,
                   double kl_out[2]);

/* ---- parameter transformer (parameter_transformer/parameter_transformer.py) ----
 *
 * The reference's ParameterTransformer on the device, so that VariationalPosterior's original-space
 * calls run there.  A ctx holds two descriptors: slot 0 belongs to the ctx mixture, slot 1 to the second
 * mixture of vbmc_kl_div_mc_orig.  The descriptor is the transformer's fields: per-dimension type_D
 * (0 unbounded, 3 logit, 12 probit, 13 student4 -- the reference's float codes, :81-114), lb / ub
 * (lb_orig / ub_orig), mu / delta (the centring), and the optional rotoscaling R_mat (D x D, row-major)
 * and scale (D); pass NULL for a field the transformer holds as None.  Bounded dimensions need finite
 * lb < ub.  D <= 32 (VBMC_E_UNSUP above).  Setting the values a slot already holds uploads nothing. */
int vbmc_set_transformer(vbmc_ctx* ctx, int slot, int D, const double* type_D, const double* lb_D,
                         const double* ub_D, const double* mu_D, const double* delta_D,
                         const double* R_DxD, const double* scale_D);
int vbmc_clear_transformer(vbmc_ctx* ctx, int slot);

/* Slot 0's transformer on n host points: direction 0 = __call__ (x -> u, out n x D), 1 = inverse
 * (u -> x, out n x D), 2 = log_abs_det_jacobian (u, out n) (:135-269). */
enum { VBMC_XF_FORWARD = 0, VBMC_XF_INVERSE = 1, VBMC_XF_LOG_ABS_DET = 2 };
int vbmc_transform(vbmc_ctx* ctx, int64_t n, int direction, const double* in_nxD, double* out);

/* vbmc_mixture_sample_t's samples (same Philox stream, same seed -> same transformed draws), returned
 * through slot 0's inverse: VariationalPosterior.sample(orig_flag=True) (:355-362). */
int vbmc_mixture_sample_orig(vbmc_ctx* ctx, int64_t N, uint64_t seed, int balance_flag, double df,
                             double* x_NxD, int32_t* comp_N);

/* VariationalPosterior.pdf(orig_flag=True) (:429-439, :543-559): rows strictly inside slot 0's bounds
 * (every dimension) are transformed, their density taken in u and log|J| subtracted (log_flag) or
 * exp(log|J|) divided out; rows outside are 0 / -inf, their density (and gradient row) taken at the
 * original coordinates with non-finite ones replaced by 0.  dy: the transformed-space gradient rows,
 * as the reference returns them.  log_flag with grad_flag is VBMC_E_UNSUP, as in the reference. */
int vbmc_mixture_pdf_orig(vbmc_ctx* ctx, int64_t n, const double* x_nxD, int log_flag, int grad_flag,
                          double df, double* y_n, double* dy_nxD);

/* VariationalPosterior.moments(orig_flag=True) (:791-796): N balanced samples (vbmc_mixture_sample_orig's,
 * balance_flag = 1) inverse-transformed, their mean and (cov_flag) the two-pass ddof = 1 covariance of
 * np.cov, on the device.  cov_DxD is written in full (symmetric). */
int vbmc_mixture_moments_orig(vbmc_ctx* ctx, int64_t N, uint64_t seed, int cov_flag, double* mean_D,
                              double* cov_DxD);

/* vbmc_kl_div_mc between posteriors with different transformers (slot 0: the ctx mixture's, slot 1: the
 * second mixture's), in original space as the reference computes it (:1107-1126): samples of each mixture
 * (seed, seed + 1) through their own inverse, then both densities in their own transformed spaces with
 * their Jacobians and bound masks, the zero-replacement rules, kl_out = max(0, [KL12, KL21]). */
int vbmc_kl_div_mc_orig(vbmc_ctx* ctx, int64_t N, uint64_t seed, int K2, const double* mu2_KxD,
                        const double* sigma2_K, const double* lambd2_D, const double* w2_K,
                        double kl_out[2]);

/* ---- kernel density estimate and marginal total variation (stats/kde_1d.py, mtv) ----
 *
 * kde_1d (stats/kde_1d.py:144-257) for a batch of ncol columns of n host samples each (column c at
 * x_colxn + c * n), mesh n_mesh (a power of two, <= 2^14: VBMC_E_UNSUP above).  lb_col / ub_col: the
 * bounds per column, or NULL to derive them as min - 0.1 (max - min) / max + 0.1 (max - min) (:218-225).
 * Every column is sorted on the device; from it the mesh, the bin counts (_linear_binning, :6-31),
 * len(np.unique), the DCT, the bandwidth of _root / _fixed_point (:34-108, scipy's brentq restated) or,
 * when that fails, Scott's rule (:111-130), and the density (:236-257).  Out: density and xmesh
 * (ncol x n_mesh; xmesh nullable), the bandwidth per column, and info_colx2 = {len(np.unique(column)),
 * flags}: 1 Scott's rule was used, 4 the mesh is degenerate (dx == 0 or non-finite: the reference
 * raises IndexError), 8 _root stopped where the reference would repeat the same brentq call forever
 * (Scott's rule used).  A non-finite sample -> VBMC_E_NONFINITE (the reference computes garbage). */
int vbmc_kde_1d(vbmc_ctx* ctx, int ncol, int64_t n, const double* x_colxn, int n_mesh, const double* lb_col,
                const double* ub_col, double* density_colxm, double* xmesh_colxm, double* bandwidth_col,
                int64_t* info_colx2);

/* One side of vbmc_mtv: host samples (x_NxD, row-major), or the N balanced draws of the ctx mixture through
 * transformer slot 0 / of the second mixture through slot 1 -- the samples of vbmc_mixture_sample_orig
 * with `seed`, which stay on the device.  lb_D / ub_D: the transformer's lb_orig / ub_orig (+-inf for
 * samples, :974-975). */
enum { VBMC_MTV_HOST = 0, VBMC_MTV_MIX1 = 1, VBMC_MTV_MIX2 = 2 };
typedef struct vbmc_mtv_side {
  int source;
  int64_t n;
  const double* x_NxD;
  uint64_t seed;
  const double* lb_D;
  const double* ub_D;
} vbmc_mtv_side;

/* VariationalPosterior.mtv (variational_posterior.py:921-1030): per dimension, the kde_1d density of each
 * side on 2^13 points within max(min - range/10, lb) .. min(max + range/10, ub) (:978-990), normalised
 * by its trapezoid sum (:996-1002), the not-a-knot cubic spline of each (interp1d kind="cubic", 0 outside
 * its mesh), and 0.5 * the trapezoid of |s1 - s2| over the three linspace(bb[j], bb[j+1], 1e5) segments of
 * the sorted mesh ends (:1018-1029).  The second mixture (mu2 .. w2, K2) is needed only by a
 * VBMC_MTV_MIX2 side.  All 2 D columns run at once; mtv_D gets the D distances and info_2Dx2 (nullable)
 * vbmc_kde_1d's info per column (side 1's D columns, then side 2's).  A non-finite sample ->
 * VBMC_E_NONFINITE. */
int vbmc_mtv(vbmc_ctx* ctx, int D, const vbmc_mtv_side* s1, const vbmc_mtv_side* s2, int K2,
             const double* mu2_KxD, const double* sigma2_K, const double* lambd2_D, const double* w2_K,
             double* mtv_D, int64_t* info_2Dx2);

/* ---- marginals of the variational posterior: the numbers of a corner plot ----
 *
 * VariationalPosterior.plot's call of corner.corner (variational_posterior.py:1191-1206): the D one-dimensional and
 * P = D (D - 1) / 2 two-dimensional histograms of n samples, here with the order-statistic quantiles, the
 * highest-density levels of every pair and the kde_1d curve of every column, in one call with one download.
 * src: the samples, a vbmc_mtv_side -- VBMC_MTV_HOST: x_NxD uploaded; VBMC_MTV_MIX1: the n draws of the ctx mixture,
 * unbalanced (vbmc_mixture_sample_t with `seed`), through transformer slot 0 when orig_flag
 * (vbmc_mixture_sample_orig), which stay on the device; lb_D / ub_D are not read.  1 <= D <= 32, 1 <= bins <= 128,
 * 1 <= n <= 2^22: VBMC_E_UNSUP beyond.  ranges_Dx2: (lo, hi) per dimension, lo < hi finite, or (NaN, NaN) for the
 * column's own [min, max] ((min - 0.5, max + 0.5) when they are equal).  Binning is np.histogram's / np.histogram2d's:
 * edges = linspace(lo, hi, bins + 1), a sample at hi in the last bin, a sample outside a dimension's range left out of
 * that dimension's histogram and of every pair with it.  Out: edges (D x (bins + 1)), counts1 (D x bins), counts2
 * (P x bins x bins, pair p = (i, j), i < j, row-major order; [p][a][b] = dimension i in bin a, j in bin b), inside2
 * (P: the sum of counts2[p]), quantiles (nq x D: np.quantile's linear rule at q_nq), and per pair and level l of
 * levels_nl: level_counts (P x nl), the count of the last cell of the shortest non-empty prefix of the cells sorted by
 * count, descending, whose sum is >= l inside2[p], and level_mass (P x nl), the sum of the cells with at least that
 * count over inside2[p] (NaN when inside2[p] is 0).  kde_mesh: 0, or 2^10 for kde_x, kde_density (D x 2^10) and
 * kde_bandwidth (D): vbmc_kde_1d of every column with its range as the bounds.  stage_ms (nullable): six times between
 * events -- samples, sort and columns, kde, bin indices, pair histograms, levels.  A non-finite sample ->
 * VBMC_E_NONFINITE. */
int vbmc_marginals(vbmc_ctx* ctx, int D, const vbmc_mtv_side* src, int orig_flag, int bins, const double* ranges_Dx2,
                   int nq, const double* q_nq, int nl, const double* levels_nl, int kde_mesh, double* edges,
                   int64_t* counts1, int64_t* counts2, int64_t* inside2, double* quantiles, int64_t* level_counts,
                   double* level_mass, double* kde_x, double* kde_density, double* kde_bandwidth, float* stage_ms);

/* ---- mode of the variational posterior (variational_posterior.py:810-919) ----
 *
 * VariationalPosterior.mode: n_opts rounds, each "n candidates (+ the K component centres in round 0), the one
 * with the highest log-density starts a local search"; the best round's point is the mode.  The mixture and the
 * transformer (slot 0, needed when orig_flag) are the ones set in the context.  Candidates: cand_RxnxD, a host
 * array of n_opts x n x D points in the requested space (the reference's self.sample(n, orig_flag) per round),
 * or NULL = round r draws the n samples of vbmc_mixture_sample / vbmc_mixture_sample_orig(n, seed + r,
 * balance_flag 0) in the kernel, never stored.  Start selection: highest value, ties to the lowest index, a
 * NaN value never wins.  The local search (csrc/mode.hip) replaces SciPy's minimize (:906-908) by a monotone
 * ascent with analytic derivatives -- safeguarded Newton steps, mean-shift (transformed space) or projected
 * gradient (original space, inside the reference's L-BFGS-B box lb + sqrt(eps) .. ub - sqrt(eps), :888-898)
 * otherwise -- until a step is <= step_tol max(1, |y|_inf) or max_iter iterations.  The original-space
 * objective assumes an orthogonal rotation matrix (the caller's check).
 * Out: x_D and its log-density f_out (nullable; pdf(x, orig_flag, log_flag=True)); rec_Rx5 (nullable), per
 * round {start index, start value, final value, iterations, status: 0 converged, 1 converged on a bound, 2
 * iteration cap}; pts_RxD (nullable), the rounds' final points, and ys_RxD (nullable), the same in the search
 * coordinates.  With a host array all n_opts x n x D candidates are uploaded in one piece (n_opts = 37, D = 32:
 * 0.95 GB of device scratch); n <= 2^24.  D > 32 -> VBMC_E_UNSUP. */
int vbmc_mixture_mode(vbmc_ctx* ctx, int n_opts, int orig_flag, int64_t n, const double* cand_RxnxD,
                      uint64_t seed, int max_iter, double step_tol, double* x_D, double* f_out,
                      double* rec_Rx5, double* pts_RxD, double* ys_RxD);

/* ---- input warping / rotoscaling (whitening/whitening.py:7-375) ----
 *
 * The composed map "old inference space -> original space -> new inference space" on the device.  Transformer slot 0
 * holds the OLD transformer, slot 1 the NEW one (vbmc_set_transformer), both of dimension D <= 32 (VBMC_E_UNSUP above,
 * before any launch).  FP64 throughout; every reduction runs in a fixed order, so a call is bit-reproducible.  A `source`
 * argument says which space the input points are in:
 *   VBMC_WARP_FROM_OLD   slot 0's inference space:  y = new(old^-1(x))          (needs both slots)
 *   VBMC_WARP_FROM_ORIG  the original space:        y = new(x)                  (slot 1 only)
 *   VBMC_WARP_IN_NEW     slot 1's inference space:  y = x (for the log-Jacobian at a given point; slot 1 only) */
enum { VBMC_WARP_FROM_OLD = 0, VBMC_WARP_FROM_ORIG = 1, VBMC_WARP_IN_NEW = 2 };

/* n points mapped as `source` says: warp_input's re-map of the training set (:191-200) and of the search cache
 * (:221-223), the dy / dy_old terms of warp_gp_and_vp (:309-313, :331-332, :369-370).  Outputs, all nullable:
 * y_NxD, lj_new_N = log|det J| of slot 1 at y, lj_old_N = log|det J| of slot 0 at x (VBMC_WARP_FROM_OLD only:
 * VBMC_E_ARG otherwise).  n = 0 returns at once, nothing launched. */
int vbmc_warp_points(vbmc_ctx* ctx, int D, int64_t n, int source, const double* x_NxD, double* y_NxD, double* lj_new_N,
                     double* lj_old_N);

/* unscent_warp (:7-77) with the warp fixed to new(old^-1(.)): base points x_NxD, scales sigma (sigma_rows x D,
 * sigma_rows = n or 1: one row is broadcast, :50-53).  Per base point the U = 2 D + 1 sigma points x, x +- sqrt(D)
 * sigma_d e_d are warped; mean_NxD is their mean and std_NxD their ddof = 1 standard deviation, taken in two passes
 * about the mean, both summed in the order u = 0 .. U - 1.  pts_UxNxD (nullable): the warped points in the
 * reference's layout.  n >= 1; sigma_rows other than 1 or n -> VBMC_E_ARG. */
int vbmc_warp_unscent(vbmc_ctx* ctx, int D, int64_t n, const double* x_NxD, int64_t sigma_rows, const double* sigma,
                      double* mean_NxD, double* std_NxD, double* pts_UxNxD);

/* The GP branch of warp_gp_and_vp (:296-313) for all S hyper-parameter samples in one launch: per sample s and
 * training point X_n the unscented warp with ell_s = exp(hyp_SxP[s][0 .. D)) (the host's libm), then
 * logell_SxD[s] = mean_n log(ell_new) (:303).  Also mean_n of dy = log|det J| of slot 1 at new(old^-1(X_n)) and of
 * dy_old = log|det J| of slot 0 at X_n (dy_mean, dy_old_mean: one double each, nullable; ConstantMean, :309-313).
 * The means over n are sums in a fixed order divided by N.  N >= 1, S >= 1, P >= D; a state of more than 2^27 doubles
 * -> VBMC_E_UNSUP. */
int vbmc_warp_gp(vbmc_ctx* ctx, int D, int N, int S, int P, const double* X_NxD, const double* hyp_SxP,
                 double* logell_SxD, double* dy_mean, double* dy_old_mean);

/* warp_input's box statistics (:168-180, :208-219): n uniform draws in the box [lo_D, hi_D], u (hi - lo) + lo, mapped
 * as `source` says.  The uniforms u_NxD are the caller's (np.random.rand(n, D)), or NULL = drawn on the device: draw i's
 * dimensions 2 p, 2 p + 1 are the two 53-bit uniforms of Philox block (i, p, stream 9) under `seed` (the streams are
 * listed in csrc/sample.hip).  mode 0: out_2xD = the 0.05 and 0.95 quantiles per dimension by np.quantile's default rule
 * (linear interpolation between the exact order statistics: the columns are sorted); mode 1: the minimum and maximum.
 * sorted_Dxn (nullable, mode 0): the sorted columns.  1 <= n <= 2^30; a non-finite mapped value -> VBMC_E_NONFINITE
 * (mode 0). */
int vbmc_warp_box(vbmc_ctx* ctx, int D, int64_t n, int source, const double* lo_D, const double* hi_D,
                  const double* u_NxD, uint64_t seed, int mode, double* out_2xD, double* sorted_Dxn);

/* ---- multi-GPU: one process per GPU, one collective ---------- */

/* 128-byte RCCL unique id, created on rank 0 and shipped to the other ranks by
 * the host launcher (file / env / any side channel). */
int vbmc_comm_unique_id(uint8_t id_out[128]);
/* Join the communicator: after this, vbmc_entmc / vbmc_neg_elcbo all-reduce the
 * raw entropy accumulator over `world` ranks. */
int vbmc_comm_init(vbmc_ctx* ctx, const uint8_t id[128], int rank, int world);
int vbmc_comm_destroy(vbmc_ctx* ctx);
/* Rank and size of the communicator as RCCL reports them (ncclCommUserRank / ncclCommCount);
 * 0 and 1 without a communicator.  bench.py prints the size as `comm_world` so a multi-GPU
 * line can be checked against the ranks that really took part. */
int vbmc_comm_info(vbmc_ctx* ctx, int* rank_out, int* world_out);
/* Device-side barrier + max over ranks of a host double (bench timing). */
int vbmc_comm_allreduce_max(vbmc_ctx* ctx, double* value_inout);
int vbmc_comm_barrier(vbmc_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* VBMC_HIP_H */
