// Internal declarations shared by the translation units of libvbmc_hip.so.
// Not part of the ABI (that is include/vbmc_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/vbmc_hip.h"
#include "gp_cand_host.h"
#include "gp_fit_host.h"
#include "scratch.h"
#include "transform.h"

struct ncclComm;

// Device-resident copy of the mixture, laid out for the kernels.
// One contiguous allocation of doubles; offsets below in units of double.
struct MixLayout {
  int D = 0, K = 0;
  int o_mup = 0;    // [K][D]  mu_dk / lambda_d   (means in lambda-scaled coordinates)
  int o_mu = 0;     // [K][D]  mu_dk
  int o_is2 = 0;    // [K]     1 / sigma_k^2
  int o_wc = 0;     // [K]     w_k * nconst / sigma_k^D   (nconst = (2pi)^(-D/2) / prod lambda)
  int o_rc = 0;     // [K]     nconst / sigma_k^D
  int o_lrc = 0;    // [K]     log2(nconst / sigma_k^D)
  int o_sig = 0;    // [K]     sigma_k
  int o_w = 0;      // [K]     w_k
  int o_lam = 0;    // [D]     lambda_d
  int o_ilam = 0;   // [D]     1 / lambda_d
  int total = 0;
  void plan(int D_, int K_) {
    D = D_;
    K = K_;
    int o = 0;
    o_mup = o; o += K * D;
    o_mu = o; o += K * D;
    o_is2 = o; o += K;
    o_wc = o; o += K;
    o_rc = o; o += K;
    o_lrc = o; o += K;
    o_sig = o; o += K;
    o_w = o; o += K;
    o_lam = o; o += D;
    o_ilam = o; o += D;
    total = o;
  }
};

// theta = [mu (K D) | ln sigma (K) | ln lambda (D) | eta (K)], each block present when its bit of the optimise mask
// (1, 2, 4, 8) is set: where the blocks start, which entry of the raw entropy vector [H | d mu | d sigma | d lambda | d w]
// and which coordinate of the extended soft-bound vector [mu | ln sigma + ln lambda | eta] belongs to an entry.  Kernels
// build it at the top of their body, where its values are wave-uniform locals.
struct ThetaMap {
  int D, K;
  int mask;
  __host__ __device__ bool o_mu() const { return mask & 1; }
  __host__ __device__ bool o_sg() const { return mask & 2; }
  __host__ __device__ bool o_lm() const { return mask & 4; }
  __host__ __device__ bool o_w() const { return mask & 8; }
  int p_sg, p_lm, p_w;  // first entry of the sigma, lambda and eta blocks (mu starts at 0)
  int n_sc;             // entries of the extended soft-bound vector's scale block: the (D,K) array of ln scales if sigma or lambda
  __host__ __device__ ThetaMap(int D_, int K_, int mask_) : ThetaMap(D_, K_, mask_, 0) { p_w = n_theta() - K; }
  // (n_theta: of a caller that holds it already)
  __host__ __device__ ThetaMap(int D_, int K_, int mask_, int n_theta_)
      : D(D_), K(K_), mask(mask_), p_sg((mask_ & 1) ? D_ * K_ : 0), p_lm(p_sg + ((mask_ & 2) ? K_ : 0)), p_w(n_theta_ - K_),
        n_sc((mask_ & 6) ? D_ * K_ : 0) {}
  __host__ __device__ int n_theta() const { return p_lm + (o_lm() ? D : 0) + (o_w() ? K : 0); }
  // the extended soft-bound vector: mu | ln scale | eta
  __host__ __device__ int n_bnd() const { return p_sg + n_sc + (o_w() ? K : 0); }
  // the block theta index i lies in (tested in this order; what is left is the eta block)
  __host__ __device__ bool in_mu(int i) const { return o_mu() && i < D * K; }
  __host__ __device__ bool in_sg(int i) const { return o_sg() && i >= p_sg && i < p_sg + K; }
  __host__ __device__ bool in_lm(int i) const { return o_lm() && i >= p_lm && i < p_lm + D; }
  __host__ __device__ int raw_w() const { return 1 + D * K + K + D; }  // weight block of the raw vector
  __host__ __device__ int raw_index(int i) const {
    if (o_w() && i >= p_w) return raw_w() + (i - p_w);
    if (o_lm() && i >= p_lm) return 1 + D * K + K + (i - p_lm);
    if (o_sg() && i >= p_sg) return 1 + D * K + (i - p_sg);
    return 1 + i;
  }
  // coordinate i of the extended soft-bound vector; sigma / lambda: the attributes, for the blocks theta does not carry
  __host__ __device__ double bound_coord(int i, const double* theta, const double* sigma, const double* lambda) const {
    double x;
    if (i < p_sg) {
      x = theta[i];
    } else if (i < p_sg + n_sc) {
      const int q = i - p_sg, k = q / D, d = q - k * D;  // ravel('F') of the (D,K) array
      const double ls = o_sg() ? theta[p_sg + k] : log(sigma[k]);
      const double ll = o_lm() ? theta[p_lm + d] : log(lambda[d]);
      x = ll + ls;
    } else {
      x = theta[p_w + (i - p_sg - n_sc)];
    }
    return x;
  }
};

struct GpState {
  bool set = false;
  int N = 0, D = 0, S = 0, P = 0, mean_kind = 0;
  std::vector<double> hyp;       // S x P (host copy)
  std::vector<int32_t> L_chol;   // S
  std::vector<double> sn2_eff;   // S  (1 / sW[0]^2)
  std::vector<double> sn2_mult;  // S
  double* d_X = nullptr;      // N x D
  double* d_XT = nullptr;     // D x N: the same, transposed (glj_block.h reads a dimension of consecutive points)
  double* d_alpha = nullptr;  // S x N
  double* d_L = nullptr;      // S x N x N
  double* d_Linv = nullptr;   // S x N x N : inverse of the upper Cholesky factor (L_chol samples)
  double* d_LinvP = nullptr;  // S x ld x ld, ld = predict_ld(N): the same, zero padded (predict_var_dma_kernel)
  double* d_sW = nullptr;     // S x N
  double* d_hyp = nullptr;    // S x P
  double* d_xc = nullptr;     // D : column means of X (centre of the pairwise-distance expansion)
  double* d_smeta = nullptr;  // S x 3 : (L_chol as 0/1, sn2_mult, 1/sn2_eff) per sample, for kernels batched over s
  size_t cap_X = 0, cap_XT = 0, cap_alpha = 0, cap_L = 0, cap_Linv = 0, cap_LinvP = 0, cap_sW = 0, cap_hyp = 0, cap_xc = 0, cap_smeta = 0;
  std::vector<double> h_small;  // host source of the xc / smeta uploads
  std::vector<double> h_XT;     // host source of the d_XT upload
  // a posterior built on the device (api_gp_post.hip): what vbmc_gp_append needs on top of the above
  bool dev_built = false;       // installed by vbmc_gp_posterior / vbmc_gp_append (vbmc_set_gp clears it)
  bool homo = false;            // every point's noise variance is its sample's constant: a point can be appended
  double* d_y = nullptr;        // N
  double* d_r = nullptr;        // S x N : y - m_s(X)
  double* d_sn2 = nullptr;      // S x N : noise variance per point
  double* d_sl = nullptr;       // S : sn2_div * sn2_mult, the scale of A = K / sl + diag(sn2 / sn2_div)
  size_t cap_y = 0, cap_r = 0, cap_sn2 = 0, cap_sl = 0;
  std::vector<double> h_X, h_y, h_sl;  // host copies: X (N x D), y (N), sl (S)
  std::vector<double> h_sn2;           // host copy of d_sn2 (S x N): vbmc_gp_append_noisy extends it by a column
};

// per-sample results of the GP expected log joint on the host (api_gp.hip glj_finalize)
struct GljHost {
  std::vector<double> G;        // S
  std::vector<double> I_sk;     // S x K
  std::vector<double> mu;       // S x (K*D)   d/dmu, 'F' order (K blocks of D)
  std::vector<double> sigma;    // S x K       pre-Jacobian
  std::vector<double> lambd;    // S x D
  std::vector<double> w;        // S x K  (= I_sk)
};

// host scratch of one fused evaluation, kept in the context so that the hot call allocates nothing
struct ElboScratch {
  GljHost glj;
  std::vector<double> dG, dH, dF, dFb, mu, sg, lm, wg, ext, dL, wpen, jw;
};

// The timed intervals of vbmc_last_kernel_ms (the numbers are ABI): entmc, glj, pdf, predict, elbo, predict's variance
// product (timing level 2 only), the GP posterior's factorisation, the MCMC chains of vbmc_is_mcmc, one chunk of
// vbmc_gp_lml (factorisation and gradient kernels), the three phases of the acquisition search (vbmc_search_fill's
// launches; vbmc_search_eval's acquisition and mask; its sort and gather), all the rounds of one vbmc_gp_hyp_sample, all the rounds of one vbmc_search_cmaes,
// all the rounds of one vbmc_gp_hyp_optimize, the three phases of the sieve (vbmc_sieve_fill's launch; vbmc_sieve_eval's scoring
// launches; its rank and gather)
enum TimingPair { T_ENTMC = 0, T_GLJ, T_PDF, T_PREDICT, T_ELBO, T_PREDICT_VAR, T_GP_POST, T_IS_MCMC, T_GP_LML, T_SEARCH_FILL,
                  T_SEARCH_EVAL, T_SEARCH_SORT, T_GP_HYP, T_SEARCH_CMAES, T_GP_OPT, T_SIEVE_FILL, T_SIEVE_SCORE, T_SIEVE_RANK, T_COUNT };

struct vbmc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2 * T_COUNT] = {};  // pair p of TimingPair below is (ev[2 p], ev[2 p + 1])
  bool ev_valid[T_COUNT] = {};
  std::string err;
  hipDeviceProp_t prop;

  // mixture (host copies are authoritative for finalisation arithmetic)
  bool mix_set = false;
  int D = 0, K = 0;
  std::vector<double> mu, sigma, lambd, w, eta;  // mu is K x D
  MixLayout ml;
  double* d_mix = nullptr;
  // Armed evaluation (api_elbo.hip): the three launches of the NEXT host-driven evaluation are queued
  // while the current one runs; their prep kernel waits on a control word in host-written device
  // memory, so when theta arrives the host only writes the pack and that word (no launch latency).
  struct ArmedEval {
    bool armed = false;
    bool keep = false;        // set while vbmc_neg_elcbo itself runs (its inner calls must not disarm)
    uint64_t seq = 0;         // completion sequence number the armed launches will publish
    uint64_t seed = 0;        // the Philox seed they were planned for
    int n_theta = 0, mask = 0, grad_flags = 0, eps_mode = 0;
    int64_t ns_per_comp = 0, row_begin = 0, row_count = 0;
    // state to restore when the armed launches are cancelled instead of run
    int gen_cur_before = 0;
    bool ahead_before_valid = false;
    uint64_t ahead_before_seed = 0;
    int ahead_before_buf = 0;
    double ahead_before_frac = 1.0;
    uint64_t hits = 0, cancels = 0, late = 0, ident_checked = 0, ident_bad = 0, lost = 0;  // see vbmc_armed_stats
    bool ident = false;       // its launches carry an identity (DoneSignal)
    double limit_ms = 1.0;  // use it within this time of arming (>= 1 ms, 2.5 x the last evaluation's duration); the device waits twice as long
    std::chrono::steady_clock::time_point t_armed;  // the device gives up after 2 ms: the host does not use an armed evaluation older than 1 ms
  } spec;
  uint64_t* d_ctl = nullptr;   // fine-grained device memory, 8 words: go / cancel word of evaluation seq is [seq & 7]
  double* d_stage = nullptr;   // device staging of the results the polled step hands to the host (DoneSignal)
  size_t d_stage_cap = 0;
  double* d_mix_fg = nullptr;  // host-writable (fine-grained) device memory: the host-driven step writes the pack here itself
  std::vector<double> mu_scratch;
  std::vector<double> t2m_mu, t2m_sg, t2m_lm, t2m_w, t2m_eta;  // vbmc_theta_to_mixture's working copies  // vbmc_set_mixture_dk's transposed means
  double* d_acq_fg = nullptr;  // the same kind of memory for a small acquisition batch's points (api_acq.hip); 256 x 33 doubles
  bool acq_fg_failed = false;
  uint64_t acq_seq = 0;        // sequence number of the acquisition completion word (h_done[7])
  size_t d_mix_fg_cap = 0;
  bool mix_fg_failed = false;
  size_t d_mix_cap = 0;

  // Philox draws generated ahead of the entropy kernel (fused objective): two buffers, so the
  // draws of evaluation i+1 can be generated behind evaluation i's finish kernel while the host
  // is busy with result i (api_elbo.hip); `ahead` says what the speculative buffer holds
  double* d_epsgen[2] = {nullptr, nullptr};
  size_t d_epsgen_cap[2] = {0, 0};
  int gen_cur = 0;  // buffer the current evaluation reads
  struct AheadDraws {
    bool valid = false;
    uint64_t seed = 0;
    int K = 0, D = 0, buf = 0;
    int64_t rows = 0, n_half = 0, row_begin = 0;
    double frac = 1.0;  // the part [0, frac) of the items is (being) generated; the consumer's prep launch adds the rest
  } ahead;
  // completion word of the fused objective: the finish kernel's last result wave stores the
  // evaluation's sequence number into pinned host memory and the host polls it -- the spare
  // workgroups of the same launch go on generating the next evaluation's draws meanwhile
  uint64_t* h_done = nullptr;   // pinned, device-visible
  uint64_t* hd_done = nullptr;  // its device-side address
  int* d_done_cnt = nullptr;    // result waves finished so far (reset by the last one)
  int* d_done_sub = nullptr;    // 16 sub-counters of the finish launch, 64 ints apart (DoneSignal::sub)
  uint64_t done_seq = 0;

  // resident antithetic half draws: [K][eps_rows][D]
  double* d_eps = nullptr;
  size_t d_eps_cap = 0;
  int eps_K = 0, eps_D = 0;
  int64_t eps_rows = 0, eps_row_begin = 0, eps_n_half = 0;

  // scratch (grown on demand)
  double* d_scratch = nullptr;
  size_t d_scratch_cap = 0;
  double* d_out = nullptr;  // small result vectors
  size_t d_out_cap = 0;
  double* d_ptick = nullptr;  // predict: one arrival ticket (int) per 64-point row tile and GP sample (gp.hip, the fused finish)
  size_t d_ptick_cap = 0;
  double* h_pinned = nullptr;  // pinned host staging for results (also written directly by kernels)
  double* h_eps = nullptr;     // pinned host buffer the reference-stream draws are generated into (vbmc_set_eps_numpy)
  size_t h_eps_cap = 0;
  size_t h_pinned_cap = 0;
  double* h_pack = nullptr;    // pinned source of the mixture pack upload
  size_t h_pack_cap = 0;
  bool pack_in_flight = false;   // a mixture-pack upload was queued and the stream not waited for since
  bool pack_valid = false;     // d_mix holds the pack of the host copies (mu, sigma, lambd, w)
  bool defer_mix_upload = false;  // set_mixture_host packs but leaves the copy to upload_packed_mixture
  double* hp_dev = nullptr;    // device-side address of h_pinned (cached: the query is an API call)
  int timing = 0;              // 1: record the HIP event pair around the dominant kernel (vbmc_set_timing); 2: also the pair INSIDE predict
  double host_us[5] = {0, 0, 0, 0, 0};  // see vbmc_last_host_us
  double step_marks[4] = {0, 0, 0, 0};  // see vbmc_last_step_marks
  int gp_where = 0;  // where the GP sums of the launches issued last run: 0 prep launch, 1 finish launch, 2 entropy launch
  // vbmc_set_option switches (defaults from the environment at context creation)
  int opt_entmc_valu = 0;   // 1: always the generic entropy kernel
  int opt_gp_ship = 1;      // host-driven step: the prep launch's GP sums are shipped to the host by a workgroup of the matrix-pipe entropy launch (EntArgs::ship_*)
  int opt_entmc_mfma = 1;   // the matrix-pipe form of the entropy kernel where its shape applies (entropy_mfma.hip)
  int opt_elbo_pregen = 1;  // Philox draws generated ahead of the entropy kernel
  int opt_elbo_ahead = 1;   // ... and those of seed+1 speculatively behind the finish kernel
  int opt_predict_dma = 1;  // predict's variance product through the LDS-direct kernel (batches on Cholesky samples)
  int opt_predict_fused = 1;  // ... with predict's finish in its epilogue: 0 never, 1 for one-round product grids, 2 always (gp.hip)
  int opt_arm_late_test = 0;  // test hook: n > 0 = the n-th use of an armed evaluation from now takes the late-go recovery path
  int opt_acq_poll = 1;       // small acquisition batches: points written by the CPU, results polled (api_acq.hip)
  int opt_is_mcmc_threads = 512;  // workgroup size of vbmc_is_mcmc's chains: 256, 512 or 768 (acq_is_mcmc.hip)
  int opt_gp_lml_chunk = 0;       // vbmc_gp_lml: n > 0 = candidates per chunk (test hook); 0 = the largest under the byte cap
  int opt_gp_hyp_rounds = 4;      // vbmc_gp_hyp_sample: rounds queued between two reads of the unfinished-chain count (test hook)
  int opt_gp_opt_rounds = 4;      // vbmc_gp_hyp_optimize: rounds queued between two reads of the unfinished-run count
  int opt_cmaes_rounds = 8;       // vbmc_search_cmaes: rounds queued between two reads of the count of runs not yet stopped
  void (*release_cb)(void*) = nullptr;  // vbmc_set_release_callback
  void* release_cb_user = nullptr;
  int opt_adam_fused = 1;     // the optimiser loop as one launch per batch where its shape applies (adam_fused.hip)
  int opt_adam_tail = 1;      // the optimiser loop at large sample counts as two launches per iteration (adam.hip adam_tail_kernel)
  int opt_ident_test = 0;     // test hook: n > 0 = the n-th identity check from now fails (the recovery path runs)
  bool ident_retry = false;   // inside the re-evaluation after a failed identity check
  int opt_elbo_arm = 1;     // queue the next host-driven evaluation's launches ahead of its theta (armed evaluation): 0 never, 1 while
                            // this context is the only one on its device in the process, 2 always
  bool counted = false;     // this context is in the per-device count of live contexts (ctx.hip)
  int opt_ws_span = 1;      // entropy kernel: span mode (entropy_args.h WsSpan: front / filler parts sized to end together); 0 = equal chunks
  int opt_ws_front = 0;     // span mode: the front workgroup's share of a CU's batches, per mille (0 = the built-in value)
  int opt_ws_pad = -1;      // span mode: padding slots behind every component (-1 = the built-in value)
  int opt_ws_roles = 1;     // wave-split kernel: rotated roles in a CU's filler workgroup, loops end at the components owned (EntArgs::roles); 0 = role = wave, all rows
  int opt_mix_bar = 1;      // host-driven step: pack written by the CPU into device memory (no upload launch), GP sums in the finish launch
  double* h_pack_dev = nullptr;     // device-side address of h_pack ...
  double* h_pack_dev_of = nullptr;  // ... valid for this h_pack
  // exp(eta) and its sum, shared by the three softmax Jacobians of an evaluation
  std::vector<double> exp_eta;
  double exp_eta_sum = 0.0;
  bool exp_eta_valid = false;
  int last_plan[4] = {-1, 0, 0, 0};  // see vbmc_last_entmc_plan
  size_t last_raw_off = 0;           // see vbmc_last_elbo_raw: offset into h_pinned, length (0: none)
  int last_raw_n = 0;

  GpState gp;
  GpState gp_next;             // vbmc_gp_posterior / vbmc_gp_append build here and swap it with `gp` when the build succeeded
  double* d_post_ws = nullptr;  // their workspace: inverted diagonal blocks, the append's vectors, the per-sample flags
  size_t d_post_ws_cap = 0;

  ncclComm* comm = nullptr;
  int rank = 0, world = 1;

  // host arrays the device GP came from, re-checksummed by vbmc_neg_elcbo while it waits (vbmc_set_gp_watch)
  std::vector<const double*> gp_watch_ptrs;
  std::vector<int64_t> gp_watch_lens;
  uint64_t gp_watch_ck = 0;

  ElboScratch elbo;      // api_elbo.hip
  void* adam = nullptr;  // device-resident optimiser state (adam.hip)
  void* acq_is = nullptr;  // resident importance-sampling state of AcqFcnVIQR / IMIQR (api_acq_is.hip)
  bool host_bound = false;    // vbmc_ctx_create narrowed the calling thread's affinity to the device's NUMA node (ctx.hip)
  int host_cpus = 0;          // CPUs in that thread's affinity set after context creation (0: not looked at)
  void* randn_dev = nullptr;  // buffers of the device-side NumPy stream (device_randn.hip)
  int randn_last_reused = 0;  // the last device pass found its window in the pass before (device_randn.hip)
  int opt_randn_dev = 1;      // vbmc_set_eps_numpy: the reference's stream generated on the device (0: on the host cores + PCIe)
  void* xf = nullptr;         // parameter-transformer descriptors, two slots (transform.hip)
  void* search = nullptr;     // the resident search set of the acquisition search (api_search.hip)
  void* sieve = nullptr;      // the resident candidate set of the sieve (api_sieve.hip)
  void* elcbo = nullptr;      // the full-ELCBO record of optimize_vp's last stage (api_elcbo_full.hip)
  uint64_t stream_waits = 0;  // stream_wait() calls so far (vbmc_elcbo_record_info reports them since the record)
  uint64_t gp_launches = 0;   // launches of the GP expected log joint queued so far: its sums (prep.hip), its variance (gp.hip)
};
// the device's CU count, which sizes one round of workgroups (256 where the runtime reports none)
inline int ctx_cus(const vbmc_ctx* ctx) { return ctx->prop.multiProcessorCount > 0 ? ctx->prop.multiProcessorCount : 256; }
int vbmc_live_contexts_on(int device);  // ctx.hip
void adam_free(vbmc_ctx* ctx);
void acq_is_free(vbmc_ctx* ctx);
void randn_dev_free(vbmc_ctx* ctx);
void xf_free(vbmc_ctx* ctx);  // transform.hip
void search_free(vbmc_ctx* ctx);  // api_search.hip
void sieve_free(vbmc_ctx* ctx);   // api_sieve.hip
void elcbo_free(vbmc_ctx* ctx);   // api_elcbo_full.hip
// device_randn.hip: the next n values of NumPy's legacy randn stream into d_out (device memory), state advanced as
// vbmc_mt19937_randn does; VBMC_W_NOT_FUSED = not this path's size (the caller uses the host generator)
int randn_device(vbmc_ctx* ctx, uint32_t* key, int* pos, int* has_gauss, double* gauss, double* d_out, int64_t n);

// error helpers -----------------------------------------------------------
int vbmc_fail(vbmc_ctx* ctx, int code, const char* fmt, ...);
extern thread_local std::string g_create_err;

#define HIP_TRY(ctx, call)                                                            \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return vbmc_fail((ctx), VBMC_E_HIP, "%s failed: %s (%s:%d)", #call,             \
                       hipGetErrorString(e_), __FILE__, __LINE__);                    \
  } while (0)

// The padded widths DP of the per-point kernels (density, sampler consumers, transformer): 2, 4, 6, 8, 10, 12, 16, 20,
// 24, 32.  CALL(DP) with the narrowest one that holds D (D <= 32 is the caller's check).
#define VBMC_DISPATCH_DP(D, CALL)   \
  do {                              \
    if ((D) <= 2) CALL(2);          \
    else if ((D) <= 4) CALL(4);     \
    else if ((D) <= 6) CALL(6);     \
    else if ((D) <= 8) CALL(8);     \
    else if ((D) <= 10) CALL(10);   \
    else if ((D) <= 12) CALL(12);   \
    else if ((D) <= 16) CALL(16);   \
    else if ((D) <= 20) CALL(20);   \
    else if ((D) <= 24) CALL(24);   \
    else CALL(32);                  \
  } while (0)

// Entry points that launch kernels refuse a host-only context (device_id -1).
// cancel an armed evaluation (api_elbo.hip): its queued kernels return at once, host state is restored
void spec_disarm(vbmc_ctx* ctx);
#define NEED_DEVICE(ctx)                                                                     \
  do {                                                                                       \
    if ((ctx)->device < 0)                                                                   \
      return vbmc_fail((ctx), VBMC_E_NODEV,                                                  \
                       "host-only context: this entry point needs a gfx950 device "          \
                       "(libvbmc_hip has no CPU fallback)");                                 \
    if ((ctx)->spec.armed && !(ctx)->spec.keep) spec_disarm(ctx);                            \
  } while (0)

void write_mixture_pack(const MixLayout& ml, const double* mu_KxD, const double* sigma,
                        const double* lambd, const double* w, double* p);
// a second mixture (kl_div's and mtv's vp2) from host arrays: sigma2 checked (failure code `err`, message prefix `who`),
// its layout planned and its pack written
int make_mixture2(vbmc_ctx* ctx, const char* who, int err, int D, int K2, const double* mu2_KxD, const double* sigma2_K,
                  const double* lambd2_D, const double* w2_K, MixLayout& ml2, std::vector<double>& pack2);
int theta_to_arrays(int D, int K, const double* theta, int n_theta, int optimize_mask, double* mu,
                    double* sg, double* lm, double* w, double* eta);
// [mu | sigma | lambda | w | eta] of the context's mixture (adam_dev::aux_len doubles) into dst / back from src
void ctx_pack_aux(const vbmc_ctx* ctx, double* dst);
void ctx_unpack_aux(vbmc_ctx* ctx, const double* src);
// this rank's slice of the ns_per_comp / 2 antithetic rows (opts->row_count < 0: the even split over the ranks), checked
// against the range and, for resident draws, against what the context holds; `who` prefixes the messages
int resolve_row_slice(vbmc_ctx* ctx, const vbmc_elbo_opts* opts, const char* who, int64_t* row_begin, int64_t* row_count);
int upload_packed_mixture(vbmc_ctx* ctx);
double* write_pack_to_device(vbmc_ctx* ctx);
int set_mixture_host(vbmc_ctx* ctx, int D, int K, const double* mu_KxD, const double* sigma_K,
                     const double* lambd_D, const double* w_K, const double* eta_K, bool skip_if_same);

// buffer helpers (ctx.hip) --------------------------------------------------
int ensure_dev(vbmc_ctx* ctx, double** p, size_t* cap, size_t n_doubles);
int ensure_pinned(vbmc_ctx* ctx, size_t n_doubles);
// the buffer behind a listed layout (scratch.h): grown to sc.total, sc.base set.  reserve: the context's scratch, the one
// place the entry points outside the step's path ensure it; reserve_in: another grown buffer (gp_post.hip's workspace)
int reserve_in(vbmc_ctx* ctx, double** p, size_t* cap, Scratch& sc);
int reserve(vbmc_ctx* ctx, Scratch& sc);
// n doubles of device memory to the host through the pinned buffer, in chunks
int download_chunked(vbmc_ctx* ctx, const double* d_src, double* dst, size_t n);
// A batch's result vectors: d_src[i] (count doubles each, i < k) to h_pinned + i * stride, one wait, then on to
// dst[i] + o; a null dst[i] is skipped.  dst == nullptr: they stay in h_pinned for the caller to read (pinned memory for
// k * stride doubles is the caller's: predict_reserve).
int fetch_vectors(vbmc_ctx* ctx, int k, const double* const* d_src, double* const* dst, size_t count, size_t stride, size_t o);
// csrc/host_randn.hip: vbmc_mt19937_randn with progress(user, m) = "out[0 .. m) is final", called from
// the calling thread while the worker threads still write the rest
int randn_with_progress(uint32_t* key, int* pos, int* has_gauss, double* gauss, double* out, int64_t n, int n_threads,
                        void (*progress)(void*, int64_t), void* user);

// raw-vector length of the entropy accumulator
static inline int raw_len(int D, int K) { return 1 + D * K + 2 * K + D; }

// arguments of the prep launch (prep.hip): table rows for the wave-split entropy kernel
// and/or the GP expected-log-joint sums
// A slice of the draw buffer eps[K][rows][D] for other kernels' spare workgroups to fill: the
// (row, block) items [item_begin, item_begin + item_count) of the K * rows * ceil(D/4) items -- one
// Philox block = up to four normals of a row (philox.h) -- 256 per workgroup.  The values
// depend on (seed, row, block) only, so any kernel may generate any slice.
// completion signalling of entmc_finish_kernel (all null/0: none)
struct DoneSignal {
  int* cnt = nullptr;        // device counter of finished result waves
  // optional, entmc_finish_kernel: sixteen sub-counters, 256 B apart.  One word takes ~88 atomic increments per us, and at
  // K = 100, D = 20 the reduction has 556 workgroups that arrive together: 6 us of the 14 between the entropy kernel and the
  // completion word.  From 256 workgroups on, workgroup b counts on sub-counter b % 16 and the last of each on `cnt`.
  int* sub = nullptr;
  int sub_min = 256;         // workgroups from which the sub-counters are used
  uint64_t* flag = nullptr;  // device-visible pinned word that receives `seq` when all are done
  uint64_t seq = 0;
  // Staged hand-over (optional): the kernel's result pointer is then DEVICE memory, and the last
  // workgroup to count copies host_n doubles from there to host_out (pinned) in coalesced stores
  // before it publishes.  One 8-byte store per result straight to pinned memory is one PCIe write
  // each -- ~1700 of them per evaluation queue up for 9-14 us in front of the completion word.
  double* host_out = nullptr;
  int host_n = 0;
  // armed evaluation: the finish kernel returns at once when *cancel == ~0 (ArmedEval)
  const uint64_t* cancel = nullptr;
  // Self-identifying results (optional): next to the sequence number the publishing workgroup hands
  // the host WHAT was evaluated -- ident_dst[0] = *ident_src, the checksum the prep launch's copy
  // block took of the mixture pack it actually read (pack_checksum below), ident_dst[1] = ident_seed,
  // the Philox seed these launches were planned for.  The host compares both with what it sent
  // before it accepts the result block (api_elbo.hip): a result computed on a stale pack or by the
  // launches of another evaluation cannot pass for this one's.
  const uint64_t* ident_src = nullptr;
  uint64_t* ident_dst = nullptr;
  uint64_t ident_seed = 0;
  // Device-side hand-over (optimiser loop, adam.hip): results AND flag are device memory and the reader is another
  // workgroup of the same launch -- write-through (agent-scope) stores, drained, then the flag at agent scope; no host copy
  int dev = 0;
};

// Order-independent 64-bit checksum of a block of doubles: sum_i bits(v_i) * (odd_i) mod 2^64.  Every
// multiplier is odd, hence invertible: any change of a single element changes the sum.  The same
// terms are added up by the host (over its pinned pack) and by the 256 threads of the prep launch's
// copy block (over the pack as the device reads it).
__host__ __device__ inline uint64_t pack_ck_term(double v, uint32_t i) {
  uint64_t b;
  __builtin_memcpy(&b, &v, 8);
  return b * (0x9E3779B97F4A7C15ull + 2ull * i);
}
inline uint64_t pack_checksum(const double* p, size_t n) {
  uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  size_t i = 0;
  for (; i + 4 <= n; i += 4) {
    s0 += pack_ck_term(p[i], (uint32_t)i);
    s1 += pack_ck_term(p[i + 1], (uint32_t)i + 1);
    s2 += pack_ck_term(p[i + 2], (uint32_t)i + 2);
    s3 += pack_ck_term(p[i + 3], (uint32_t)i + 3);
  }
  for (; i < n; ++i) s0 += pack_ck_term(p[i], (uint32_t)i);
  return (s0 + s1) + (s2 + s3);
}

#ifdef __HIPCC__
// The staged hand-over's copy (DoneSignal): n doubles from device memory written by other workgroups
// (write-through stores, already drained) to pinned host memory, by the 256 threads of one
// workgroup.  Eight loads are in flight per thread before the first store (a load -> store chain
// per element costs one memory latency each); sc1 loads read past this XCD's L2.
__device__ __forceinline__ void staged_copy_to_host(const double* __restrict__ src, double* __restrict__ dst, int n) {
  // (indices are clamped, not predicated: threads past the end repeat element n-1 -- the same value to
  // the same address -- so the loop body has no branch and the compiler keeps all eight loads, then
  // all eight write-through stores, in flight instead of draining the queue around every one)
  for (int base = 0; base < n; base += 256 * 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = min(base + u * 256 + (int)threadIdx.x, n - 1);
      v[u] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = min(base + u * 256 + (int)threadIdx.x, n - 1);
      __hip_atomic_store(dst + i, v[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): acknowledged
}
#endif

struct GenSlice {
  double* eps = nullptr;
  int K = 0, D = 0;
  int nb = 0;              // ceil(D / 4): Philox blocks per row
  uint32_t nb_magic = 0, rows_magic = 0;  // min(floor(2^32 / d), 2^32 - 1) for the two 32-bit divisions (philox.h gen_div32)
  int64_t rows = 0;        // rows per component held in eps (this rank's slice of the n_half pairs)
  int64_t n_half = 0, row_begin = 0;
  uint64_t seed = 0;
  const int* seed_add = nullptr;  // optional device-side addend (the Adam loop's iteration base)
  int64_t item_begin = 0, item_count = 0;
  int n_blocks = 0;        // ceil(item_count / 256)
};

struct PrepArgs {
  const double* mix = nullptr;
  MixLayout ml;
  // optional: one more workgroup copies mix[0 .. mix_copy_n) to mix_copy (the host-driven step
  // hands the pack over in host-written device memory; the later launches read the ordinary copy)
  double* mix_copy = nullptr;
  int mix_copy_n = 0;
  uint64_t* ident_out = nullptr;  // optional: that workgroup also stores pack_checksum(mix[0 .. mix_copy_n)) here (DoneSignal)
  // armed evaluation (ArmedEval): every workgroup first waits until *go == go_seq (the host has
  // written the pack) -- or leaves at once when it reads ~0 (cancelled); after ~2 ms without either
  // it cancels by itself (*go = ~0 for the launches behind it, *dead = go_seq for the host)
  uint64_t* go = nullptr;
  uint64_t go_seq = 0;
  uint64_t go_timeout = 200000;  // wall-clock ticks (100 MHz) the launch waits for the go word
  uint64_t* dead = nullptr;
  // table part (n_table = K blocks, or 0)
  int n_table = 0, DP = 0, K4 = 0;
  double* table = nullptr;
  // GP part (n_glj = S*K blocks, or 0)
  int n_glj = 0, N = 0, P = 0, want_grad = 0;
  int batch = 1;              // candidates (grid.y); candidate b uses mix + b*mix_stride, res + b*res_stride
  size_t mix_stride = 0, res_stride = 0;
  const double* X = nullptr;
  const double* XT = nullptr;  // [D][N]
  int x_lds = 0;               // glj_block.h: the launch's dynamic LDS holds X^T behind the block's own arrays (glj_block_lds_x): staged once per workgroup
  const double* alpha = nullptr;
  const double* hyp = nullptr;
  double* res = nullptr;  // [S][K][1+2D]  (device or device-visible pinned host memory)
  double* Z = nullptr;    // optional [S][K][N]
  // draw-generation part (gen.n_blocks workgroups, or 0): Philox/Box-Muller normals of the entropy
  // kernel -- throughput work that fills the GPU while the few table / GP blocks above sit in
  // their latency chains
  GenSlice gen;
  // optional completion word of the GP part (res must then be pinned host memory): the GP blocks
  // store their sums write-through, drain, and the last one to count publishes done.seq, so the
  // host can finalise G / dG while the entropy kernel runs
  DoneSignal done;
};
// the slice [frac_begin, frac_end) of the K * rows * ceil(D/4) draw items of eps[K][rows][D]
GenSlice make_gen_slice(double* eps, int K, int D, int64_t rows, int64_t n_half, int64_t row_begin,
                        uint64_t seed, const int* seed_add, double frac_begin, double frac_end);
// wait for everything queued on the ctx stream (also: the pinned mixture pack is free again)
inline hipError_t stream_wait(vbmc_ctx* ctx) {
  if (ctx->spec.armed) spec_disarm(ctx);  // (launches waiting for a theta would make this wait last their time-out)
  ++ctx->stream_waits;
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) ctx->pack_in_flight = false;
  return e;
}
// the event pair around a timed interval on ctx->stream, recorded while vbmc_set_timing is on
inline int timing_begin(vbmc_ctx* ctx, TimingPair p) {
  if (ctx->timing) HIP_TRY(ctx, hipEventRecord(ctx->ev[2 * p], ctx->stream));
  return 0;
}
inline int timing_end(vbmc_ctx* ctx, TimingPair p) {
  if (ctx->timing) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2 * p + 1], ctx->stream));
    ctx->ev_valid[p] = true;
  }
  return 0;
}
int launch_prep(vbmc_ctx* ctx, const PrepArgs& a);                           // on ctx->stream
int launch_prep_on(vbmc_ctx* ctx, hipStream_t stream, const PrepArgs& a);

// staged launch of the Monte-Carlo entropy (entropy.hip)
struct EntPlan;
// entmc_plan decides the geometry and which kernel runs (EntPlan::kernel).
// gp_items: GP expected-log-joint items the caller would like a span-mode launch to carry in spare workgroup slots (the
// plan says whether they fit: EntPlan::gp_in_ws; the optimiser loop's pre workgroup is the LAST block of a span-mode launch
// and finds one of the slots the plan leaves free)
// gp_per_slot > 0 (the optimiser loop): that many items per workgroup and one more free slot, for its pre workgroup
int entmc_plan(vbmc_ctx* ctx, int64_t ns_per_comp, int eps_mode, uint64_t seed, int64_t row_begin,
               int64_t row_count, int want_grad, EntPlan& p, int gp_items = 0, int gp_per_slot = 0);
// attach the GP sums `gp` (gp.n_glj items) to the plan's entropy launch when they fit its spare workgroup slots; returns
// whether they ride there (the plan is untouched when not)
bool entmc_take_gp(const vbmc_ctx* ctx, EntPlan& p, const PrepArgs& gp);
void entmc_fill_prep(const vbmc_ctx* ctx, const EntPlan& p, PrepArgs& a);
int entmc_pregen(vbmc_ctx* ctx, EntPlan& p, PrepArgs& a);

int entmc_launch_main(vbmc_ctx* ctx, const EntPlan& p);
// `gen`: optional slice of draws for spare workgroups of the finish launch to generate
int entmc_launch_finish(vbmc_ctx* ctx, const EntPlan& p, double* raw_out, const GenSlice* gen = nullptr,
                        const DoneSignal* done = nullptr);
// multi-GPU step: hand the all-reduced raw vector (device memory) to the host and publish done.seq;
// spare workgroups generate `gen` (entropy.hip)
int entmc_launch_publish(vbmc_ctx* ctx, const double* d_raw, const DoneSignal& done, const GenSlice* gen);
// the slice of seed+1's draws the finish launch's spare workgroups should generate (n_blocks == 0: none)
GenSlice entmc_ahead_slice(vbmc_ctx* ctx, const EntPlan& p);
void glj_fill_prep(const vbmc_ctx* ctx, int want_grad, double* res, double* Z, PrepArgs& a);

// kernels' host launchers (one per .hip file) -------------------------------
// entropy
int launch_entmc(vbmc_ctx* ctx, int64_t ns_per_comp, int eps_mode, uint64_t seed,
                 int64_t row_begin, int64_t row_count, int want_grad, double* d_raw);
int launch_entlb(vbmc_ctx* ctx, double* d_res);  // writes raw entlb terms
// the in-line Philox/Box-Muller draws of the entropy kernel, written to eps[K][rows][D] by a
// kernel of their own on `st` (same values: counter = global row, pair; key = seed [+ *seed_add,
// a device-side int, when given])
int launch_eps_gen(vbmc_ctx* ctx, hipStream_t st, const GenSlice& g);
// mixture pdf
int launch_mixture_pdf(vbmc_ctx* ctx, int64_t n, const double* d_x, int log_flag,
                       int grad_flag, double df, double* d_y, double* d_dy);
int launch_mixture_pdf_on(vbmc_ctx* ctx, const double* d_pack, const MixLayout& ml, int64_t n,
                          const double* d_x, int log_flag, double* d_y);
// sampling (sample.hip): counts / cdf of a mixture's component selection; without balance n_exact = 0 and cdf is
// np.random.choice(p=w)'s cumulative sum
struct Selector {
  int64_t n_exact = 0;
  std::vector<int64_t> cum;  // K+1
  std::vector<double> cdf;   // K
};
void make_selector(const double* w, int K, int64_t N, int balance, Selector& s);
// The selection vectors in device scratch, a piece of selector_elems(K) doubles: (K+1) int64 counts | K doubles of cdf
// (mode.hip draws from the cdf alone and carves selector_cdf_elems(K))
inline size_t selector_cdf_elems(int K) { return (size_t)K; }
inline size_t selector_elems(int K) { return (size_t)K + 1 + selector_cdf_elems(K); }
inline int64_t* selector_cum(double* d_sel) { return (int64_t*)d_sel; }
inline double* selector_cdf(double* d_sel, int K) { return d_sel + K + 1; }
// N draws of the mixture `d_pack` (selection vectors through d_sel, a piece of selector_elems(K) doubles)
int launch_sample(vbmc_ctx* ctx, const double* d_pack, const MixLayout& ml, const double* w_host, int64_t N,
                  uint64_t seed, int balance, double* d_sel, double* d_x, int32_t* d_comp, double df = INFINITY);
// per-block partial sums of log q_other - log q_own with kl_div's zero-replacement rules (nblk blocks)
int launch_kl_terms(vbmc_ctx* ctx, const double* d_y_own, const double* d_y_other, int64_t n, int nblk, double* d_part);
// gp
int launch_gp_log_joint(vbmc_ctx* ctx, int want_grad, double* d_res, double* d_Z);
int launch_gp_var(vbmc_ctx* ctx, const double* d_Z, double* d_V, double* d_Q);
// d_Dinv: the inverted 64 x 64 diagonal blocks [S][nb] when the caller has them already (gp_post.hip's factorisation
// forms them); the first stage is then skipped
int launch_trinv(vbmc_ctx* ctx, const double* d_Dinv = nullptr);
int launch_pad_linv(vbmc_ctx* ctx);
// gp_post.hip: the posterior of ctx->gp's X, y, hyp, noise built in ctx->gp's buffers (covariance, blocked upper
// Cholesky, L^-1, alpha); d_flag[s] != 0 afterwards: sample s met a pivot that is not a positive finite number
int launch_gp_post_build(vbmc_ctx* ctx, double* d_Dinv, int* d_flag);
// the workspace of an append to S samples of N points, listed once: flags | kvec, lvec, uvec [S][N] | dd 3 S | rnew S |
// tvec [S][N + 1]
struct GpAppendWs {
  Scratch sc;
  Piece<int> flag;
  Piece<> kvec, lvec, uvec, dd, rnew, tvec;
};
GpAppendWs gp_post_append_ws(int S, int N);
// one point appended: `from` (N points, live) -> ctx->gp (N + 1 points, X / XT / hyp / sl / sn2 already in place);
// ws: gp_post_append_ws(from.S, from.N), reserved.  d_sn2_new[s * sn2_stride]: the new point's noise variance in sample s
int launch_gp_post_append(vbmc_ctx* ctx, const GpState& from, double y_new, const double* d_sn2_new, size_t sn2_stride,
                          const GpAppendWs& ws);
void gp_post_free(vbmc_ctx* ctx);
// api_gp_post.hip: the host-side fields of a device-built state w that follow from w.h_X, w.h_sl and the shapes (L_chol,
// sn2_eff, sn2_mult, h_small = predict centre | smeta, h_XT) and sW as uploaded
void gp_post_host_fields(GpState& w, int N, int D, int S, int P, int mean_kind, std::vector<double>& sW_host);
// gp_fit.hip: the hand-over kernels of vbmc_gp_fit (gp_fit_host.h has their arguments).  design: the B candidate rows;
// stage: candidates [b0, b0 + S) into the staged GP's slots; rank: scores from ws.lml and the prior, the order, the
// optimiser's starts; select: the optimum and the chains' starts; handover: the S samples into the staged GP.
int launch_gp_fit_design(vbmc_ctx* ctx, const GpFitArgs& f);
int launch_gp_fit_stage(vbmc_ctx* ctx, const GpFitArgs& f, int b0, int S);
int launch_gp_fit_rank(vbmc_ctx* ctx, const GpFitArgs& f);
int launch_gp_fit_select(vbmc_ctx* ctx, const GpFitArgs& f);
int launch_gp_fit_handover(vbmc_ctx* ctx, const GpFitArgs& f);
// gp_lml.hip: value and gradient of the log marginal likelihood of ctx->gp's S candidates from the factor state
// launch_gp_post_build left there.  d_sums [S][2], d_part [S][gp_lml_part_elems], d_mg [S][mean parameters]: workspace;
// d_lml [S], d_dlml [S][P] (want_grad): results, device memory
int launch_gp_lml(vbmc_ctx* ctx, int want_grad, const double* d_dsn2, double* d_sums, double* d_part, double* d_mg,
                  double* d_lml, double* d_dlml);
// api_gp_lml.hip: the launching side of gp_cand_host.h, shared by vbmc_gp_lml and the lockstep entries.
// gp_stage_data: the fields of the staged state w and the uploads that do not change from chunk to chunk (X, X^T, y).
int gp_stage_data(vbmc_ctx* ctx, GpState& w, int N, int D, int P, int mean_kind, const double* X, const double* y);
// gp_cand_begin: the device, the stream drained, ctx->gp_next grown for `chunk` candidates
int gp_cand_begin(vbmc_ctx* ctx, int N, int D, int P, int chunk);
// gp_lml_chunk: S candidates, staged in ctx->gp_next, through the factorisation and the value (and gradient) kernels;
// their flags, lml and dlml go to slots [slot0, slot0 + S) of ws.  ctx->gp_next is swapped in as ctx->gp for the launches
// and swapped back on every path.
int gp_lml_chunk(vbmc_ctx* ctx, const Scratch& sc, const GpLmlWs& ws, int S, int slot0);
// gp_cand_stage: a lockstep entry's uploads, once per call -- X, X^T, y and the packed `in` block to d_in -- ws's cleared
// range and the entry's own pieces [own_off, sc.total) zeroed (count, a zeroed state = every run at its start, zeros
// where an invalid run writes nothing), and a's lml, flag and g_* wired.  A failure has waited for the stream.
int gp_cand_stage(vbmc_ctx* ctx, const char* who, const Scratch& sc, const GpLmlWs& ws, double* d_in,
                  const std::vector<double>& in, size_t own_off, int mean_kind, const double* X, const double* y, GpCandArgs& a);
// One round of a lockstep entry: per chunk of the runs, advance(b0, S) -> rc moves the runs [b0, b0 + S) on by one
// evaluation and leaves their candidates in the staged GP, then gp_lml_chunk evaluates them.
template <class Advance>
int gp_cand_round(vbmc_ctx* ctx, const Scratch& sc, const GpLmlWs& ws, int runs, int chunk, Advance advance) {
  int rc = 0;
  for (int b0 = 0; b0 < runs && !rc; b0 += chunk) {
    const int S = runs - b0 < chunk ? runs - b0 : chunk;
    if (!(rc = advance(b0, S))) rc = gp_lml_chunk(ctx, sc, ws, S, b0);
  }
  return rc;
}
// lockstep.hip.  Where a run's "finished" word sits: each state's owner states it next to its state's size.
struct LockstepWord {
  size_t state_elems = 0, offset_bytes = 0;  // doubles of one run's state; the 32-bit word's offset in it
  int done_value = 0;
};
// *d_count = the runs of [0, n_runs) whose word is not done_value
int launch_lockstep_count(vbmc_ctx* ctx, const double* d_state, int n_runs, size_t state_elems, size_t word_offset_bytes,
                          int done_value, int* d_count);
// The rounds of a lockstep entry (DESIGN.md "lockstep drivers"): round_fn(rounds) -> rc queues one round; after per_batch
// of them (never past max_rounds) the count is launched, ONE int comes back through ctx->h_pinned and the host goes on
// while it is not zero.  Returns the first rc; the failure epilogue and the "unfinished" message are the caller's.
template <class RoundFn>
int lockstep_rounds(vbmc_ctx* ctx, const char* what, int per_batch, long long max_rounds, int n_runs, const double* d_state,
                    const LockstepWord& word, int* d_count, RoundFn round_fn, long long* rounds, int* left) {
  int rc = 0;
  *rounds = 0;
  *left = n_runs;
  while (*left > 0 && *rounds < max_rounds) {
    for (int q = 0; q < per_batch && *rounds < max_rounds; ++q, ++*rounds)
      if ((rc = round_fn(*rounds))) return rc;
    if ((rc = launch_lockstep_count(ctx, d_state, n_runs, word.state_elems, word.offset_bytes, word.done_value, d_count)))
      return rc;
    hipError_t e = hipMemcpyAsync(ctx->h_pinned, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = stream_wait(ctx);
    if (e != hipSuccess) return vbmc_fail(ctx, VBMC_E_HIP, "%s: %s", what, hipGetErrorString(e));
    *left = *(const int*)ctx->h_pinned;
  }
  return 0;
}
// A call's results in one copy: the tail [from, sc.total) of its scratch to ctx->h_pinned (the caller's ensure_pinned; the
// pinned copy keeps the pieces' spacing), one wait, then each piece to its host array; a null dst is skipped.
struct FetchPiece {
  size_t off;  // the piece's offset in the scratch, doubles
  void* dst;
  size_t bytes;
};
int fetch_tail(vbmc_ctx* ctx, const Scratch& sc, size_t from, std::initializer_list<FetchPiece> pieces);
// gp_hyp.hip: the lockstep slice chains of vbmc_gp_hyp_sample over lml + log prior.  One advance launch moves the chains
// [b0, b0 + S) of a chunk on by one evaluation: chain c consumes lml[c] / flag[c] of the round before and writes its next
// candidate into slot c - b0 of the buffers launch_gp_post_build reads.  All pointers device memory.
struct GpHypArgs : GpCandArgs {
  int C = 0, n = 0, thin = 0, burn_in = 0;
  uint64_t seed = 0;
  const double* widths = nullptr;      // [P]
  double *x = nullptr, *xp = nullptr;  // [C][P] the chain's point; the point under evaluation
  double *hyp_out = nullptr, *logpost = nullptr, *logprior = nullptr;  // [C][n][P], [C][n], [C][n]
};
size_t gp_hyp_state_elems();  // doubles of one chain's state
LockstepWord gp_hyp_done_word();
int launch_gp_hyp_advance(vbmc_ctx* ctx, const GpHypArgs& a, int b0, int S);
// gp_opt.hip: the lockstep quasi-Newton runs of vbmc_gp_hyp_optimize over phi = -(lml + log prior).  One advance launch
// moves the runs [b0, b0 + S) of a chunk on by one evaluation: run r consumes lml[r] / dlml[r][:] / flag[r] of the round
// before and writes its next trial point into slot r - b0 of the buffers launch_gp_post_build reads, and that slot's
// d sn2 / d log sn into dsn2[r - b0].  All pointers device memory.
struct GpOptArgs : GpCandArgs {
  int R = 0, max_iter = 0, m = 0, trace_cap = 0;
  double tol_g = 0.0, tol_f = 0.0;
  const double* dlml = nullptr;  // [R][P]: the round before's gradient
  double* dsn2 = nullptr;        // [chunk]
  double *hyp_out = nullptr, *logpost = nullptr, *grad = nullptr;  // [R][P], [R], [R][P]
  // stats [R][4]: iterations, evaluations, history resets, stop reason
  double *trace_it = nullptr, *trace_ev = nullptr;  // [R][trace_cap][3 P + 3], [R][1 + 31 trace_cap][4] (trace_cap > 0)
};
size_t gp_opt_state_elems(int P, int m);
LockstepWord gp_opt_done_word(int P, int m);
int launch_gp_opt_advance(vbmc_ctx* ctx, const GpOptArgs& a, int b0, int S);
// api_gp.hip: the device buffers of a GP state of N points, D dimensions, S samples, P hyper-parameters, kept across GP
// updates and only grown (capacity n + n / 8 + 64: active sampling makes N creep up by one); with_post: also what a
// device-built posterior keeps (y, residuals, noise variances, sl)
int gp_state_grow(vbmc_ctx* ctx, GpState& g, int N, int D, int S, int P, bool with_post);
// leading dimension of the padded operands of predict's variance product, and the size of the
// K* scratch of a batch of mb points (rows rounded up to whole 64-row tiles)
inline int predict_ld(int N) { return (N + 63) / 64 * 64; }
inline size_t predict_ks_elems(int S, int64_t mb, int N) {
  return (size_t)S * (size_t)((mb + 63) / 64 * 64) * (size_t)predict_ld(N);
}
// The batch plan of an entry point that runs predict on M points: mb points per batch -- budget / cost doubles,
// in whole 64-row tiles, at most cap and at most M -- and the scratch of one batch listed as
//   xs (mb x D) | Ks [S] (256-byte aligned: read by 16-byte LDS-direct loads) | part, fpart [S][ntiles][mb] |
//   fmu [S][mb] | fs2 [S][mb].
// The caller adds its own pieces to p.sc behind these, then predict_reserve ensures the device scratch and
// pinned_per_point x mb doubles of pinned memory and forms the pointers.
struct PredictPlan {
  int64_t mb = 0;
  int ntiles = 0;
  Scratch sc;
  Piece<> p_xs, p_Ks, p_part, p_fmu, p_fs2;
  double *xs = nullptr, *Ks = nullptr, *part = nullptr, *fmu = nullptr, *fs2 = nullptr;
};
inline void predict_plan(const vbmc_ctx* ctx, int64_t M, int64_t budget, int64_t cost, int64_t cap, PredictPlan& p) {
  const int S = ctx->gp.S, N = ctx->gp.N, D = ctx->gp.D;
  p.ntiles = (N + 63) / 64;
  int64_t mb = budget / cost;
  mb = mb > cap ? cap : (mb < 64 ? 64 : (mb / 64) * 64);
  p.mb = mb = M < mb ? M : mb;
  p.p_xs = p.sc.add((size_t)mb * D);
  p.p_Ks = p.sc.add(predict_ks_elems(S, mb, N), 32);
  p.p_part = p.sc.add(2 * (size_t)S * p.ntiles * mb);
  p.p_fmu = p.sc.add((size_t)S * mb);
  p.p_fs2 = p.sc.add((size_t)S * mb);
}
inline int predict_reserve(vbmc_ctx* ctx, PredictPlan& p, size_t pinned_per_point) {
  int rc = reserve(ctx, p.sc);
  if (rc) return rc;
  rc = ensure_pinned(ctx, pinned_per_point * (size_t)p.mb);
  if (rc) return rc;
  p.xs = p.sc.ptr(p.p_xs);
  p.Ks = p.sc.ptr(p.p_Ks);
  p.part = p.sc.ptr(p.p_part);
  p.fmu = p.sc.ptr(p.p_fmu);
  p.fs2 = p.sc.ptr(p.p_fs2);
  return 0;
}
int launch_gp_predict_products(vbmc_ctx* ctx, int64_t M, const double* d_xs, double* d_Ks, double* d_part,
                               const void* fin = nullptr, bool* fin_done = nullptr);
// C (M x NC) = A (M x KD) B (KD x NC), row-major: the panel-product kernel of predict, store only; upper_b: B is upper
// triangular (KD = NC) and the panels below the diagonal of a column tile are skipped
int launch_gp_panel_product(vbmc_ctx* ctx, const double* d_A, const double* d_B, double* d_C, int64_t M, int KD, int NC,
                            bool upper_b = false);
int launch_gp_predict_all(vbmc_ctx* ctx, int64_t M, const double* d_xs, double* d_Ks, double* d_part,
                          int add_noise, double* d_fmu, double* d_fs2, int64_t ld);
// One batch of m device points (d_xs, reserved plan p) through the acquisition, no copy in or out: what vbmc_acq_eval
// and vbmc_acq_is_eval run per batch, and vbmc_search_eval on the resident search set.
// api_acq.hip, the closed forms: d_dens (mb) workspace, d_sn2 (m; VBMC_ACQ_NOISY only), d_res = acq | f_bar | var_tot, mb apart
int launch_acq_closed(vbmc_ctx* ctx, const PredictPlan& p, int64_t m, const double* d_xs, const double* d_sn2, int kind,
                      double y_max, double tol_gp_var, double* d_dens, double* d_res);
// api_acq_is.hip, the importance-sampled kinds: the resident importance state checked against the context's GP (`who`
// prefixes the message), its number of importance points, and the batch -- d_Kx (mb x N), d_T (mb x Na), d_as [S][mb]
// workspace, d_res = acq | var_tot, mb apart
int acq_is_need(vbmc_ctx* ctx, const char* who, int64_t* Na);
int launch_acq_is(vbmc_ctx* ctx, const PredictPlan& p, int64_t m, const double* d_xs, const double* d_sn2, double u,
                  double* d_Kx, double* d_T, double* d_as, double* d_res);
// search.hip: the kernels of the acquisition search (api_search.hip), all on ctx->stream
struct XfView;
struct SearchSrcDev {  // one source of the fill table as the generator kernel reads it
  int kind, pad;
  long long begin, count;  // rows [begin, begin + count) of the set
  unsigned long long seed;
  long long par;           // offset of its parameters in the table's block of doubles
};
// rows of the affine-Gaussian and box-normal sources drawn, every row clamped to [d_lb, d_ub] (null: no clamp) and its
// integer columns (bit d of int_bits) rounded in original space (t null: the identity transformer)
int launch_search_fill(vbmc_ctx* ctx, double* d_X, int64_t M, int D, const SearchSrcDev* d_src, int n_src, const double* d_par,
                       const double* d_lb, const double* d_ub, uint32_t int_bits, const XfView* t);
// acq[m] = +inf where the point (inverse-transformed, t null: as it is) lies outside [d_lb, d_ub]
int launch_search_mask(vbmc_ctx* ctx, const double* d_X, int64_t M, int D, const XfView* t, const double* d_lb,
                       const double* d_ub, double* d_acq);
// the noise lookup's operands: d_xsc = X / ell per column; the column sums of a set in d_part (search_sum_blocks x D
// doubles) and the centre of AbstractAcqFcn._sq_dist from the two sets' sums
constexpr int search_sum_blocks = 64;
int launch_search_scale(vbmc_ctx* ctx, const double* d_X, int64_t M, int D, const double* d_ell, double* d_xsc);
int launch_search_colsum(vbmc_ctx* ctx, const double* d_x, int64_t n, int D, double* d_part);
int launch_search_centre(vbmc_ctx* ctx, const double* d_part_a, int64_t n, const double* d_part_b, int64_t m, int D,
                         double* d_cen);
int launch_search_take(vbmc_ctx* ctx, const double* d_table, int64_t n_table, const int64_t* d_pos, int64_t M, double* d_out);
// the importance kinds' tail (abstract_acq_fcn.py:110-131): variance regularisation of a log-valued acquisition, clamp
int launch_search_is_finish(vbmc_ctx* ctx, int64_t M, double tol_gp_var, const double* d_var_tot, double* d_acq);
// stable ascending order of acq[0 .. M) (NaN last): d_keys / d_idx hold search_sort_len(M) pairs; d_order[M] (int64) and
// d_Xs (M x D, the rows of d_X in that order) are written
int64_t search_sort_len(int64_t M);
int launch_search_sort(vbmc_ctx* ctx, const double* d_acq, int64_t M, uint64_t* d_keys, uint32_t* d_idx);
int launch_search_gather(vbmc_ctx* ctx, const double* d_X, const uint32_t* d_idx, int64_t M, int D, int64_t* d_order,
                         double* d_Xs);
// api_search.hip: scoring a block of device rows with the acquisition -- the noise lookup, launch_acq_closed / launch_acq_is
// with launch_search_is_finish, launch_search_mask -- for vbmc_search_eval (the resident set) and vbmc_search_cmaes (a
// generation's candidates).  A call's order: check (the arguments, before anything is launched), list (the pieces of
// at most M rows into s.p.sc, the caller's own pieces behind them), predict_reserve(ctx, s.p, 0), upload (the hard
// bounds and the noise table, once), rows (per set: scale, column sums, centre, sq_dist argmin, take, the acquisition in
// batches, the mask; d_acq[0 .. m) written).
struct SearchScore {
  int kind = 0, use_xf = 0;
  bool is_kind = false, noisy = false;
  int64_t Na = 0, n_noise = 0, M = 0;
  XfView t;
  const double *X_rescaled = nullptr, *sn2_new = nullptr, *length_scale = nullptr, *lb_eps = nullptr, *ub_eps = nullptr;
  std::vector<double> bnd;  // host source of the hard bounds' upload
  PredictPlan p;
  Piece<> p_dens, p_Kx, p_T, p_as, p_res, p_sn2, p_bnd, p_ell, p_xsc, p_b, p_tab, p_cen, p_part, p_pmin;
  Piece<int64_t> p_am;
};
int search_score_check(vbmc_ctx* ctx, const char* who, int kind, int64_t n_noise, const double* X_rescaled_NxD,
                       const double* sn2_new_N, const double* length_scale_D, int use_xf, const double* lb_eps_orig_D,
                       const double* ub_eps_orig_D, SearchScore& s);
int search_score_list(vbmc_ctx* ctx, const char* who, int64_t M, SearchScore& s);
int search_score_upload(vbmc_ctx* ctx, SearchScore& s);
int search_score_rows(vbmc_ctx* ctx, const SearchScore& s, const double* d_X, int64_t m, double y_max, double tol_gp_var,
                      double u, double* d_acq);
int search_set_rows_cap();                       // the search set's row cap (2^20)
int search_fail_wait(vbmc_ctx* ctx, int rc);     // a failed call waits for the copies it queued from its own host memory
// api_batch.hip: the sieve's scoring launches (pack, GP sums, lower-bound entropy, finalisation) on B thetas that are in
// device memory already, for vbmc_neg_elcbo_batch (its uploaded rows) and vbmc_sieve_eval (the resident set).  A call's
// order: check (before anything is queued), list (the pieces into sc, behind the caller's own), the caller's reserve and
// ensure_pinned (batch_score_pinned doubles at hp), queue.  F | G | H are then the piece p_out, the flags p_flags
// ([0] the pack's non-finite status, [1] the first non-finite candidate or 0x7fffffff); s must outlive the stream wait.
struct BatchScore {
  int B = 0, n_theta = 0, n_bnd = 0, n_aux = 0, mask = 0;
  size_t stride = 0;
  MixLayout ml;
  Piece<> p_aux, p_packs, p_res, p_H, p_out, p_base, p_bnd;
  Piece<int> p_flags;
  int flags0[2] = {0, 0};  // host source of the flags' upload
};
int batch_score_check(vbmc_ctx* ctx, const char* who, int B, int n_theta, const vbmc_elbo_opts* opts);
void batch_score_list(const vbmc_ctx* ctx, int B, int n_theta, const vbmc_elbo_opts* opts, Scratch& sc, BatchScore& s);
size_t batch_score_pinned(const BatchScore& s);
int batch_score_queue(vbmc_ctx* ctx, const char* who, const Scratch& sc, BatchScore& s, const vbmc_elbo_opts* opts, double* d_th,
                      double* hp);
// sieve.hip: the candidate generator of the sieve (api_sieve.hip), one workgroup per candidate, on ctx->stream.  All
// pointers device memory; a null Z = the draws come from Philox under `seed` (streams 10, 11, 12: csrc/sieve.hip).
struct SieveFillDev {
  int D = 0, K = 0, Kn = 0, mask = 0, n_theta = 0, Ns = 0, n_slot = 0;
  long long n1 = 0, n2 = 0, n3 = 0;
  unsigned long long seed = 0;
  const double* base = nullptr;   // mu0 [K][D] | sigma0 [K] | lambd0 [D] | w0 [K]
  const double* t2 = nullptr;     // type 2's start: mu [Kn][D] | sigma [Kn]
  const double* lam_s = nullptr;  // [D]: types 2 and 3 with optimised lambd
  const double* Xs = nullptr;     // [Ns][D]
  double v3 = 0.0;                // type 3 with K == 1: mean_d var(X_star[:, d], ddof = 1)
  const double* Z = nullptr;      // [B][n_slot]
  const int* I = nullptr;         // [B][Kn]
  double* thetas = nullptr;       // [B][n_theta]
};
// dynamic LDS of a workgroup; n_keys: N_star where type 3's selection is ranked on the device (Philox draws), else 0
size_t sieve_fill_lds_bytes(int D, int Kn, int n_keys);
int launch_sieve_fill(vbmc_ctx* ctx, const SieveFillDev& a);
// F, G, H [b] = NaN where row b of thetas holds a value that is not finite
int launch_sieve_nan_rows(vbmc_ctx* ctx, const double* d_thetas, int64_t B, int n_theta, double* d_F, double* d_G, double* d_H);
// elcbo_full.hip: the kernels of optimize_vp's last stage (api_elcbo_full.hip), on ctx->stream; all pointers device memory.
// I_sk [S][K] from the GP sums d_res [S][K][1 + 2 D] of launch_gp_log_joint (api_gp.hip glj_finalize's I_k: the sum, the
// mean function's constant and quadratic parts) for the context's mixture and GP
int launch_elcbo_isk(vbmc_ctx* ctx, const double* d_res, double* d_I);
// The re-weighting: G_s and varG_s over the alive columns alive[0 .. Ka) of I [S][K0] and J [S][K0][K0] (null: no
// variance) with the weights w[0 .. Ka) into part [2][S], then out = G, varG, var_ss over s (api_gp.hip:246-288)
int launch_elcbo_reweight(vbmc_ctx* ctx, int S, int K0, int Ka, const double* d_I, const double* d_J, const double* d_w,
                          const int* d_alive, double* d_part, double* d_out);
// cmaes.hip: the lockstep CMA-ES runs of vbmc_search_cmaes.  One advance launch moves every run on by one generation:
// run r consumes val[r lam .. r lam + lam) (round 1: val[r], the start's value) and writes its next lam candidates,
// rounded, into rows[r lam ..] (round 0: the start into rows[r]).  All pointers device memory; the constants are the
// host's float64 values (api_cmaes.hip).
struct CmaesArgs {
  int R = 0, D = 0, lam = 0, mu = 0, hist = 0;
  long long max_fevals = 0;
  uint64_t seed = 0;
  double tol_fun = 0.0, tol_x = 0.0;  // tol_x <= 0: 1e-11 sigma0 of the run
  // 1 - c_sigma, sqrt(c_sigma (2 - c_sigma) mu_eff), (1 - c_sigma)^2, (1.4 + 2 / (D + 1)) chi_D, 1 - c_c,
  // sqrt(c_c (2 - c_c) mu_eff), 1 - c_1 - c_mu, c_1, c_mu, c_c (2 - c_c), c_sigma / d_sigma, 1 / chi_D
  double one_cs = 0, a_ps = 0, q_cs = 0, hs_thresh = 0, one_cc = 0, a_pc = 0, c_old = 0, c1 = 0, cmu = 0, cc2 = 0, cs_ds = 0, inv_chi = 0;
  const double* w = nullptr;  // [mu]
  const double *x0 = nullptr, *sigma0 = nullptr, *lb = nullptr, *ub = nullptr;  // [R][D], [R], [D], [D]
  uint32_t int_bits = 0;
  int has_xf = 0;
  XfView t;
  const double* val = nullptr;  // [R lam]
  double* rows = nullptr;       // [R lam][D]
  double* state = nullptr;      // [R][CmaState(D, lam, hist).total], zeroed by the caller: a zeroed state is a run at its start
  double *x_best = nullptr, *f_best = nullptr, *f0 = nullptr, *mean = nullptr, *sigma = nullptr, *C = nullptr;
  long long* stats = nullptr;   // [R][4]: generations, evaluations, stop reason, generation of the best
};
int launch_cmaes_advance(vbmc_ctx* ctx, const CmaesArgs& a);
LockstepWord cmaes_done_word(const CmaState& ly);  // a run has stopped
// acq_is_mcmc.hip: the S slice-sampling chains of active_importance_sampling's step 2, one workgroup each, on ctx->stream
// (all pointers device memory; d_invalid [S] zeroed by the caller), and the dynamic LDS a workgroup of `threads` needs
size_t is_mcmc_lds_bytes(int N, int threads);
int launch_is_mcmc(vbmc_ctx* ctx, int ln_y_fmu, double u_q, const double* d_x0, const double* d_widths, const double* d_lb,
                   const double* d_ub, int n, int thin, int burn_in, uint64_t seed, double* d_X, double* d_logp,
                   double* d_fmu, double* d_fs2, long long* d_stats, int* d_invalid);
// c[n][m] = |a_n - b_m|^2 (centred expansion, cross term on the FP64 matrix cores), optional
// row-wise argmin; d_cen[D] = the centre subtracted from both sets
int launch_sq_dist(vbmc_ctx* ctx, const double* d_a, int64_t n, const double* d_b, int m, int D,
                   const double* d_cen, double* d_c, double* d_pmin, int64_t* d_argmin);

// host finalisation of the GP expected log joint (api_gp.hip)
void glj_finalize(const vbmc_ctx* ctx, const double* res, int want_grad, GljHost& o);
// packs dG for one sample (or the average) into out; returns its length
int glj_pack(vbmc_ctx* ctx, const double* mu, const double* sg, const double* lm,
             const double* wg, int grad_flags, int jacobian_flag, double* out);
// comm
bool ctx_is_multi(const vbmc_ctx* ctx);  // the entropy sums go through the all-reduce
int comm_allreduce_sum(vbmc_ctx* ctx, double* d_buf, int n);

// host finalisation (api_entropy.hip) -------------------------------------
void softmax_jacobian_apply(vbmc_ctx* ctx, const double* g, double* out);  // J_w(ctx->eta) @ g
int entropy_pack(vbmc_ctx* ctx, double H, const double* mu, const double* sg,
                 const double* lm, const double* wg, int grad_flags, int jacobian_flag,
                 double* H_out, double* dH_out);
