// vb_internal.hpp — host-side launch interface between the C ABI layer
// (vb_capi.hip) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vb_gemm.hpp"

namespace vbk {

constexpr int kBlockDMax = 16;  // largest D handled by the block-per-problem kernel

// The variational family of a call: kind (0 = mf gaussian, 1 = mf t, kFamilyFrT) and
// the constants that follow from df (check_family in vb_capi.hip).
struct Family {
  int kind, D;
  double df;
  double t_scale, shape;  // mf t: sqrt(df/2), df/2
  double t_const;         // log normaliser of the t density (per coordinate / multivariate)
  int R = 0;              // low-rank Gaussian (kFamilyLrGaussian): columns of B
};

// Where a launch takes its standardized draws from: host-generated draws already in
// device memory (eps), or Philox counters.  Launch functions unpack it into the
// kernels' own arguments (Rng, step).
struct Noise {
  const double* eps;  // null: Philox
  uint32_t k0, k1, stream;
  uint32_t stride;    // problem q draws from stream + q * stride
  long long step;     // step counter of the first step (the kernels use its low 32 bits)
  // the same source for problem q, k steps on (eps is the caller's to move)
  Noise at(long long q, long long k) const {
    Noise n = *this;
    n.stream += (uint32_t)q * stride;
    n.step += k;
    return n;
  }
};

// learning_rate_schedule (vb.py:324-342) evaluated on the device for local step i.
// a, b, start, end are computed on the host with the reference's own float
// expression order; device fp64 division is IEEE, so lr(i) matches bit for bit.
struct LrSched {
  double lr, lr_end, a, b;
  long long start, end;
  int has_end;
  __host__ __device__ double at(long long i) const {
    if (!has_end || i < start) return lr;
    if (i < end) return a / (((b + (double)i) - (double)start) + 1.0);
    return lr_end;
  }
};

// Arguments of the column-pair persistent KLVI kernel (separable targets).
struct SepArgs {
  int D, N, W, n_pairs, n_steps, emit_grad;
  int pd;  // value with the sampled log q (black_box_klvi_pd): 0 off, 1 Gaussian, 2 t family
  long long step0, hist_start;  // local step index of the first step; 3*n_iters//4
  long long rng_step0;          // Philox step counter of the first step
  int n_waves;
  double t_scale, shape;  // t family: sqrt(df/2), df/2
  double eps;             // adagrad epsilon
  LrSched lr;
  double* lam;            // [P]
  double* ring;           // [W][P]
  double* hist;           // [n_hist][P]
  double* vpart;          // [n_steps][n_waves]
  double* grad;           // [P] (emit_grad)
  const double* noise;    // host noise [n_steps][N][D] or null
  uint32_t k0, k1, stream;
  int pairs2, blocks2, blocks1;  // filled by the launcher (2-pair / 1-pair split)
  // launch timing (vb_run_set_timing): the kStampStripe start words of this launch's
  // stamp slot, or null (timing off: the kernel takes no stamp)
  unsigned long long* stamp;
};

// Launch-time stamps (the constant 100 MHz clock), written with plain stores, one
// writer per word: the first kStampStripe blocks of sep_kernel (the blocks dispatched
// first, one per XCD) store their entry time into start word blockIdx.x, every block of
// sep_values_kernel the time after its store into end word blockIdx.x (a launch has at
// most kStampEnds steps); the host takes the min / max.  (Every block folding its time
// into a shared word with an atomic cost the headline launch ~10 us: ~1 300 blocks'
// atomics queue at a few addresses ahead of the table barrier,
// profiles/sep_launch/ab_short_atomics.log.)
constexpr int kStampStripe = 8;
constexpr int kStampEnds = 256;

// Arguments of the block-per-problem kernel (any target, D <= kBlockDMax).
struct BlockArgs {
  int D, N, W, P, n_steps, emit_grad, chivi;
  int pd;   // KLVI value -(mean log p - mean log q(x)) (black_box_klvi_pd)
  int opt;  // 0 adagrad window (history: post-update, tail quarter); 1 RMSProp-IA, 2 Adam-IA
            // (state in ring rows 0/1, history: pre-update, last n_hist iterations)
  long long step0, hist_start, n_iters, n_hist, rng_step0;
  double alpha;
  double t_scale, shape, t_const, df;  // t family constants
  double eps;
  LrSched lr;
  double* lam;          // [n_problems][P]
  double* ring;         // [n_problems][W][P]
  double* hist;         // [n_problems][n_hist][P]
  double* values;       // [n_problems][n_iters] (indexed by global step)
  double* grad;         // [n_problems][P] (emit_grad)
  const double* noise;  // host noise [n_problems][n_steps][N][D] or null
  // with noise: per-sample log q partials [n_problems][n_steps][N] (sum over the
  // column pairs, without -sum log sigma) from launch_block_predraw, or null
  const double* noise_lq;
  uint32_t k0, k1, stream, stream_stride;
  int pf;   // device-noise rows staged into LDS by a copy wave (VIABEL_AMD_BLOCK_PF, default on);
            // 2: also split rows (two lanes per sample) where block_layout allows them
};

// family kind 0 = mf gaussian, 1 = mf t; target kind per vb_target_kind.
hipError_t launch_sep(int fam, int tgt, bool host_noise, const SepArgs& a, hipStream_t s);
// block step skeleton without draws / target (vb_block_floor)
hipError_t launch_block_floor(int D, int N, bool host_layout, bool chivi, int n_steps, int nprob,
                              double* out, hipStream_t s, int pf = 0);
hipError_t launch_block(int fam, int tgt, bool host_noise, const BlockArgs& a, int n_problems,
                        hipStream_t s);
// whether device-noise blocks of this shape get the copy wave (its LDS ring fits)
bool block_pf_layout(int N, int D, bool need_lq, int pf_mode);
bool target_separable(int tgt);
// Pre-drawn block-kernel noise: the standardized draws of n_steps steps of
// n_problems problems, [q][s][N][D], bit-identical to the block kernel's own
// Philox draws (same counters: pair, sample, rng_step0 + s, stream + q * stride),
// and, when lq is non-null, each sample's log q partial sum [q][s][N].
hipError_t launch_block_predraw(const Family& f, int N, int n_steps, int n_problems,
                                const Noise& nz, double* noise, double* lq, hipStream_t s);

// values[i] = -(c0 + sum_w vpart[s][w]) for i = step0 + s; stamp_end: the launch's
// kStampEnds end words, or null
hipError_t launch_sep_values(const double* vpart, int n_steps, int n_waves, double c0,
                             double* values_at_step0, hipStream_t s,
                             unsigned long long* stamp_end = nullptr);
// out[p] = mean over rows of hist [rows][P]   (per problem block of rows)
hipError_t launch_row_mean(const double* hist, long long rows, long long P, long long n_problems,
                           double* out, hipStream_t s);

// elementwise family helpers
// Bailey t samples of a mean-field t family (the log-weight draws, vbrng.c family 2)
hipError_t launch_sample_bailey(const Family& f, long long m, const double* lam, const Noise& nz,
                                double* x, hipStream_t s);
hipError_t launch_sample(const Family& f, long long n, const double* lam, const Noise& nz,
                         double* x, hipStream_t s);
hipError_t launch_family_logdensity(const Family& f, long long n, const double* lam,
                                    const double* x, double* out, hipStream_t s);
hipError_t launch_target_logdensity(int tgt, int D, long long n, const double* x, double* out,
                                    double* grad, hipStream_t s);
// fused materialised step rows (draw, x, target log p + gradient, optional log q)
// for separable device targets with wide rows; see mfw_rows_kernel.  logp / logq
// receive mfw_rows_parts(D) chunk partials per row, laid out [part][n].
bool mfw_rows_fusable(int tgt, int D, long long n);
int mfw_rows_parts(int D);
hipError_t launch_mfw_rows(const Family& f, int tgt, long long n, const double* lam, bool with_lq,
                           const Noise& nz, double* x, double* grad, double* logp, double* logq,
                           hipStream_t s);
// rows > 1: lam [rows][2 D], lw [rows][m]; row q draws from stream + q * nz.stride
hipError_t launch_log_weights(const Family& f, int tgt, long long m, const double* lam,
                              const Noise& nz, double* lw, double* xs, hipStream_t s,
                              int rows = 1);
// scale (nullable): [min(step + 1, W)] window scales, oldest first
hipError_t launch_adagrad_update(long long P, double* lam, const double* g, double* ring, int W,
                                 long long step, double lr, double eps, const double* scale,
                                 hipStream_t s,
                                 double* hrow = nullptr);
// RMSProp-IA / Adam-IA step (opt 1 / 2) on device state [2][P], or (opt 3)
// RMSProp-IA with avg_grad_norm: every coordinate divided by sqrt(eps + norm2);
// old_out (nullable) receives the pre-update parameters.
hipError_t launch_ia_update(int opt, long long P, double* lam, const double* g, double* state,
                            long long step, double lr, double eps, double norm2,
                            double* old_out, hipStream_t s);
// R-hat (functions.py:8-31) of chains [nc][n][P] (row stride P) over n_jobs
// iteration segments [start, start + len) (len even): out [n_jobs][P] (var_hat
// in var_out when non-null).
hipError_t launch_rhat_stats(const double* chains, long long nc, long long n, long long P,
                             long long n_jobs, const long long* start, const long long* len,
                             double* mean_out, double* ss_out, hipStream_t s);
hipError_t launch_rhat_combine(const double* mean, const double* ss, long long nc2, long long P,
                               long long n_jobs, const long long* len, double* var_out,
                               double* rhat_out, hipStream_t s);
// cumulative means (functions.py:68-77) of x[start:, cols] with row stride ld
hipError_t launch_iterate_average(const double* x, long long n, long long ld, long long cols,
                                  long long start, double* out, hipStream_t s);

// bounds
hipError_t bounds_divergence(const double* lw, long long n, double alpha, int has_elbo,
                             double elbo, double* dev_scratch, double* out7_dev, hipStream_t s);
hipError_t bounds_divergence_rows(const double* lw, long long rows, long long n, long long ld,
                                  double alpha, int has_elbo, double elbo, double* scratch,
                                  double* out7, hipStream_t s);
size_t bounds_divergence_scratch_doubles(long long rows);
hipError_t bounds_centered_moments(const double* x, long long n, long long d,
                                   double* dev_scratch, double* out2_dev, hipStream_t s);
hipError_t bounds_covariance(const double* x, long long n, long long d, double* dev_scratch,
                             double* mean_dev, double* cov_dev, hipStream_t s);
size_t bounds_scratch_doubles(long long n, long long d);
size_t bounds_wcov_scratch_doubles(long long n, long long d);
hipError_t bounds_weighted_covariance(const double* x, long long n, long long d, const double* w,
                                      bool logw, int ddof, double* scratch, double* sc_out,
                                      double* mean, double* cov, hipStream_t s);
constexpr int kCovDMax = 64;

// PSIS (vb_psis.hip)
size_t psis_scratch_bytes(long long tail_cap);  // scratch for tails / gpdfit inputs <= tail_cap
long long psis_tail_max();
size_t psis_col_stride(long long tail_cap);      // scratch bytes per column of psis_columns
hipError_t psis_columns(const double* lw, double* out, long long n, int m, long long rs,
                        long long cs, long long Mt, void* scratch, double* k_dev,
                        long long* tail_idx_dev, long long tail_cap, long long* n_tail_dev,
                        hipStream_t s, unsigned* flag_dev = nullptr,
                        unsigned* flag_host = nullptr);
hipError_t psis_gpdfit(const double* x, long long n, void* scratch, double* out4,
                       double* ks_out, double* w_out, hipStream_t s);
hipError_t psis_gpinv(const double* p, long long n, double k, double sigma, double* out,
                      hipStream_t s);
size_t psis_sumlogs_rows_scratch_bytes(long long rows, long long n);
hipError_t psis_sumlogs_rows(const double* x, long long rows, long long n, void* scratch,
                             double* out, hipStream_t s);
hipError_t psis_sumlogs(const double* x, long long n, void* scratch, double* out, hipStream_t s);

}  // namespace vbk

// ---- full-rank Student-t family (vb_fr.hip) ----------------------------------
struct vb_ctx;
struct vb_plugin;
namespace vbk {

int vb_set_error(int code, const char* fmt, ...);  // defined in vb_capi.hip

constexpr int kFamilyFrT = 2;
constexpr int kTargetCorrGauss = 4;
constexpr int kTargetCallback = 5;
constexpr int kTargetRegression = 6;
constexpr int kTargetPlugin = 9;
// Regression target (vb_glm.hip): host copy of the parameter block's header
// (include/viabel_amd.h); X [M][D] starts kGlmHeader doubles into the block.
constexpr int kGlmHeader = 8;
struct GlmHead {
  int lik;            // 0 gaussian, 1 student_t, 2 bernoulli_logit, 3 poisson_log,
                      // 4 neg_binomial_2_log
  long long M;        // observations
  double nu, sigma, prior;
  // likelihoods 3 and 4: the dispersion (4), and the block's last value, the sum of the
  // data-only constants; eta0 [M] follows y in the block
  double phi, c_data;
  // learn = 1: the last coordinate is lambda = log sigma (likelihoods 0, 1) or log phi (4),
  // e^lambda ~ half-Cauchy(0, s_aux); X is [M][D - 1]; sigma / phi above are not used.
  // Likelihood 4: J and T [J] follow c_data in the block (J = 0: no table)
  int learn;
  double s_aux;
  long long J;
};
// log p [n] and (grad non-null) d log p / dx [n][D] of the rows of x [n][D] for the
// regression target whose parameter block is at `params` (device).  scratch holds
// glm_scratch_doubles(D, n, h, grad != null) doubles: the chunk partials (none for one
// chunk) and, for a learned dispersion, the table sums of the n rows.  Two identical
// calls give identical bits.
size_t glm_scratch_doubles(int D, long long n, const GlmHead& h, bool grad);
hipError_t launch_glm_rows(int D, long long n, const GlmHead& h, const double* params,
                           const double* x, double* logp, double* grad, double* scratch,
                           hipStream_t s);
constexpr int kTargetHierarchical = 7;
// Hierarchical normal means (vb_hier.hip): host copy of the parameter block's header
// (include/viabel_amd.h); y [J] starts kHierHeader doubles into the block, sigma [J]
// follows it.
constexpr int kHierHeader = 8;
struct HierHead {
  int centered;       // 0 non-centred, 1 centred
  long long J;        // groups; D = J + 2
  double mu_scale, tau_scale;
};
// log p [n] and (grad non-null) d log p / dx [n][D] of the rows of x [n][D] for the
// hierarchical target whose parameter block is at `params` (device).  grad == nullptr
// selects instances without any gradient operation or store.  No atomics and no
// scratch; a row's bits do not depend on n.
hipError_t launch_hier_rows(int D, long long n, const HierHead& h, const double* params,
                            const double* x, double* logp, double* grad, hipStream_t s);
constexpr int kTargetMultilevel = 8;
// Multilevel regression (vb_mlm.hip): host copy of the parameter block's header
// (include/viabel_amd.h); X [M][p] starts kMlmHeader doubles into the block, y [M] and
// the G + 1 group offsets follow it.
constexpr int kMlmHeader = 8;
struct MlmHead {
  int lik;            // 0 gaussian, 1 student_t, 2 bernoulli_logit, 3 poisson_log,
                      // 4 neg_binomial_2_log
  int centered;       // 0 non-centred, 1 centred
  long long M, G;     // observations, groups; D = p + 1 + G + learn
  double nu, sigma, prior, tau_scale;
  // likelihoods 3 and 4: the dispersion (4), and the sum of the data-only constants, the
  // last value of a fixed block; eta0 [M] follows the group offsets in the block
  double phi, c_data;
  // learn = 1: the last coordinate is lambda = log sigma (likelihoods 0, 1) or log phi (4),
  // e^lambda ~ half-Cauchy(0, s_aux); sigma / phi above are not used.  s_aux follows
  // everything a fixed block has; likelihood 4: J and T [J] follow it (J = 0: no table)
  int learn;
  double s_aux;
  long long J;
};
// p, the columns of X, from the dimension of the sample rows (< 1: no such block)
inline long long mlm_coefs(long long D, const MlmHead& h) { return D - 1 - h.G - h.learn; }
// log p [n] and (grad non-null) d log p / dx [n][D] of the rows of x [n][D] for the
// multilevel target whose parameter block is at `params` (device).  scratch holds
// mlm_scratch_doubles(D, n, h, grad != null) doubles of chunk partials.  grad == nullptr
// selects instances without gradient work; their values equal the with-gradient
// values bit for bit.  No atomics; two identical calls give identical bits.
size_t mlm_scratch_doubles(int D, long long n, const MlmHead& h, bool grad);
hipError_t launch_mlm_rows(int D, long long n, const MlmHead& h, const double* params,
                           const double* x, double* logp, double* grad, double* scratch,
                           hipStream_t s);
// host model callback (vb_target_callback) + its user pointer
struct HostTarget {
  int (*fn)(void* user, const double* x, int64_t n, int64_t d, double* logp, double* grad);
  void* user;
};
struct FrWork;
// Evaluate a host target on device x [n][D] into device logp [n] / grad [n][D]
// (grad nullable): staged through pinned buffers of the workspace; synchronises.
int host_target_eval(FrWork* W, const HostTarget& t, int D, long long n, const double* x,
                     double* logp, double* grad, hipStream_t st);


// Device model plugin (vb_plugin.hip): what a launch of the user's kernel needs, taken
// from a checked vb_plugin handle.  n_data: doubles in the target's data block.
struct PluginTarget {
  hipFunction_t function;
  int block, rows_per_block;
  long long n_data;
};
// Checks the handle (live, loaded on `device`, dim within its dmax) and fills *out.
int plugin_view(const vb_plugin* p, int device, long long dim, long long n_data, PluginTarget* out);
int plugin_retain(vb_plugin* p);   // one more reference (a vb_run's); vb_plugin_release drops it
// log p [n] and (grad non-null) d log p / dx [n][D] by the plugin's kernel on `st`:
// ceil(n / rows_per_block) blocks of `block` threads, no dynamic LDS, no synchronisation
int plugin_target_eval(const PluginTarget& p, int D, long long n, const double* data,
                       const double* x, double* logp, double* grad, hipStream_t st);
// (vb_capi.hip) the context's device, selected, and its stream; and a stream
// synchronisation that a context already destroyed turns into a no-op
int ctx_device_stream(vb_ctx* c, int* device, hipStream_t* stream);
int ctx_synchronize_if_alive(vb_ctx* c);

struct FrWork;  // per-context workspace + rocBLAS handle
FrWork* fr_work_create();
void fr_work_destroy(FrWork* w);

// A checked target (check_target in vb_capi.hip), with everything a launch needs.  A
// kind is wired in three places: its header parse in check_target fills the member of
// the union that belongs to it, target_eval (vb_fr.hip) has its case, and choose_path
// (vb_capi.hip) says which paths take it.  stage_target puts `params` on the device.
struct Target {
  int kind = 0, D = 0;
  const double* params = nullptr;  // device; corr_gauss: P* [D][D] and the log normaliser;
                                   // regression / hierarchical / multilevel / plugin: the block
  long long n_params = 0;          // doubles at params
  double tconst = 0.0;             // corr_gauss log normaliser
  union {                          // only the kind's own member is meaningful
    GlmHead glm;                   // kTargetRegression
    HierHead hier;                 // kTargetHierarchical
    MlmHead mlm;                   // kTargetMultilevel
    PluginTarget plugin;           // kTargetPlugin
    HostTarget host;               // kTargetCallback
  };
  Target() : glm{} {}
};
// log p [n] and (grad non-null) d log p / dx [n][D] of the rows of device x [n][D]: the one
// switch over the target kind.  The regression and multilevel chunk partials are reserved
// in the workspace; a callback synchronises; n == 0 evaluates nothing.
int target_eval(FrWork* W, const Target& t, long long n, const double* x, double* logp,
                double* grad, hipStream_t st);

// What the full-rank and the materialised mean-field paths evaluate: family, target
// and objective (N = 0 and no objective flags for log weights).
struct Spec {
  Family fam;
  int N, chivi, pd;
  double alpha;
  Target tgt;
};

// All return 0 or a VB_E* code (message via vb_set_error).
int fr_prepare(FrWork* W, int D, const double* lam, hipStream_t st);  // eigh of Sigma
// Newton-Schulz sqrtm; warm: Sigma is close to the previous call's (optimisation run)
int fr_sqrt(FrWork* W, int D, const double* lam, hipStream_t st, bool warm = false,
            const void* owner = nullptr, bool ready = false);
constexpr int kFrNSMax = 40;  // Newton-Schulz iterations launched at most per root
constexpr int kFrPcgMax = 192; // PCG iterations launched at most per gradient
// nz.eps (host draws) = [s (n), z (n x D)] on the device
int fr_draw(FrWork* W, const Family& f, long long n, const Noise& nz, const double** s_out,
            const double** z_out, hipStream_t st);
int fr_transform(FrWork* W, int D, long long n, const double* mu, const double* s,
                 const double* z, double* x, hipStream_t st);
struct MfUpdate;
// The next step of a fused run: its draws (rng step `step`) and L are prepared by
// this step's last kernel when `prep`.
struct FrNext {
  bool prep;
  uint32_t step;
};
// up (non-null, Philox draws): the windowed adagrad step is fused into the last
// kernel (lam updated in place, ring / history row written; grad keeps only the
// mean part), and with next->prep the step after it is prepared (FrWork).
int fr_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz, double* value,
                  double* grad, hipStream_t st, bool warm = false,
                  const void* owner = nullptr, const MfUpdate* up = nullptr,
                  const FrNext* next = nullptr);
int fr_logdensity(FrWork* W, const Family& f, const double* lam, const double* x, long long n,
                  double* out, hipStream_t st);
int fr_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                   double* lw, double* xs, hipStream_t st);
int fr_moments(FrWork* W, int D, const double* lam, double* sigma, double* eig, hipStream_t st);

// Mean-field families on the materialised path (any D, any objective / target).
// Optional windowed-adagrad step fused into the gradient pass (lam updated in
// place, the step's gradient pushed into ring [W][P], new parameters copied to
// hrow when non-null); same arithmetic as launch_adagrad_update without scales.
struct MfUpdate {
  double* ring;
  int W;
  long long step;
  double lr, eps;
  double* hrow;
};
int mf_wide_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz,
                       double* value, double* grad, hipStream_t st, const MfUpdate* up = nullptr);
int mf_wide_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                        double* lw, double* xs, hipStream_t st);
// 0, or a VB_E* code with the message set (eigendecomposition / Newton-Schulz /
// PCG failure since the last call); synchronises the stream.
// retry (non-null): a warm Newton-Schulz root that did not converge sets *retry,
// raises the learnt count and returns 0 (the caller runs the steps again).
int fr_info(FrWork* W, hipStream_t st, bool* retry = nullptr);
// Warm state of the next full-rank step (previous root, power vectors, schedule
// block): saved before a run's advance, restored when the advance runs again.
// Peak-rate microbenchmarks (vb_probe.hip): kind 0 HBM copy / 1 HBM read (GB/s,
// n bytes), 2 fp64 MFMA (TFLOP/s), 3 fp64 FMA / 4 u64 multiply VALU issue (G
// wave-instructions/s; n iterations).
int probe_rate(int kind, long long n, int reps, hipStream_t st, double* out);
// Device-math probe (vb_probe.hip): out[i] (out2[i], nullable) = helper fn at x[i].
bool math_probe_fn_ok(int fn);
hipError_t launch_math_probe(int fn, const double* x, long long n, double* out, double* out2,
                             hipStream_t st);
int fr_warm_save(FrWork* W, hipStream_t st);
int fr_warm_restore(FrWork* W, hipStream_t st);
// Clears the Newton-Schulz floor a rerun set (the rerun's own warm steps have
// taught fr_info the count they need).
void fr_retry_done(FrWork* W);
hipError_t launch_fr_lw(const Family& f, long long m, const double* logp, const double* zz,
                        const double* s, const double* scal, double* lw, hipStream_t st);

// ---- full-rank Gaussian family on its Cholesky factor (vb_frg.hip) -------------
constexpr int kFamilyFrGaussian = 3;
// Both full-rank kinds share the parameter layout [mu (D), tril(M) (D(D+1)/2)].
inline bool family_full_rank(int kind) { return kind == kFamilyFrT || kind == kFamilyFrGaussian; }
// The workspace's row buffers, reserved for n rows of dimension D: draws Z [n][D],
// samples X [n][D], target gradient G [n][D], logp / zz [n] and 8 scalars.  Taking
// them drops the t family's prepared next step (FrWork::prep_owner).
struct FrRows {
  double *Z, *X, *G, *logp, *zz, *scal;
};
int fr_rows(FrWork* W, int D, long long n, FrRows* out);
// nz.eps (host draws) = z [n][D] on the device, N(0,1)
int frg_sample(FrWork* W, const Family& f, const double* lam, long long n, const Noise& nz,
               double* x, hipStream_t st);
// up (non-null): the windowed adagrad step is fused into the gradient kernel's
// epilogue (lam updated in place, ring / history row written, grad untouched)
int frg_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz, double* value,
                   double* grad, hipStream_t st, const MfUpdate* up = nullptr);
int frg_logdensity(FrWork* W, const Family& f, const double* lam, const double* x, long long n,
                   double* out, hipStream_t st);
int frg_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                    double* lw, double* xs, hipStream_t st);

// ---- low-rank-plus-diagonal Gaussian family (vb_lrg.hip) ------------------------
// lambda = [mu (D), log_d (D), B row-major (D x R)], Sigma = B B^T + diag(exp(2 log_d)).
constexpr int kFamilyLrGaussian = 4;
constexpr int kLrgRankMax = 64;
// Standard normals per draw of a family on the FullRank / LowRank paths: z (D), the
// t family's scale s (1), the low-rank family's u (R).
inline size_t family_noise_width(const Family& f) {
  return (size_t)f.D + (f.kind == kFamilyFrT ? 1 : 0) + (f.kind == kFamilyLrGaussian ? f.R : 0);
}
// `doubles` of workspace that only vb_lrg.hip uses (kept across calls, grown on demand)
int fr_extra(FrWork* W, size_t doubles, double** out);
// nz.eps (host draws) = [n][D + R] on the device, N(0,1): each row is [z (D), u (R)]
int lrg_sample(FrWork* W, const Family& f, const double* lam, long long n, const Noise& nz,
               double* x, hipStream_t st);
// up (non-null): the windowed adagrad step is fused into the gradient kernel's
// epilogue (lam updated in place, ring / history row written, grad untouched)
int lrg_value_grad(FrWork* W, const Spec& f, const double* lam, const Noise& nz, double* value,
                   double* grad, hipStream_t st, const MfUpdate* up = nullptr);
int lrg_logdensity(FrWork* W, const Family& f, const double* lam, const double* x, long long n,
                   double* out, hipStream_t st);
int lrg_log_weights(FrWork* W, const Spec& f, const double* lam, long long m, const Noise& nz,
                    double* lw, double* xs, hipStream_t st);

}  // namespace vbk
