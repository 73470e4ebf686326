/* odin_hip.h -- C ABI of libodin_hip.so: the MI355X (gfx950) VAE training-step path.
 *
 * The reference (trungnt13/odin-ai) is pure Python: it has no FFI of its own, its device
 * arithmetic is executed by TensorFlow 2.5 / TFP 0.13 ops called from the Python files
 * cited below.  Each entry point here replaces one such call site; a maintainer binds
 * them with ctypes.  Conventions:
 *   - every pointer is a DEVICE pointer to fp32 (int32 where noted), borrowed for the
 *     duration of the call; nothing is allocated, freed or retained by the library;
 *   - activations are NHWC, Conv2D kernels (kh,kw,Cin,Cout), Conv2DTranspose kernels
 *     (kh,kw,Cout,Cin), Dense kernels (in,out) -- the Keras layouts, never transposed;
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it;
 *   - return value 0 = OK, negative = error (odin_last_error() has the text).
 * File:line citations are relative to the reference repository root.
 */
#ifndef ODIN_HIP_H
#define ODIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { ODIN_LINEAR = 0, ODIN_ELU = 1, ODIN_RELU = 2 };

/* Geometry of one Conv2D / Conv2DTranspose layer (TF `SAME` padding resolved by the
 * caller: pad_t/pad_l are the SAME "before" pads of the strided conv; for a transposed
 * conv they are the pads of the forward conv on the OUTPUT size). */
typedef struct odin_conv_desc {
  int B, H, W, Cin;   /* layer input  [B,H,W,Cin]   */
  int OH, OW, Cout;   /* layer output [B,OH,OW,Cout] */
  int KH, KW, stride;
  int pad_t, pad_l;
  int act;            /* fused epilogue activation (forward only) */
  int center;         /* fold CenterAt0 (2x-1) into the input load (image_networks.py:121-126) */
  /* Backward pass only, both optional (NULL): the dynamic-range side channel of the 4x4/stride-2 layers whose
   * fp32 operands travel through the f16 matrix pipe as two planes.  Each range word (a block of
   * ODIN_RANGE_WORDS uint32: 32 sub-words on separate memory lines, the bound is their maximum) holds the fp32
   * BIT PATTERN of an upper bound of max|t| of a gradient tensor t; the caller zeroes the words once per step
   * (odin_range_reset), producers fold their outputs in with one atomicMax per workgroup, consumers scale t by an
   * exact power of two on its way into the planes.  dy_amax: word of dy (this layer's pre-activation gradient) -- read by the data / weight gradient,
   * written by the fused tail that produces dy.  dx_amax: word of dx -- CONTRACT (round 5): a data gradient (and the
   * fused tail for dy_amax) that is handed a word leaves a valid bound in it whatever kernel family ran: folded in from
   * the kernel's epilogue where the family tracks its outputs (odin_*_dgrad_keeps_range = 1: free), by one extra pass
   * over the tensor otherwise.  A consumer without a word computes the bound itself (odin_absmax: one extra pass over
   * the tensor), and only if it is a plane kernel. */
  uint32_t* dy_amax;
  uint32_t* dx_amax;
  /* Forward pass only, both optional (NULL), round 5: the same side channel for ACTIVATIONS.  x_amax: range word of the
   * layer input x (read: a plane kernel whose input bound lies outside [2^-8, 2^15) carries x times the exact power of
   * two that brings it to [2^14, 2^15) -- f16 planes hold |x| <= 65504 and lose relative precision below 2^-25; inside
   * the window, and without a word, x is carried unscaled as in round 4: then the caller guarantees |x| <= 65504).
   * y_amax: range word of the layer output y (written, same contract as dx_amax: valid on return whatever family ran).
   * Weights are always carried unscaled: |w| <= 65504. */
  const uint32_t* x_amax;
  uint32_t* y_amax;
} odin_conv_desc;

/* ---- runtime ------------------------------------------------------------------------ */
int odin_version(void);
/* diagnostics: kernel family launched last by the calling thread ("...(f16x2)": fp32 operands through
 * the f16 matrix pipe as two planes); used by bench.py to price kernels against the right peak */
const char* odin_debug_last_path(void);
/* CRC-32C (Castagnoli) of host bytes, continuing from `crc` (0 to start): the checksum of the
 * TensorFlow checkpoint / event-file formats the reference saves (base_networks.py:373-390,
 * training/trainer.py:52-71).  Returns the checksum (not an error code). */
uint32_t odin_crc32c(uint32_t crc, const void* data, size_t n);
const char* odin_last_error(void);
int odin_max_slab_rows(void);      /* upper bound of the rows any slab-producing call writes */
/* Which producers keep a range word WITHOUT an extra pass: 1 when the data gradient of layer `d` (dispatched for
 * aux_act, aux present, no oversized column-sum slab) / the fused tail folds max|dx| / max|g_out| into d->dx_amax /
 * d->dy_amax from its own epilogue.  Informational since round 5 (cost model, tests): the word is valid either way. */
int odin_conv2d_dgrad_keeps_range(const odin_conv_desc* d, int aux_act);
int odin_deconv2d_dgrad_keeps_range(const odin_conv_desc* d, int aux_act);
int odin_bernoulli_tail_keeps_range(int is_deconv, const odin_conv_desc* d, int C1);
/* Range words (odin_conv_desc.dy_amax / dx_amax; ODIN_RANGE_WORDS uint32 each): zero `n` words at the top of a
 * step; fold max|t[0..n)| of an fp32 tensor into a word (producers that do not track their outputs themselves, or
 * external callers). */
#define ODIN_RANGE_WORDS 2048
int odin_range_reset(uint32_t* words, int n, void* stream);
int odin_absmax(const float* t, size_t n, uint32_t* word, void* stream);
/* diagnostics: a stream with the traffic of the fused Bernoulli ELBO kernel (out = a + b over n floats; 12 bytes per
 * element) in several launch shapes -- the ceiling bench.py prices that kernel against beside the 8 TB/s peak */
int odin_debug_stream_probe(const float* a, const float* b, float* out, size_t n, int variant, int blocks,
                            void* stream);
/* diagnostics: how many times a consumer had to bound a gradient tensor itself (no range word given) */
int odin_debug_absmax_fallbacks(void);

/* ---- Conv2D (keras.layers.Conv2D, odin/networks/image_networks.py:166-169,463-466) --- */
int odin_conv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                    const odin_conv_desc* d, void* stream);
/* dx = conv2d_backprop_input(dy) * act'(aux);  replaces tape.gradient
 * (odin/networks/base_networks.py:514-518).  aux = the layer's INPUT activation (post
 * activation of the previous layer) or NULL.  colsum_slab (optional,
 * [*slab_rows_out][Cin]) receives per-workgroup column sums of dx (the bias gradient
 * of the previous layer when that layer is a Conv2DTranspose). */
int odin_conv2d_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                      float* colsum_slab, int* slab_rows_out, const odin_conv_desc* d,
                      void* stream);
/* Slab-producing calls: passing the output pointer (dx / slab) as NULL is a DRY RUN that only
 * reports *slab_rows_out (used to size workspaces).
 * slab[g][kh,kw,Cin,Cout | Cout] partial (dW | db) per workgroup g < *slab_rows_out;
 * finish with odin_slab_reduce.  x = layer input, dy = grad wrt pre-activation output. */
int odin_conv2d_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out,
                      const odin_conv_desc* d, void* stream);

/* ---- Conv2DTranspose (odin/networks/image_networks.py:170-173,497-505) ---------------- */
int odin_deconv2d_fwd(const float* x, const float* w, const float* bias, float* y,
                      const odin_conv_desc* d, void* stream);
int odin_deconv2d_dgrad(const float* dy, const float* w, const float* aux, int aux_act,
                        float* dx, float* colsum_slab, int* slab_rows_out,
                        const odin_conv_desc* d, void* stream);
/* slab[g][kh,kw,Cout,Cin] partial dW (bias grad comes from the producer's colsum slab) */
int odin_deconv2d_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out,
                        const odin_conv_desc* d, void* stream);

/* ---- a layer's whole backward pass in ONE call: weight gradient (wslab as in *_wgrad) + data gradient (dx,
 * colsum_slab as in *_dgrad; same argument meaning, same results bit for bit).  Where both halves run on the
 * small-layer implicit-GEMM kernels they share one launch -- each alone is a latency-bound launch of a few hundred
 * workgroups -- otherwise the call is the two calls above.  Replaces the tape.gradient of one layer
 * (odin/networks/base_networks.py:514-518).
 * Round 5: a Conv2DTranspose(k4, s2) over 32 or 64 output channels whose rows are 8 / 16 / 32 pixels wide back-propagates
 * in ONE launch that fetches, scales and splits dy once for both gradients (bwd_planes.hip; needs aux_act = ELU).  With
 * 32 output channels the results are still bit-identical to the two calls; with 64 the weight-gradient slab is
 * partitioned like the data gradient's tiles (equal to rounding) and has MORE rows than odin_deconv2d_wgrad reports: a
 * dry run of odin_deconv2d_bwd (every pointer NULL, aux_act as it will be passed) reports the rows of the one-call
 * form -- size the slab for the larger of the two. */
int odin_conv2d_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                    float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out,
                    const odin_conv_desc* d, void* stream);
int odin_deconv2d_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                      float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out,
                      const odin_conv_desc* d, void* stream);
/* The FIRST layer's weight gradient folded into the data gradient of the layer above it: d = the second layer, a
 * Conv2D(32 -> 32, k4, s2) with 16 x 16 outputs, dy / w / aux / aux_act / dx as in odin_conv2d_dgrad (aux_act = ELU;
 * colsum_slab / colsum_rows_out optional, as there); d0 =
 * the first layer, a Conv2D(1 -> 32, k4, s2, SAME) on a 64 x 64 image x0 (d0->center honoured).  ONE launch computes dx,
 * and from the dx tile it holds the partial (dW0 | db0) rows wslab0[g][16 * 32 | 32], g < *wslab0_rows_out, in the
 * layout of odin_conv2d_wgrad(x0, dx, ..., d0) -- the same fp32 products, summed in that kernel's order inside a
 * workgroup (the same bits after odin_slab_reduce where both give a workgroup one image: 256 samples on 256 CUs).  dx == NULL: the
 * gradient is not stored at all (nothing below the first layer needs it); dx != NULL: dx and d->dx_amax exactly as
 * odin_conv2d_dgrad leaves them.  wslab0 == NULL: dry run (rows only).  -2: shapes outside the kernel, nothing is
 * launched -- the caller keeps the two calls. */
int odin_conv2d_dgrad_first(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                            float* colsum_slab, int* colsum_rows_out, const odin_conv_desc* d, const float* x0,
                            float* wslab0, int* wslab0_rows_out, const odin_conv_desc* d0, void* stream);
/* Dense: either half may be left out (want_wgrad / want_dgrad); dy_amax / dx_amax are the optional range words of dy
 * (read) and dx (written: from the epilogue when odin_dense_dgrad_keeps_range(B, K, N) = 1, by one extra pass
 * otherwise) -- layers with both widths >= 256 run on the
 * f16 matrix pipe as two planes (dense_h.hip) like the 4x4/s2 convolutions. */
int odin_dense_bwd(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                   float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out, int B, int K,
                   int N, int want_wgrad, int want_dgrad, const uint32_t* dy_amax, uint32_t* dx_amax, void* stream);
/* The Dense entry points with the ACTIVATION range words of round 5 (odin_conv_desc.x_amax / y_amax: same contract):
 * x_amax (optional) is read by the two-plane GEMM (forward, and the weight gradient's x operand), y_amax (optional) is
 * valid on return whatever family ran. */
/* 1: a launch of this layer (forward or weight gradient, as dispatched now) reads the range word of the layer input:
 * the caller asks the layer below to keep that word only then (a wrong 0 is harmless: no word = unscaled = round 4). */
int odin_conv2d_reads_x_range(const odin_conv_desc* d);
int odin_deconv2d_reads_x_range(const odin_conv_desc* d);
int odin_dense_reads_x_range(int B, int K, int N);
int odin_dense_fwd_ranged(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, int act,
                          const uint32_t* x_amax, uint32_t* y_amax, void* stream);
int odin_dense_bwd_ranged(const float* x, const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                          float* colsum_slab, int* colsum_rows_out, float* wslab, int* wslab_rows_out, int B, int K,
                          int N, int want_wgrad, int want_dgrad, const uint32_t* dy_amax, uint32_t* dx_amax,
                          const uint32_t* x_amax, void* stream);
int odin_dense_dgrad_keeps_range(int B, int K, int N);

/* ---- fused decoder tail of the TRAINING step: layer (Conv2DTranspose if is_deconv else
 * Conv2D, activation d->act, Cout<=32) -> Conv2D 1x1 linear with C1<=4 maps (w1 [Cout,C1],
 * b1 [C1]) -> Independent(Bernoulli(logits),3).log_prob(target), forward AND backward:
 *   logits (optional out), g_out = dL/d(pre-activation of the layer) for
 *   L = -scale[0]*sum llk, llk_part[b][part] (n_part per sample), and
 *   tail_slab[g][Cout*C1 (dW1) | C1 (db1) | Cout (db of the layer)], g < *slab_rows_out.
 * The [B,OH,OW,Cout] activation never reaches HBM.  Replaces decoder4->decoder6->Bernoulli
 * (odin/networks/image_networks.py:505-511,87-93) + px.log_prob(x)
 * (variational_autoencoder.py:528-530) + their tape.gradient.  g_out==NULL = dry run. */
int odin_bernoulli_tail_fwd_bwd(int is_deconv, const float* x, const float* w, const float* bias,
                                const float* w1, const float* b1, const float* target,
                                float* logits, float* g_out, float* llk_part, int* n_part_out,
                                float* tail_slab, int* slab_rows_out, const float* scale,
                                const odin_conv_desc* d, int C1, void* stream);

/* ---- the same tail with the Conv2DTranspose BELOW it in the same launch (tconv_planes.hip: tconv_chain2_kernel): d3 =
 * Conv2DTranspose(k4, s2, ELU) [B,16,16,64] -> y3 [B,32,32,32] (decoder3 of the 64 x 64 image stacks; x, w3, b3; d3->x_amax
 * optional, d3->y_amax optional: receives the word of y3 as odin_deconv2d_fwd leaves it), d4 = the tail's layer on y3
 * (w4, b4; d4->dy_amax as in odin_bernoulli_tail_fwd_bwd; d4->x_amax is not read).  The forward pass couples no
 * samples: a workgroup owns whole images, runs d3 for them and goes straight on to the tail for the same images.
 * y3, logits and g_out are what the two calls compute, bit for bit; llk_part, the slab rows and the word of g_out
 * depend on the partition as they do in the tail itself: *same_partition_out = 1 where the chain's partition is that
 * of odin_bernoulli_tail_fwd_bwd -- then they are bit-identical too (provided the bound of every workgroup's part of y3
 * lies inside [2^-8, 2^15) whenever the batch's does: the tail scales y3 by its OWN images' bound).
 * y3 == NULL = dry run (n_part, rows, same_partition).  -2: shapes outside the chain, the plane kernels switched off. */
int odin_decoder_tail_chain(const float* x, const float* w3, const float* b3, float* y3, const odin_conv_desc* d3,
                            const float* w4, const float* b4, const float* w1, const float* b1, const float* target,
                            float* logits, float* g_out, float* llk_part, int* n_part_out, float* tail_slab,
                            int* slab_rows_out, int* same_partition_out, const float* scale, const odin_conv_desc* d4,
                            int C1, void* stream);

/* ---- Dense (keras Dense: base_networks.py:1002-1014; DistributionDense projection:
 * odin/bay/layers/dense_distribution.py:229-238) ------------------------------------- */
int odin_dense_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K,
                   int N, int act, void* stream);
int odin_dense_dgrad(const float* dy, const float* w, const float* aux, int aux_act, float* dx,
                     float* colsum_slab, int* slab_rows_out, int B, int K, int N, void* stream);
/* slab[g][K*N | N] partial (dW | db) */
int odin_dense_wgrad(const float* x, const float* dy, float* slab, int* slab_rows_out, int B,
                     int K, int N, void* stream);

/* dst[i] = sum_{g<rows} src[g*stride + i], i < n; any number of jobs per call. */
typedef struct odin_reduce_job {
  const float* src;
  float* dst;
  int n;      /* elements reduced per row */
  int rows;   /* G */
  int stride; /* floats between consecutive slab rows (0 = n) */
  int pad_;
} odin_reduce_job;
int odin_slab_reduce(const odin_reduce_job* jobs, int n_jobs, void* stream);

/* ---- latent posterior q(z|x) = MVNDiag(loc, softplus(raw))
 * MultivariateNormalLayer.new (odin/bay/layers/continuous.py:459-483), sample =
 * loc + scale*eps, KL: kl_divergence (odin/bay/helpers.py:177-282): analytic=0 -> MC
 * log q(z) - log p(z) at the same z; analytic=1 -> closed form KL(q||p); analytic=2 -> closed
 * form KL(p||q) (`reverse=False`, helpers.py:261-262); free_bits<0 = disabled,
 * else max(kl, free_bits*D).   p [B,2D], eps [B,D] -> z [B,D], kl [B] (after free bits),
 * fbmask [B] (1 where the gradient flows).  capacity (optional DEVICE scalar C(step)): BetaCapacityVAE
 * (odin/bay/vi/autoencoder/beta_vae.py:132-177) -- kl <- |kl - C|, fbmask <- fbmask * sign(kl - C). */
int odin_latent_fwd(const float* p, const float* eps, float* z, float* kl, float* fbmask, int B,
                    int D, int analytic, float free_bits, const float* capacity, void* stream);
/* dp [B,2D] of  L = sum_b klw[0]*kl_b  given dz (+ dz_extra) = dL/dz from the decoder
 * / regularisers (may be NULL) and optional extra grads (dloc_x, dscale_x: total correlation).  klw is a DEVICE scalar
 * (= beta / B) so that graph replays see schedule updates. */
int odin_latent_bwd(const float* p, const float* eps, const float* z, const float* dz,
                    const float* dz_extra, const float* fbmask, const float* klw,
                    const float* dloc_x, const float* dscale_x, float* dp, int B, int D,
                    int analytic, void* stream);

/* ---- latent posterior q(z|x) = MultivariateNormalTriL(loc, L): the full-covariance Gaussian (latent_tril.hip)
 * MultivariateNormalLayer.new with covariance='tril' (odin/bay/layers/continuous.py:459-474; RVconf(D, 'mvntril',
 * projection=True), odin/bay/distribution_alias.py:22-23); the prior stays N(0, I) (random_variable.py:80-86).
 * p [B, D + M], M = D (D + 1) / 2: loc = p[:, :D], r = p[:, D:] (loc_activation None) and
 *   L = FillScaleTriL(diag_bijector=softplus, diag_shift=1e-5)(r): r[D:] followed by r reversed are D * D values, read
 *   row-major as a D x D matrix of which the lower triangle is kept -- for j <= i and k = i D + j:
 *     L_raw[i][j] = r[D + k] if k < M - D, else r[D D - 1 - k]      (r = [1 .. 6] -> [[4, 0, 0], [6, 5, 0], [3, 2, 1]])
 *   L_ii = softplus(L_raw_ii) + 1e-5, off-diagonal entries unchanged.
 * z = loc + L eps;  log q(z) = -1/2 |eps|^2 - sum_i log L_ii - D/2 log 2 pi;  log p(z) = -1/2 |z|^2 - D/2 log 2 pi.
 * KL as odin_latent_fwd's `analytic`: 0 = the single-sample Monte-Carlo log q(z) - log p(z) at the z written
 * (helpers.py:267-276), 1 = the closed form 1/2 (|L|_F^2 + |loc|^2 - D) - sum_i log L_ii; 2 (KL(p || q): needs the
 * inverse of L) is refused.  free_bits / capacity / fbmask act on the per-sample scalar exactly as in odin_latent_fwd.
 * backward, with w = klw[0] fbmask_b and g = dz + dz_extra (either may be NULL):
 *   analytic 0: gz = g + w z; dloc = gz;  dL_ij = gz_i eps_j - w delta_ij / L_ii
 *   analytic 1: dloc = g + w loc;         dL_ij = g_i eps_j + w (L_ij - delta_ij / L_ii)
 *   dr = dL_ij off the diagonal, dL_ii sigmoid(L_raw_ii) on it (through the inverse of the fill map)
 * Every element of dp [B, D + M] is written exactly once, no float atomics: bit-reproducible.  dp_amax (optional): the
 * range word of dp, max |dp| folded in (the projection's gradient kernels read it where they run on two planes: both
 * widths >= 256 and multiples of 8, at least 32 rows -- D = 29, 32, 45, ..., not D = 22 with its 275 columns).  klw is a DEVICE scalar as in odin_latent_bwd.
 * odin_latent_tril_sample_logprob: the companion of odin_latent_sample_logprob (p: [B, D + M], eps / z: [n, B, D],
 * logq / logp: [n, B]).
 * Limits (a negative return code otherwise, nothing launched, no output touched): 1 <= D <= 64 (one row of L per lane of
 * a wave), 1 <= B (n B) <= 2^31 - 16. */
int odin_latent_tril_fwd(const float* p, const float* eps, float* z, float* kl, float* fbmask, int B, int D,
                         int analytic, float free_bits, const float* capacity, void* stream);
int odin_latent_tril_bwd(const float* p, const float* eps, const float* z, const float* dz, const float* dz_extra,
                         const float* fbmask, const float* klw, float* dp, uint32_t* dp_amax, int B, int D,
                         int analytic, void* stream);
int odin_latent_tril_sample_logprob(const float* p, const float* eps, float* z, float* logq, float* logp, int n,
                                    int B, int D, void* stream);

/* ---- latent posterior q(z|x) = RelaxedOneHotCategorical(tau, logits): the Concrete / Gumbel-softmax latent
 * (latent_concrete.hip).  RelaxedOneHotCategoricalLayer (odin/bay/layers/discrete.py:286-343; RVconf(K, 'relaxedonehot',
 * projection=True), odin/bay/distribution_alias.py:113-114) is ONE K-way variable; the prior is OneHotCategorical with
 * equal logits (random_variable.py:141-146).  p [B, K] are the logits l (no activation), tau > 0 a constant.
 *   g ~ Gumbel(0, 1);  u = (l + g) / tau;  y = u - logsumexp(u);  z = exp(y)  (on the simplex; the decoder's input)
 *   log q(z) = lgamma(K) + (K - 1) log tau + sum_k log_softmax(l - tau y)_k - sum_k y_k
 *            = lgamma(K) + (K - 1) log tau - sum_k g_k - K logsumexp(-g) - sum_k y_k   (the form evaluated)
 *   log p(z) = -log K sum_k z_k
 * All arithmetic stays in y -- log(z) is never taken: where z underflows to 0 (tau = 0.1) kl, logq and dp stay finite.
 * KL as odin_latent_fwd's `analytic`: 0 = the single-sample log q(z) - log p(z) at the z written (helpers.py:267-276),
 * 1 = the categorical KL of Jang et al., sum_k pi_k (log pi_k + log K) with pi = softmax(l) (a departure: TFP registers
 * no KL between the two distributions).  free_bits (units: K) / capacity / fbmask act on the per-sample scalar exactly
 * as in odin_latent_fwd.
 * odin_rng_gumbel: out[e] = -log(-log U_e), U_e = ((bits >> 8) + 0.5) 2^-24 with `bits` component e & 3 of Philox counter
 *   e >> 2 under (seed, step_dev[0]) -- odin_rng_normal's counter scheme; never 0 or 1, so every value is finite and lies
 *   in [-2.86, 17.33].
 * odin_latent_concrete_fwd: draw = 0 reads the noise g [B, K]; draw = 1 draws it in the kernel -- bit for bit the stream
 *   odin_rng_gumbel writes for (seed, step_dev) -- and STORES it to g (VAEEngine._latent_fwd: the step needs no RNG
 *   launch).  Writes z [B, K], kl [B], fbmask [B].
 * odin_latent_concrete_bwd (VAEEngine._backward_enc), with w = klw[0] fbmask_b, G = dz + dz_extra (either may be NULL),
 *   a_j = G_j - sum_k G_k z_k:
 *     analytic 0: dl_j = (z_j a_j - w (1 - K z_j)) / tau
 *     analytic 1: dl_j = z_j a_j / tau + w pi_j (log pi_j - sum_k pi_k log pi_k)
 *   klw is a DEVICE scalar as in odin_latent_bwd (graph replays see the beta schedule).  The gradients need z alone: g is
 *   the step's noise buffer and is not read (it may be NULL).  Every element of dp [B, K] is written exactly once, no
 *   float atomics: bit-reproducible.
 * odin_latent_concrete_sample_logprob (VariationalAutoencoder.marginal_log_prob): the companion of
 *   odin_latent_tril_sample_logprob -- p [B, K], g / z [n, B, K], logq / logp [n, B] (the single-sample forms above).
 * One wave per sample, lane k owns category k.  Limits (-2, nothing launched, no output touched): 2 <= K <= 64,
 * 1 <= B (n B) <= 2^31 - 16, tau > 0, analytic in {0, 1}. */
int odin_rng_gumbel(float* out, size_t n, uint64_t seed, const int32_t* step_dev, void* stream);
int odin_latent_concrete_fwd(const float* p, float* g, float* z, float* kl, float* fbmask, int B, int K, float tau,
                             int analytic, float free_bits, const float* capacity, int draw, uint64_t seed,
                             const int32_t* step_dev, void* stream);
int odin_latent_concrete_bwd(const float* p, const float* g, const float* z, const float* dz, const float* dz_extra,
                             const float* fbmask, const float* klw, float* dp, int B, int K, float tau, int analytic,
                             void* stream);
int odin_latent_concrete_sample_logprob(const float* p, const float* g, float* z, float* logq, float* logp, int n,
                                        int B, int K, float tau, void* stream);

/* ---- latent posterior q(z|x) = RelaxedBernoulli(tau, logits): the binary Concrete latent (latent_binconcrete.hip).
 * RelaxedBernoulliLayer (odin/bay/layers/discrete.py:346 ff.; RVconf(D, 'relaxedbern' | 'relaxedsigmoid' |
 * 'relaxedbernoulli', projection=True), odin/bay/distribution_alias.py:111-112) is D INDEPENDENT binary units; the prior
 * is Independent(Bernoulli(logits = 0)) (random_variable.py:149-154).  p [B, D] are the logits l (no activation), tau > 0
 * a constant.
 *   n ~ Logistic(0, 1);  u = (l + n) / tau;  z = sigmoid(u)  (in (0, 1)^D; the decoder's input)
 *   log q(z) = sum_d [ log tau - n_d - 2 softplus(-n_d) + softplus(u_d) + softplus(-u_d) ]
 *            = D log tau + sum_d [ S(u_d) - S(n_d) ],  S(x) = |x| + 2 log1p(exp(-|x|))       (the form evaluated)
 *   log p(z) = -D log 2
 * All arithmetic stays in u -- log z and log(1 - z) are never taken: where z rounds to exactly 0 or 1 (tau = 0.1) kl,
 * logq and dp stay finite.
 * KL as odin_latent_fwd's `analytic`: 0 = the single-sample log q(z) + D log 2 at the z written (helpers.py:267-276; it
 * may be negative), 1 = the Bernoulli KL of Jang et al., sum_d [pi log pi + (1 - pi) log(1 - pi) + log 2] with
 * pi = sigmoid(l) (a departure: TFP registers no KL between the two distributions), evaluated per unit as
 * t tanh t - log cosh t, t = l / 2, in a form that keeps its relative precision at l -> 0.  free_bits (units: D) /
 * capacity / fbmask act on the per-sample scalar exactly as in odin_latent_fwd.
 * odin_rng_logistic: out[e] = the Logistic(0, 1) value of `bits`, component e & 3 of Philox counter e >> 2 under
 *   (seed, step_dev[0]) -- odin_rng_normal's counter scheme.  With m = bits >> 8: m < 2^23: a = (m + 0.5) 2^-24,
 *   log a - log1p(-a); otherwise the exact complement c = (2^24 - m - 0.5) 2^-24, log1p(-c) - log c.  Every value is
 *   finite, |out| <= 25 ln 2 < 17.33, and the map is exactly antisymmetric in m <-> 2^24 - 1 - m.
 * odin_latent_relaxedbern_fwd: draw = 0 reads the noise n [B, D]; draw = 1 draws it in the kernel -- bit for bit the
 *   stream odin_rng_logistic writes for (seed, step_dev) -- and STORES it to n (VAEEngine._latent_fwd: the step needs no
 *   RNG launch).  Writes z [B, D], kl [B], fbmask [B].
 * odin_latent_relaxedbern_bwd (VAEEngine._backward_enc), with w = klw[0] fbmask_b, G = dz + dz_extra (either may be
 *   NULL):
 *     analytic 0: dl_d = (G_d z_d (1 - z_d) + w (2 z_d - 1)) / tau
 *     analytic 1: dl_d = G_d z_d (1 - z_d) / tau + w pi_d (1 - pi_d) l_d
 *   klw is a DEVICE scalar as in odin_latent_bwd (graph replays see the beta schedule).  z (1 - z) and 2 z - 1 are formed
 *   from u = (l + n) / tau: the noise n is READ, the stored z is not (it may be NULL).  Every element of dp [B, D] is
 *   written exactly once, no float atomics: bit-reproducible.
 * odin_latent_relaxedbern_sample_logprob (VariationalAutoencoder.marginal_log_prob): the companion of
 *   odin_latent_concrete_sample_logprob -- p [B, D], n / z [n_samples, B, D], logq / logp [n_samples, B] (logp is the
 *   constant -D log 2).
 * One wave per sample, lane k owns units k, k + 64, k + 128, k + 192.  Limits (-2, nothing launched, no output touched):
 * 1 <= D <= 255, 1 <= B (n_samples B) <= 2^31 - 16, tau > 0, analytic in {0, 1}. */
int odin_rng_logistic(float* out, size_t n, uint64_t seed, const int32_t* step_dev, void* stream);
int odin_latent_relaxedbern_fwd(const float* p, float* n, float* z, float* kl, float* fbmask, int B, int D, float tau,
                                int analytic, float free_bits, const float* capacity, int draw, uint64_t seed,
                                const int32_t* step_dev, void* stream);
int odin_latent_relaxedbern_bwd(const float* p, const float* n, const float* z, const float* dz, const float* dz_extra,
                                const float* fbmask, const float* klw, float* dp, int B, int D, float tau, int analytic,
                                void* stream);
int odin_latent_relaxedbern_sample_logprob(const float* p, const float* n, float* z, float* logq, float* logp,
                                           int n_samples, int B, int D, float tau, void* stream);

/* ---- the bottleneck as one launch per direction (latent_block.hip): DistributionDense(P -> 2D) ->
 * MVNDiag(loc, softplus(raw)) -> reparameterised sample + KL term -> the decoder's first Dense(D -> N0)
 * (dense_distribution.py DistributionDense; variational_autoencoder.py:515-542; helpers.py:236-286;
 * image_networks.py:494-497), i.e. odin_rng_normal + odin_dense_fwd + odin_latent_fwd + odin_dense_fwd,
 * and in the backward pass odin_dense_dgrad/wgrad + odin_latent_bwd + odin_dense_wgrad/dgrad.
 * odin_latent_block_rows: workgroups (= slab rows the backward launch writes), 0 when the shapes are
 * outside the fused regime (both weight matrices must fit in LDS).
 * forward: h [B,P] encoder output, wl [P,2D], bl [2D]; eps_in [B,D] or NULL = draw the noise from the
 * Philox stream of odin_rng_normal(seed, step_dev) and store it in eps_out; writes p [B,2D], z [B,D],
 * kl [B], fbmask [B] exactly like odin_latent_fwd and y0 = act0(z w0 + b0) [B,N0].
 * backward: g0 [B,N0] = dL/d(pre-activation of that Dense); klw / dz_extra / dloc_x / dscale_x as in
 * odin_latent_bwd; writes dz [B,D], dp [B,2D], dh = (dp wl^T) * act'(h) [B,P] and one partial row per
 * workgroup of slab0 [rows][D*N0 + N0] = (dW0 | db0) and slabl [rows][P*2D + 2D] = (dWl | dbl);
 * dh_amax (optional): the range word of dh (ODIN_RANGE_WORDS, below), max |dh| folded in. */
int odin_latent_block_rows(int B, int P, int D, int N0);
int odin_latent_block_fwd(const float* h, const float* wl, const float* bl, const float* eps_in,
                          float* eps_out, uint64_t seed, const int32_t* step_dev, float* p, float* z,
                          float* kl, float* fbmask, const float* w0, const float* b0, float* y0, int B,
                          int P, int D, int N0, int act0, int analytic, float free_bits,
                          const float* capacity, void* stream);
int odin_latent_block_bwd(const float* g0, const float* w0, const float* z, const float* p,
                          const float* eps, const float* fbmask, const float* klw, const float* dz_extra,
                          const float* dloc_x, const float* dscale_x, const float* wl, const float* h,
                          int h_act, float* dz, float* dp, float* dh, float* slab0, float* slabl, int B,
                          int P, int D, int N0, int analytic, uint32_t* dh_amax, void* stream);

/* ---- the NECK of the 64x64 stacks in one launch per direction (round 6; neck.hip): the encoder's last convolution
 * and projection, the latent block above, the decoder's projection and first Conv2DTranspose
 *   image_networks.py:466-471  Conv2D(64, 4, 2, 'same', act3) on [8,8,64] -> [4,4,64]; Flatten; Dense(P, act4)
 *   dense_distribution.py:339-380 / continuous.py:443-483 / helpers.py:236-286  (as odin_latent_block_*)
 *   image_networks.py:494-502  Dense(D -> 16 C0, act0); Reshape(4,4,C0); Conv2DTranspose(64, 4, 2, 'same', act1)
 * i.e. odin_conv2d_fwd + odin_dense_fwd + odin_latent_block_fwd + odin_deconv2d_fwd of those layers (and in the
 * backward pass their DATA gradients plus the weight gradients of the three small matrices; the two large weight
 * gradients -- conv3: a reduction over all B*16 pixels, projection: over the batch -- stay odin_conv2d_wgrad /
 * odin_dense_wgrad on dy3 / dh4, which the backward launch leaves with their range words).  No layer of the chain
 * couples samples: a workgroup owns two samples.  Same results as the separate calls to fp32 rounding (the conv runs
 * as two f16 planes per operand like the plane kernels: <= 3 * 2^-22 per product).
 * odin_neck_rows: workgroups (= rows of slab1 / slab0 / slabl), 0 when the shapes are outside the fused regime
 * (P in {128, 256}, C0 in {8, 16}, D <= 32). */
typedef struct odin_neck_args {
  int B, P, D, C0;                 /* batch, projection width, latent dims, channels of the decoder's first image */
  int act2, act3, act4, act0, act1;/* activations: of the layer BELOW conv3 (backward: dx *= act2'(x)), conv3, projection, decoder projection, deconv1 */
  int analytic;                    /* KL form as odin_latent_fwd: 0 Monte Carlo, 1 KL(q||p), 2 KL(p||q) */
  float free_bits;                 /* < 0: off */
  uint64_t seed;                   /* Philox key of odin_rng_normal (eps_in == NULL) */
  const int32_t* step_dev;         /* device int: the RNG step */
  /* ---- forward ---- */
  const float* x;                  /* [B,8,8,64] input of conv3 (output of the layer below) */
  const uint32_t* x_amax;          /* its activation range word or NULL */
  const float *w3, *b3;            /* Conv2D (4,4,64,64), [64] */
  float* y3;                       /* [B,4,4,64] */
  const float *w4, *b4;            /* Dense (1024,P), [P] */
  float* y4;                       /* [B,P] */
  const float *wl, *bl;            /* DistributionDense (P,2D), [2D] */
  const float* eps_in;             /* [B,D] or NULL: draw */
  float* eps;                      /* [B,D] written when drawn */
  float *p, *z, *kl, *fbmask;      /* [B,2D], [B,D], [B], [B] */
  const float* capacity;           /* BetaCapacityVAE device scalar or NULL */
  const float *w0, *b0;            /* Dense (D,16*C0), [16*C0] */
  float* y0;                       /* [B,16*C0] = [B,4,4,C0] */
  const float *w1, *b1;            /* Conv2DTranspose (4,4,64,C0), [64] */
  float* y1;                       /* [B,8,8,64]; NULL: the launch stops behind the latent block (p, z, kl, fbmask: the encoder's half) */
  uint32_t* y1_amax;               /* activation range word of y1 (written) or NULL */
  /* ---- backward (forward tensors above are read) ---- */
  const float* dy1;                /* [B,8,8,64] dL/d(pre-activation of deconv1) */
  const float* klw;                /* device scalar: KL weight beta / B */
  const float *dz_extra, *dloc_x, *dscale_x;   /* optional extra terms as odin_latent_bwd */
  float *dz, *dp;                  /* [B,D], [B,2D] */
  float* dh4;                      /* [B,P]  dL/d(pre-activation of the projection) */
  float* dy3;                      /* [B,4,4,64] dL/d(pre-activation of conv3) */
  float* dx;                       /* [B,8,8,64] dL/d(pre-activation of the layer below) = conv3's data gradient * act2'(x) */
  uint32_t *dh4_amax, *dy3_amax, *dx_amax;     /* gradient range words (written) or NULL */
  float* slab1;                    /* [rows][16*64*C0]       partial dW1 (deconv1's bias gradient: column sums of dy1, the caller's) */
  float* slab0;                    /* [rows][D*16*C0 + 16*C0] partial (dW0 | db0) */
  float* slabl;                    /* [rows][P*2D + 2D]       partial (dWl | dbl) */
} odin_neck_args;
/* Weight-gradient calls (odin_conv2d_wgrad / odin_deconv2d_wgrad / odin_dense_wgrad / odin_dense_bwd with want_dx = 0)
 * issued between _begin and _end on ONE stream are declared independent of one another by the caller: where two of
 * them land on the small-layer implicit-GEMM kernels they share a launch (results bit-identical to the separate
 * launches).  _end issues a call that found no partner.  Used behind odin_neck_bwd for conv3's and the projection's
 * weight gradients. */
void odin_wgrad_pair_begin(void);
int odin_wgrad_pair_end(void);
int odin_neck_rows(int B, int P, int D, int C0);
int odin_neck_fwd(const odin_neck_args* a, void* stream);
int odin_neck_bwd(const odin_neck_args* a, void* stream);
/* odin_neck_bwd whose launch also executes a part of the step's slab reduction, on the CUs the neck's workgroups (one
 * per CU on half of the chip, latency bound) leave idle.  jobs / n_jobs / g / g_n / part: the WHOLE job list of the step,
 * as the step's odin_slab_reduce_sumsq would be given it (at most 64 jobs); early_mask (bit j = job j): the jobs whose
 * slabs are complete before this launch.  ONE plan is made over all jobs, exactly odin_slab_reduce_sumsq's (grid width,
 * every job's slice of the norm partials); n_reducers extra workgroups (< 0:
 * odin_neck_reduce_workgroups' count) execute the early jobs of it -- same code, same rows, same order, partials at the same
 * indices -- and odin_slab_reduce_sumsq_masked(jobs, n_jobs, early_mask, ...) executes the others and stages the hyper
 * row.  Together bit-identical to odin_neck_bwd + odin_slab_reduce_sumsq.  Of a job outside early_mask only dst, n,
 * stride and the alignment of src are read here.  No workgroup waits for another; a reducing workgroup touches none of
 * the neck's tensors.  part == NULL: dry run, nothing is launched (the count: odin_slab_reduce_sumsq_masked's dry run).
 * early_mask == 0: odin_neck_bwd's launch.  -2, nothing launched: more than 64 jobs, a mask beyond the list, an early
 * job whose dst lies outside [g, g + g_n) -- the range-word reset among them --, n_reducers < 0 where
 * odin_neck_reduce_workgroups gives 0.
 * odin_neck_reduce_workgroups: the reducers the launch takes by itself -- one per four virtual blocks of the early jobs,
 * so that each walks one step (the measured regime) -- if the neck's own workgroups (one per CU) leave that many CUs
 * free; else 0, as for arguments the launch rejects: the caller keeps odin_neck_bwd and the plain reduction (on 256 CUs
 * with the dSprites decoder: from B = 286 on). */
int odin_neck_reduce_workgroups(const odin_neck_args* a, const odin_reduce_job* jobs, int n_jobs, uint64_t early_mask,
                                const float* g, size_t g_n);
int odin_neck_bwd_reduce(const odin_neck_args* a, const odin_reduce_job* jobs, int n_jobs, uint64_t early_mask,
                         const float* g, size_t g_n, float* part, int n_reducers, void* stream);

/* ---- the discriminator's head with its loss in ONE launch (round 6; thin_dense.hip): Dense(K -> 1) on h [B, K]
 * (factor_discriminator.py:60-95: the last layer of FactorDiscriminator), the mean it feeds, and the layer's backward:
 *   logit[b] = h[b, :] . w + bias
 *   mode 0 (total_correlation, factor_discriminator.py:169-198): out[0] = mean_b logit[b]; dlogit[b] = dlogit_in[b]
 *   mode 1 (dtc_loss, :200-235; rows [0, B/2) = D(z), [B/2, B) = D(permute_dims(z'))):
 *          out[0] = 0.5 (mean softplus(-logit_z) + mean softplus(logit_perm)); dlogit its gradient (-> dlogit_out, optional)
 *   dh[b, k] = dlogit[b] w[k] act'(h[b, k]) with aux_act the activation that produced h (dh == NULL: forward + loss only);
 *   max |dh| is folded into dh_amax (optional); wslab (optional, with dh): odin_disc_head_rows(B, K) rows of [K + 1]:
 *   partial (dW | db), to be summed by odin_slab_reduce.
 * workspace: 16 bytes, 8-byte aligned, zero before the FIRST launch (every launch leaves it zero): the workgroups' loss
 * sums meet there as 64-bit fixed-point numbers (integer addition: independent of the order of arrival, bit reproducible).
 * Replaces odin_dense_fwd + odin_mean / odin_dtc_loss_fwd_bwd + odin_dense_bwd of that layer: same values to fp32 rounding. */
int odin_disc_head_rows(int B, int K);
int odin_disc_head_fwd_bwd(const float* h, const float* w, const float* bias, float* logit, int mode,
                           const float* dlogit_in, float* dlogit_out, float* out, int aux_act, float* dh,
                           uint32_t* dh_amax, float* wslab, int* rows_out, void* workspace, int B, int K, void* stream);

/* ---- observation log-likelihood fused forward+backward
 * Independent(Bernoulli(logits),3).log_prob(x) (image_networks.py:87-93;
 * variational_autoencoder.py:528-530): llk_part[b][part] partial sums (n_part per
 * sample), dlogits = -(x - sigmoid(l)) * scale[0]  (scale = DEVICE scalar 1/B).
 * A NULL logits pointer is a dry run that only reports n_part. */
int odin_elbo_bernoulli_fwd_bwd(const float* logits, const float* x, float* llk_part,
                                float* dlogits, const float* scale, int B, int n_per_sample,
                                int* n_part_out, void* stream);
/* The same, and dlogits_amax (optional) receives max |dlogits| -- the range word of the decoder's top gradient.  The
 * a-priori bound 1 / B holds only for targets in [0, 1]; the reference's Bernoulli takes any real target. */
int odin_elbo_bernoulli_fwd_bwd_ranged(const float* logits, const float* x, float* llk_part,
                                       float* dlogits, const float* scale, int B, int n_per_sample,
                                       int* n_part_out, uint32_t* dlogits_amax, void* stream);
/* Independent(ContinuousBernoulli(logits),3).log_prob(x) ('cbernoulli', odin/bay/distribution_alias.py:108;
 * ContinuousBernoulliLayer, odin/bay/layers/discrete.py:82-121; elbo_cbernoulli.hip) for targets x in [0, 1], in logit
 * space: log p = x l - A(l), A(l) = log((e^l - 1) / l), A(0) = 0; dlogits = -(x - mu(l)) * scale[0] with mu = A' the
 * distribution's mean, so |dlogits| <= scale[0].  The five-term series below |l| = 1, the closed forms above (one exp,
 * one log, one reciprocal per element); the reference's `lims` band around probs = 1/2 has no counterpart here.
 * Contract of odin_elbo_bernoulli_fwd_bwd_ranged: llk_part[b][part], a NULL logits pointer is a dry run that reports
 * n_part, dlogits_amax (optional) receives max |dlogits|, fixed-order reductions (equal bits on every launch).
 * n_part depends on the shape alone: n_per_sample / 256 where n_per_sample % 256 == 0 and B * n_per_sample >= 2^20 --
 * served by a persistent grid-stride kernel when the three pointers are 16-byte aligned -- and ceil(n_per_sample / 1024)
 * otherwise (16-byte accesses where n_per_sample % 4 == 0 and the pointers are aligned, scalar ones otherwise).
 * -2, nothing launched, no output touched: B < 1, n_per_sample < 1 or > 2^30, more than 2^31 - 1 partials. */
int odin_elbo_cbernoulli_fwd_bwd(const float* logits, const float* x, float* llk_part, float* dlogits,
                                 const float* scale, int B, int n_per_sample, int* n_part_out,
                                 uint32_t* dlogits_amax, void* stream);
/* The count observations of the gene-expression stacks (elbo_counts.hip):
 * Independent(NegativeBinomial(total_count = exp(a), logits = l), 1).log_prob(x) ('nb'; NegativeBinomialLayer with
 * dispersion 'full', odin/bay/layers/count_layers.py:75-163) and, with zero_inflated = 1, its zero-inflated form ('zinb';
 * ZINegativeBinomialLayer, :311-416; odin/bay/distributions/zero_inflated.py:216-230).  params [B, P G], P = 2 +
 * zero_inflated, holds PLANES of G floats per sample, (a | l) or (a | l | pi) = split(params, P, axis=-1), pi the
 * inflation logit; x [B, G] the counts.  Per element, with r = e^a:
 *   llk = lgamma(r + x) - lgamma(r) - lgamma(1 + x) - r softplus(l) - x softplus(-l)
 *   zinb: t1 = llk - pi, t2 = softplus(-pi); log p = t1 - t2 where x > 1e-8, softplus(t1) - t2 otherwise
 * dparams [B, P G] = -scale[0] * d log p / d params, the same planes.  lgamma(r + x) - lgamma(r) and psi(r + x) -
 * psi(r) are formed as differences (exactly 0 at x = 0), in float64 inside the element.
 * Contract of odin_elbo_cbernoulli_fwd_bwd: llk_part[b][part] in the layout odin_elbo_finalize / odin_sum_parts read,
 * n_part = ceil(G / 256) (the shape alone), a NULL params pointer is a dry run that reports n_part, dparams_amax
 * (optional) receives max |dparams| -- NOT bounded by scale[0] here -- fixed-order reductions (equal bits on every
 * launch), every output written once.
 * Domain: |a| <= 30 is tested and nothing is promised beyond a = 80.  Inside the float64 element nothing overflows
 * there (e^a does near a = 709); what does is the float32 OUTPUT: past a = 88 r = e^a exceeds the float32 range, and with
 * it r softplus(l) and r sigmoid(l) unless l is correspondingly negative -- where the reference's float32 e^a overflows
 * itself.  x >= 0 need not be an integer.
 * -2, nothing launched, no output touched: B < 1, G < 1 or > 2^28, zero_inflated outside {0, 1}, more than 2^31 - 1
 * partials. */
int odin_elbo_nb_fwd_bwd(const float* params, const float* x, float* llk_part, float* dparams, const float* scale,
                         int B, int G, int zero_inflated, int* n_part_out, uint32_t* dparams_amax, void* stream);
/* LogNorm (odin/networks/image_networks.py:138-151), the encoder's first layer of the gene-expression stacks:
 * y[b, g] = log1p(1e4 x[b, g] / (sum_g x[b, g] + 1e-8)), one workgroup per row, the row total summed in float64 in a
 * fixed order, the argument scaled in float64 and the logarithm taken in float32; a row of zeros gives zeros.  No
 * parameters, no gradient.  y_amax (optional) receives max |y|, the activation range word of y.  -2: B < 1, G < 1 or
 * G > 2^28. */
int odin_lognorm_fwd(const float* x, float* y, int B, int G, uint32_t* y_amax, void* stream);
/* Independent(Normal(loc, scale)) with params = split(h,2,axis=-1)
 * (image_networks.py:95-102): softplus1 = 1 -> scale = softplus(raw + softplus^-1(1))
 * (GaussianLayer, odin/bay/layers/continuous.py:196-260; odin/backend/maths.py:279-281);
 * softplus1 = 2 -> the same (loc | raw) split parameterises
 * QuantizedLogistic(loc, softplus(raw) + e^-7, low=0, high=255, inputs_domain='sigmoid')
 * (image_networks.py:55-71; odin/bay/distributions/quantized.py:50-204): x in [0,1], pixel value
 * y = x*255, log P[Y = y] of the discretised logistic, gradients wrt loc and raw.
 * A NULL h is a dry run that only reports n_part (partials per sample). */
int odin_elbo_gaussian_fwd_bwd(const float* h, const float* x, float* llk_part, float* dh,
                               const float* scale, int B, int n_pix, int C, int softplus1,
                               int* n_part_out, void* stream);
/* The Gaussian head in one pass: Conv2D 1x1 (Cin -> 2C maps, linear; image_networks.py:505-511) ->
 * Independent(Normal(loc, scale)).log_prob(target) (:95-102; softplus1 as above, 0 or 1) forward + backward
 * (examples/vae/vae_audio.py:84-110: the audio VAE's decoder).  h [B*n_pix, Cin] = the activation below the head
 * (activation h_act already applied), w1 [Cin, 2C], b1 [2C], target [B, n_pix, C].  Writes logits [B, n_pix, 2C],
 * dlogits (optional) = -scale * d llk / d logits, dh [B*n_pix, Cin] = (dlogits w1^T) * act'(h), llk_part
 * [B][n_part] (the layout odin_elbo_finalize sums), one row (dW1 | db1) per workgroup of wslab and (optional) one
 * row of Cin column sums of dh per workgroup of colsum_slab (the bias gradient of a Conv2DTranspose below);
 * dh_amax (optional): the range word of dh.  Replaces odin_conv2d_fwd + odin_elbo_gaussian_fwd_bwd +
 * odin_conv2d_wgrad + odin_conv2d_dgrad of that layer (three passes over h) with one.  Cin in {8, 16, 32},
 * C in {1, 3}; a NULL h is a dry run that reports n_part / rows; -2: shapes outside the kernel.
 * softplus1 = 3: the Bernoulli observation instead (image_networks.py:87-93): w1 [Cin, C], logits [B, n_pix, C],
 * llk = Independent(Bernoulli(logits)).log_prob(target) -- a Bernoulli decoder whose last two layers do not fit
 * odin_bernoulli_tail_fwd_bwd's plane kernel (5x5 kernels, rows that are not 8 / 16 / 32 pixels wide).
 * softplus1 = 4: the continuous Bernoulli (odin_elbo_cbernoulli_fwd_bwd's log-prob and gradient) over the same C maps:
 * mode 3 with another element function, every 'cbernoulli' decoder that ends in a 1x1 head. */
/* Between _begin and _end the calling thread's weight gradients of the 4x4 / stride-2 plane layers are collected
 * instead of launched, and _end issues them as ONE multi-layer launch on the stream they were given (they depend on
 * nothing but their own layer's tensors; a backward pass has five of them: -4 launches).  odin_slab_reduce issues
 * whatever is still pending first, so a caller that never calls _end stays correct.  Results are bit-identical to
 * the separate launches.  (Measured on the VAE step: slower than launching each weight gradient right behind the data
 * gradient that produced its dy, which then still sits in the Infinity Cache -- odin_ai_amd/engine.py keeps it off.) */
void odin_wgrad_planes_defer_begin(void);
int odin_wgrad_planes_defer_end(void* stream);
/* tests / diagnostics: the launch size (FLOP) from which the convolutions that fit no plane kernel run on the
 * two-plane implicit GEMM (igemm_h.hip) rather than the fp32 one; 0 = every applicable shape, < 0 = only report.
 * Returns the previous value. */
double odin_debug_igemm_h_min_flop(double flop);
/* block-window plane kernels (blk_planes.hip): the launch size from which they take a 4x4 / stride-2 layer (tests: 0), and
 * a switch (0: off, 1: on, < 0: query) for A/B runs; both return the previous value */
double odin_debug_blk_min_flop(double flop);
int odin_debug_blk_planes(int enable);
/* diagnostics: 1 = the block-window kernels also take the layers the row-window plane kernels serve (A/B runs) */
int odin_debug_blk_first(int on);
/* tests / diagnostics: the number of 64 x 64 tiles from which a Dense weight gradient with both widths >= 256 runs on the
 * LDS-staged kernel (dense_h.hip: dense_hw; default 128; tests: 1; a huge value switches it off for A/B runs); < 0 = only
 * report.  Returns the previous value. */
int odin_debug_dense_hw_min_tiles(int tiles);

/* ---- fused Gaussian tail of the TRAINING step (blk_planes.hip): Conv2DTranspose(k4, s2, 32 -> 32, activation d->act) ->
 * Conv2D 1x1 linear with 2 maps (w1 [32, 2], b1 [2]: loc | raw scale) -> Independent(Normal(loc, raw | softplus1(raw)))
 * .log_prob(target [B, OH, OW, 1]), forward AND backward in one launch, any image size: logits [B, OH, OW, 2] (optional
 * out), g_out = dL/d(pre-activation of the layer) for L = -scale[0] * sum llk, llk_part[b][part] (n_part per sample),
 * tail_slab[g][32 * 2 (dW1) | 2 (db1) | 32 (db of the layer)], g < *slab_rows_out; d->x_amax (optional) / d->dy_amax
 * (optional: receives max |g_out|) as in odin_bernoulli_tail_fwd_bwd.  Replaces decoder4 -> decoder6 ->
 * RVconf(..., 'gaus', projection=False) of the audio VAE (examples/vae/vae_audio.py:84-110; image_networks.py:505-511)
 * + px.log_prob(x) + their tape.gradient.  softplus1: 0 = raw scale, 1 = softplus1.  g_out == NULL = dry run;
 * -2: shapes outside the kernel (odin_gaussian_tail_applicable: C == 1, 32 -> 32 channels, k4 s2). */
int odin_gaussian_tail_applicable(const odin_conv_desc* d, int C);
int odin_gaussian_tail_fwd_bwd(const float* x, const float* w, const float* bias, const float* w1, const float* b1,
                               const float* target, float* logits, float* g_out, float* llk_part, int* n_part_out,
                               float* tail_slab, int* slab_rows_out, const float* scale, const odin_conv_desc* d, int C,
                               int softplus1, void* stream);
int odin_gaussian_head_fwd_bwd(const float* h, const float* w1, const float* b1, const float* target,
                               float* logits, float* dlogits, float* dh, float* llk_part, int* n_part_out,
                               float* wslab, int* rows_out, float* colsum_slab, const float* scale, int B,
                               int n_pix, int Cin, int C, int softplus1, int h_act, uint32_t* dh_amax,
                               void* stream);
/* MixtureQuantizedLogistic(params, n_components=K, n_channels=C, low=0, high=255,
 * inputs_domain='sigmoid') (odin/bay/distributions/quantized.py:206-349; built by
 * _parse_distribution 'mixqlogistic', image_networks.py:72-85): h [B, n_pix, K*n_out] with
 * n_out = 1 + 2C + C(C-1)/2 (mixture logit | loc | raw scale | channel coefficients per component),
 * scale = softplus(raw) + e^-7 (:280-282); llk partials per sample, dh = -scale * d log p / d h.
 * C in {1, 3}, K = 10.  A NULL h is a dry run that only reports n_part. */
int odin_elbo_mixqlogistic_fwd_bwd(const float* h, const float* x, float* llk_part, float* dh,
                                   const float* scale, int B, int n_pix, int C, int K,
                                   int* n_part_out, void* stream);
/* VAEStep.call / VariationalModel.elbo (variational_autoencoder.py:117-126;
 * odin/bay/vi/_base.py:151-194): llk[b] = sum parts; elbo = llk - beta*kl - tc;
 * out[0]=loss=-mean(elbo), out[1]=mean llk, out[2]=mean beta*kl, out[3]=tc term.
 * hyper: DEVICE floats {beta, tc_coef}; tc: optional DEVICE scalar (total correlation or
 * mean discriminator logit), tc term = tc_coef*tc[0] (beta_vae.py:123-129,
 * factor_vae.py:211-228). */
int odin_elbo_finalize(const float* llk_part, int n_part, const float* kl, const float* hyper,
                       const float* tc, float* llk, float* out4, int B, void* stream);
/* out[0] = mean(x[0..n)) (deterministic single-workgroup tree) */
int odin_mean(const float* x, int n, float* out, void* stream);

/* ---- beta-TCVAE total correlation (odin/bay/vi/losses.py:101-157), never materialising
 * the [B,B,D] tensor.  tc_out[0] = TC; grads scaled by coef[0] (DEVICE scalar (beta-1)).
 * tc_out is also the workspace: odin_total_correlation_workspace(B_local, B_global, D) floats
 * (B_local = B_global = B for the single-device form). */
int odin_total_correlation_workspace(int B_local, int B_global, int D);
int odin_total_correlation_fwd_bwd(const float* z, const float* p, float* tc_out, float* dz,
                                   float* dloc, float* dscale, const float* coef, int B, int D,
                                   void* stream);
/* The same estimator with the batch sharded over ranks (losses.py:136-157 couples every
 * pair (j, i) of the GLOBAL batch): this rank evaluates its own rows j (z_local [B_local, D])
 * against ALL posteriors i (p_global [B_global, 2D], all-gathered): tc_out[0] = this rank's share
 * sum_j(...) / B_global (sum the shares of the ranks), dz_local [B_local, D] is complete, and
 * dloc_part / dscale_part [B_global, D] hold this rank's partial sums over its j for EVERY
 * posterior i (reduce-scatter them).  tc_out: odin_total_correlation_workspace(B_local, B_global, D) floats. */
int odin_total_correlation_shard(const float* z_local, const float* p_global, float* tc_out,
                                 float* dz_local, float* dloc_part, float* dscale_part,
                                 const float* coef, int B_local, int B_global, int D, void* stream);
/* ---- InfoVAE's maximum-mean discrepancy (odin/bay/vi/losses.py:163-276 with q_sample_shape=None: the forward's
 * sample x = z [N, D] against M prior samples y ~ N(0, I); info_vae.py:28-91) -- forward and backward in ONE launch.
 * Biased estimator over all pairs, diagonal included: MMD = mean k(x,x) + mean k(y,y) - 2 mean k(x,y);
 * kernel 0 = gaussian (k = exp(-|a-b|^2 / D), gaussian_kernel with sigma=None), 1 = linear (k = |sum_d (a_d - b_d)|,
 * linear_kernel; its gradient takes sign(0) = 0).  ws[0] = coef[0] * MMD, dz = coef_grad[0] * dMMD/dx (k(y,y) enters
 * the value only); coef / coef_grad: DEVICE scalars or NULL (1); dz NULL: forward only.  y NULL: drawn inside the
 * launch as elements [0, M*D) of the stream odin_rng_normal(prior_seed, step_dev) writes -- bit for bit.  Cross-row
 * sums in float64 in a fixed order, the workgroups' shares as 64-bit fixed-point words: bit-reproducible, no float
 * atomics.  N <= 4096, D <= 64, M <= 512.  ws: odin_mmd_workspace(...) floats, 8-byte aligned, zeroed ONCE (every
 * launch leaves it zeroed again). */
int odin_mmd_workspace(int B_local, int B_global, int M, int D);
int odin_mmd_fwd_bwd(const float* x, const float* y, float* ws, float* dz, const float* coef,
                     const float* coef_grad, int N, int M, int D, int kernel, uint64_t prior_seed,
                     const int32_t* step_dev, void* stream);
/* The same with the rows sharded over ranks: this rank's rows x_local [B_local, D] against the all-gathered
 * x_all [B_global, D] and y.  dz_local is complete (d/dx_i needs only x_i, every x_j and y); ws[0] = this rank's
 * share of the value (sum the shares: all-reduce); include_yy: 1 on exactly one rank (the k(y,y) term).  y must be
 * the same on every rank: prior_seed must not depend on the rank. */
int odin_mmd_shard(const float* x_local, const float* x_all, const float* y, float* ws, float* dz_local,
                   const float* coef, const float* coef_grad, int B_local, int B_global, int M, int D,
                   int kernel, int include_yy, uint64_t prior_seed, const int32_t* step_dev, void* stream);
/* ---- DIPVAE's disentangled-inferred-prior penalty (odin/bay/vi/losses.py:39-98; dip_vae.py) on p [N, 2D]:
 * loc = p[:, :D], scale = softplus(p[:, D:]).  Cov = centred biased covariance of loc over the N rows
 * (+ diag(mean scale^2) for type II, type2 = 1: only_mean=False); value = lambda_offdiag * sum_{k!=l} Cov_kl^2 +
 * lambda_diag * sum_k (Cov_kk - 1)^2.  ws[0] = coef[0] * value; with G = dvalue/dCov: dloc_i = coef_grad[0] *
 * (2/N) G (loc_i - mean), dscale_ik = coef_grad[0] * G_kk * 2 scale_ik / N (zeros for type I); dloc / dscale NULL:
 * not written.  ONE launch (one workgroup: float64 sums in a fixed order).  D <= 64.
 * ws: odin_dip_workspace(world, D) floats. */
int odin_dip_workspace(int world, int D);
int odin_dip_fwd_bwd(const float* p, float* ws, float* dloc, float* dscale, const float* coef,
                     const float* coef_grad, int N, int D, int type2, float lambda_diag, float lambda_offdiag,
                     void* stream);
/* Data parallel: odin_dip_moments writes this rank's moment block [n | mean[D] | centred M2[D][D] | sum scale^2 [D]]
 * (1 + 2D + D*D floats; ws + 4 of the workspace); the blocks of all ranks are all-gathered (rank order) and
 * odin_dip_finish combines them in rank order (Chan et al.'s pairwise update: no raw E[mu mu^T] - E[mu]E[mu]^T
 * cancellation), writes ws[0] = coef[0] * value -- the whole batch's, the same on every rank -- and this rank's
 * dloc / dscale. */
int odin_dip_moments(const float* p_local, float* block, int B_local, int D, void* stream);
int odin_dip_finish(const float* blocks, int world, const float* p_local, float* ws, float* dloc,
                    float* dscale, const float* coef, const float* coef_grad, int B_local, int D, int type2,
                    float lambda_diag, float lambda_offdiag, void* stream);
/* ---- VampriorVAE's prior (odin/bay/vi/autoencoder/vamprior.py:25-107): the uniform mixture of the K posteriors
 * q(z | u_k) = N(loc_k, softplus(raw_k)), pu [K, 2D] = (loc | raw), as a correction to the standard-normal KL:
 *   c[b] = log N(z_b; 0, I) - ( logsumexp_k sum_d log N(z_bd; loc_kd, sigma_kd) - log K )      (kl_vamp = kl_std + c)
 * ws[0] = coef[0] * mean_b c[b]; dz [B, D] = coef_grad[0] * d(sum_b c_b)/dz, dpu [K, 2D] = coef_grad[0] *
 * d(sum_b c_b)/d(loc | raw) (through softplus); coef / coef_grad: DEVICE scalars or NULL (1); dz and dpu both NULL:
 * forward only (the same c and ws[0] bit for bit).  Three launches inside the call (component table | rows | components);
 * the row maximum is subtracted, sums over k and over b run in float64 in a fixed order inside one workgroup each: no
 * atomics, bit-reproducible; no [B, K] tensor reaches memory beyond lse[B].  B <= 4096, K <= 1024, D <= 64, any values
 * inside.  ws: odin_vamprior_workspace(B, K, D) floats, 8-byte aligned, no initialisation needed. */
int odin_vamprior_workspace(int B, int K, int D);
int odin_vamprior_fwd_bwd(const float* z, const float* pu, float* ws, float* c, float* dz, float* dpu,
                          const float* coef, const float* coef_grad, int B, int K, int D, void* stream);
/* u = clip(w, lo, hi) and clip_by_value's gradient in place, g = scale * g * [lo < w < hi] (the pseudo-inputs'
 * hard_probs; scale: a constant factor of the chain between u and the tensor g was taken for, e.g. 2 for CenterAt0) */
int odin_clip_range_fwd(const float* w, float* u, size_t n, float lo, float hi, void* stream);
int odin_clip_range_bwd(const float* w, float* g, size_t n, float lo, float hi, float scale, void* stream);
/* ---- VQVAE's vector quantiser (odin/bay/distributions/vector_quantizer.py, odin/bay/vi/autoencoder/vq_vae.py):
 * codes [N, Cs] against codebook [K, Cs].
 * odin_vq_assign: idx[n] = argmin_k sum_d (c_nd - e_kd)^2 (fp32 sum of squared differences, never the expanded form;
 * ties: the smallest k), z_q = codebook[idx], m_out[0] = mean over all N Cs elements of (c - z_q)^2 (float64, fixed
 * order: one partial per workgroup, then one workgroup), cnt[k] = #{n: idx_n = k} (optional: NULL for a forward-only
 * call, which leaves the same idx, z_q and m bit for bit); zq_amax: range word of z_q (optional).  The codebook is
 * staged in LDS once per workgroup.  ws: odin_vq_workspace(N) floats, 8-byte aligned, no initialisation needed.
 * odin_vq_bwd: dcodes = (dz_q + 2 commitment / (N Cs) (codes - z_q)) * act'(codes) (straight through + commitment
 * term; act: the activation that produced `codes`, 0 = none; dcodes_amax: its range word, optional) and, for the
 * codebook, EITHER dcodebook[k] = 2 / (N Cs) sum_{n: idx_n = k} (e_k - c_n) (trained by gradient) OR the moving
 * averages ema_counts <- decay ema_counts + (1 - decay) cnt, ema_means <- decay ema_means + (1 - decay) sum_k,
 * codebook <- ema_means / (ema_counts + epsilon) written in place (no zero-debias); neither: dcodes only.  One
 * workgroup per code sums its members in float64 in a fixed order.  No float atomics: bit-reproducible.
 * Limits (a negative return code otherwise): N <= 65536, K <= 1024, Cs <= 256, K * Cs * 4 bytes <= 64 KB. */
int odin_vq_workspace(int N);
int odin_vq_assign(const float* codes, const float* codebook, int32_t* idx, float* z_q, float* ws, float* m_out,
                   int32_t* cnt, uint32_t* zq_amax, int N, int K, int Cs, void* stream);
int odin_vq_bwd(const float* codes, const float* z_q, const int32_t* idx, const float* dz_q, float* codebook,
                float* dcodes, float* dcodebook, float* ema_counts, float* ema_means, float commitment, double decay,
                double epsilon, int act, uint32_t* dcodes_amax, int N, int K, int Cs, void* stream);
/* permute_dims (odin/bay/vi/utils.py:233-269): out[i,l] = z[perm[i,l], l]; perm int32 [B,D] */
int odin_permute_dims(const float* z, const int32_t* perm, float* out, int B, int D, void* stream);
/* per-column random permutations generated on device (Philox), perm int32 [B,D] */
int odin_random_perm(int32_t* perm, int B, int D, uint64_t seed, const int32_t* step_dev,
                     void* stream);
/* odin_random_perm followed by odin_permute_dims(z, perm, out) as ONE launch (all rows of z local: one GPU). */
int odin_random_permute_dims(int32_t* perm, const float* z, float* out, int B, int D, uint64_t seed,
                             const int32_t* step_dev, void* stream);
/* dtc_loss (odin/bay/vi/autoencoder/factor_discriminator.py:200-235):
 * out[0] = 0.5*(mean softplus(-lz) + mean softplus(lperm)); grads wrt both logit vectors */
int odin_dtc_loss_fwd_bwd(const float* logit_z, const float* logit_perm, float* out,
                          float* dlogit_z, float* dlogit_perm, int n, void* stream);

/* ---- optimiser: tf.optimizers.Adam created at odin/networks/base_networks.py:85-112,
 * applied at :604 -- Keras form, epsilon outside the bias-corrected sqrt.
 * hyper (DEVICE): {alpha_t = lr*sqrt(1-b2^t)/(1-b1^t), beta1, beta2, eps, grad_scale};
 * gnorm2 (optional DEVICE scalar): if non-NULL and clip>0 the gradient is scaled by
 * clip/max(sqrt(gnorm2),clip) (tf.clip_by_global_norm, base_networks.py:588); if
 * non-finite AND flag is non-NULL the update is skipped (nan_gradients_policy, base_networks.py:519-547)
 * and flag[0] is set to 1; with flag == NULL ('ignore') the update is applied whatever the norm holds. */
int odin_adam_step_flat(float* theta, const float* g, float* m, float* v, size_t n,
                        const float* hyper, const float* gnorm2, float clip, int32_t* flag,
                        void* stream);
/* odin_adam_step_flat (no clip, no NaN guard) whose last small gradient pieces are formed INSIDE the launch (round 6:
 * FactorVAE's discriminator step ended in think_wgrad -> slab_reduce -> adam, two 5 us launch floors in front of the update):
 *   x != NULL     the weight gradient of a thin-K Dense layer (K <= 32): (dW [K][N] | db [N]) = (x^T dy | column sums of dy)
 *                 over B rows, written to g + w_off and applied (w_off and (K + 1) N multiples of 4)
 *   slab != NULL  g[slab_off + i] = sum over slab_rows rows of slab[r * slab_stride + i], i < slab_n (rows ascending),
 *                 written and applied (slab_off a multiple of 4)
 *   zero != NULL  zero_n 32-bit words cleared (the step's range words)
 * Every other parameter is updated from g as odin_adam_step_flat does. */
typedef struct odin_adam_fold {
  const float* x; const float* dy; int B, K, N; size_t w_off;
  const float* slab; int slab_rows; size_t slab_stride, slab_n, slab_off;
  void* zero; int zero_n;
} odin_adam_fold;
int odin_adam_step_fold(float* theta, float* g, float* m, float* v, size_t n, const float* hyper,
                        const odin_adam_fold* fold, void* stream);
/* ---- VariationalAutoencoder.marginal_log_prob (variational_autoencoder.py:396-513):
 * n posterior samples per input from one encoder pass: z[k,b,:] = loc_b + softplus(raw_b)*eps[k,b,:],
 * logq[k,b] = log q(z_kb | x_b), logp[k,b] = log N(z_kb; 0, I)   (p: [B,2D], eps/z: [n,B,D]);
 * odin_logmeanexp_rows: out[b] = logsumexp_k in[k,b] - log n  (tf.reduce_logsumexp(axis=0) - C). */
int odin_latent_sample_logprob(const float* p, const float* eps, float* z, float* logq,
                               float* logp, int n, int B, int D, void* stream);
int odin_logmeanexp_rows(const float* in, float* out, int n, int B, void* stream);
/* out[b] = sum_j llk_part[b*n_part + j]: the per-sample log p(x|z) from the partial sums the
 * fused observation kernels write (Distribution.log_prob, variational_autoencoder.py:530) */
int odin_sum_parts(const float* llk_part, int n_part, float* out, int B, void* stream);

/* ---- gradient policies of Networks.optimize (odin/networks/base_networks.py:549-596), applied
 * to the flat gradient buffer between the backward pass and the Adam launch, in this order:
 *  odin_grad_skip_threshold : `skip_update_threshold` (:549-578) -- if ANY gradient element is
 *      >= threshold (and enable[0] != 0, = `step >= when_skip_update`), every gradient of the
 *      step becomes 0 (the reference forms g - g) and skipped_count[0] += 1; the optimiser still
 *      runs (momentum-only update), exactly like apply_gradients on the zeroed list.
 *      hit: DEVICE int scratch (1 = threshold reached), enable / skipped_count may be NULL.
 *  odin_clip_by_norm_segments : `clipnorm` (:579-583), tf.clip_by_norm per variable; seg_offsets
 *      (DEVICE, n_segments + 1 int64) delimit the variables inside the flat buffer.
 *  odin_clip_by_value : `clipvalue` (:592-596), tf.clip_by_value(g, -c, c).  The reference clips
 *      by global norm BEFORE by value (:584-591): when both are requested pass the DEVICE scalar
 *      gnorm2 = sum g^2 (odin_sumsq_flat) and global_clipnorm, and the kernel first scales g by
 *      global_clipnorm / max(sqrt(gnorm2), global_clipnorm); gnorm2 = NULL: value clip only. */
int odin_grad_skip_threshold(float* g, size_t n, float threshold, const int32_t* enable,
                             int32_t* hit, int32_t* skipped_count, void* stream);
int odin_clip_by_norm_segments(float* g, const int64_t* seg_offsets, int n_segments, float clipnorm,
                               void* stream);
int odin_clip_by_value(float* g, size_t n, float clipvalue, const float* gnorm2,
                       float global_clipnorm, void* stream);

/* out[0] = sum g^2 (deterministic two-stage); workspace >= 1024 floats */
int odin_sumsq_flat(const float* g, size_t n, float* workspace, float* out, void* stream);
/* odin_sumsq_flat + odin_adam_step_flat in two launches instead of three: the Adam launch sums
 * the stage-1 partials itself (same fixed order, bit-identical norm) and writes it to gnorm2_out.
 * workspace: >= 1024 floats. */
int odin_sumsq_adam_flat(float* theta, const float* g, float* m, float* v, size_t n,
                         const float* hyper, float* workspace, float* gnorm2_out, float clip,
                         int32_t* flag, void* stream);

/* The same two launches as the LAST launches of a step whose per-step scalars live in a device ring (round 5: no
 * per-step host copy): `ring` [rows][row_floats] holds the rows of the coming steps (row of step s at s mod rows, rows a
 * power of two), `cur` is the row the step's kernels read (`hyper` and `elbo_hyper` point into it), t = the int32 at
 * cur[t_word].  The stage-1 launch copies hyper[0..4] to `staged` (>= 8 floats), the Adam launch reads them from there
 * and loads ring row (t + 1) mod rows into `cur` for the next step.  llk_part != NULL: the ELBO finalisation rides in
 * the first launch as in odin_sumsq_adam_finalize_flat.  Replaces the reference's per-step evaluation of the optimiser's
 * learning-rate schedule / beta annealing inside Networks.optimize (base_networks.py:549-596, beta_vae.py:97-126). */
int odin_sumsq_adam_ring(float* theta, const float* g, float* m, float* v, size_t n, const float* hyper,
                         float* workspace, float* gnorm2_out, float clip, int32_t* flag, const float* llk_part,
                         int n_part, const float* kl, const float* elbo_hyper, const float* tc, float* llk,
                         float* out4, int B, const float* ring, float* cur, float* staged, int rows, int row_floats,
                         int t_word, void* stream);

/* Round 5: the gradient norm's stage-1 launch rides in the slab reduction.  odin_slab_reduce_sumsq = odin_slab_reduce
 * that also leaves sum(g^2) of what it writes as one partial per active workgroup in part[0 .. *n_parts_out): jobs whose
 * dst lies inside [g, g + g_n) count -- the caller guarantees that they tile the flat gradient exactly once -- others
 * (the range-word reset) do not.  stage_src / stage_dst (optional): stage_n <= 256 floats copied by the same launch
 * (the step's hyper-parameter row: the Adam launch advances `hyper` while it still needs this step's scalars).
 * part == NULL: dry run, only *n_parts_out (static for a given job list: capture-safe).
 * odin_adam_ring_parts: norm from those partials, clip scale, NaN guard, Adam, the ring advance of
 * odin_sumsq_adam_ring and (llk_part != NULL) the ELBO finalisation, in ONE launch; `staged` = the staged row,
 * alpha_off / elbo_off = offsets of Adam's five scalars / of the ELBO weights in it (ring == NULL: no advance).  Together they replace
 * odin_slab_reduce + odin_sumsq_adam_ring (three launches -> two; base_networks.py:584-596). */
int odin_slab_reduce_sumsq(const odin_reduce_job* jobs, int n_jobs, const float* g, size_t g_n, float* part,
                           int* n_parts_out, const float* stage_src, float* stage_dst, int stage_n, void* stream);
/* The same launch without the jobs in skip_mask (bit j = job j; executed by odin_neck_bwd_reduce): same grid width, the
 * other jobs' partials at the indices the whole plan gives them, the skipped jobs' slices of `part` and their
 * destinations untouched, *n_parts_out = the count of the WHOLE list (the same with and without the mask).  At most 64
 * jobs; a skipped job's dst must lie inside [g, g + g_n): -2 otherwise, nothing launched. */
int odin_slab_reduce_sumsq_masked(const odin_reduce_job* jobs, int n_jobs, uint64_t skip_mask, const float* g, size_t g_n,
                                  float* part, int* n_parts_out, const float* stage_src, float* stage_dst, int stage_n,
                                  void* stream);
int odin_adam_ring_parts(float* theta, const float* g, float* m, float* v, size_t n, const float* staged,
                         int alpha_off, int elbo_off, const float* parts, int n_parts, float* gnorm2_out, float clip,
                         int32_t* flag, const float* llk_part, int n_part, const float* kl, const float* tc, float* llk,
                         float* out4, int B, const float* ring, float* cur, int rows, int row_floats, int t_word,
                         void* stream);

/* odin_sumsq_adam_flat whose first launch also finalises the step's ELBO (the arguments of odin_elbo_finalize):
 * one launch less per training step; loss / norm / update bit-identical to the separate calls. */
int odin_sumsq_adam_finalize_flat(float* theta, const float* g, float* m, float* v, size_t n,
                                  const float* hyper, float* workspace, float* gnorm2_out, float clip,
                                  int32_t* flag, const float* llk_part, int n_part, const float* kl,
                                  const float* elbo_hyper, const float* tc, float* llk, float* out4, int B,
                                  void* stream);

/* ---- counter-based RNG (the reference uses TF's Philox via tfd.sample; streams are not
 * reproducible across frameworks, so parity tests pass eps explicitly) ------------------ */
int odin_rng_normal(float* out, size_t n, uint64_t seed, const int32_t* step_dev, void* stream);

/* ---- on-device input pipeline: batch gather from an HBM-resident uint8 dataset
 * [N, n_per] + ImageDataset.normalize (odin/fuel/image_data/_base.py:130-147), replacing the
 * tf.data map/batch of create_dataset (:338-395).  out[b, e] = normalize(premul * data[idx[b], e]);
 * mode 0 'probs': clip(x,0,255)/255 clipped to [1e-6, 1-1e-6]; 1 'tanh': clip(x/255*2-1);
 * 2 'raster': clip(x,0,255); 3: binarised data, premul * x unchanged.  dSprites stores 0/1
 * and uses premul = 255 (fuel/image_data/shapes.py:69-72,80).  n_per % 16 == 0. */
int odin_gather_normalize_u8(const uint8_t* data, const int32_t* idx, float* out, int B, int n_per,
                             float premul, int mode, void* stream);
/* the same for a float32 dataset that is already normalised: out[b, :] = data[idx[b], :]; n_per % 4 == 0.  The
 * batch selection of Networks.fit on an in-memory array (odin/networks/base_networks.py:642-812). */
int odin_gather_rows_f32(const float* data, const int32_t* idx, float* out, int B, int n_per, void* stream);

/* ---- speech front-end: pre-emphasis -> STFT -> |.|^2 -> Slaney mel -> dB
 * (odin/preprocessing/signal.py:955-967,1442-1562,1623-1691,636-680), computed in float64 like
 * the reference, stored as float32.
 * y [B,n_samples] -> out [B,n_frames,n_mels], n_frames = 1 + (n_samples-frame_length)/step;
 * window [frame_length] float64 (already divided by its sum); twiddles [n_fft/2][2] float64 =
 * (cos, -sin)(2 pi k / n_fft); the mel_filters basis [n_mels, n_fft/2+1] as its non-zero band
 * per filter: fb_band [n_mels][3] = {first bin, count, offset into fb_vals}, fb_vals float64;
 * n_fft a power of two in [16, 2048]; top_db < 0 disables the per-utterance floor.
 * log_output: 0 = mel power; 1 = dB (power2db / amplitude_to_DB); 2 = the floored dB mapped to
 * [0, 1] by (dB - max)/top_db + 1 (input scaling for networks without batch normalisation);
 * 3 = ln(mel + 1e-6) (`AudioFeatureLoader(log_mels=True)`, odin/fuel/audio_data.py:222-223).
 * The same launch serves the TF variant (fuel/audio_data.py:17-101,210-270): un-normalised
 * periodic Hann window, preemph = 0, the HTK filterbank of tf.signal.linear_to_mel_weight_matrix. */
int odin_stft_mel_db(const float* y, const double* window, const double* twiddles,
                     const double* fb_vals, const int32_t* fb_band, float* out, int B,
                     int n_samples, int frame_length, int step_length, int n_fft, int n_mels,
                     double preemph, double top_db, int log_output, void* stream);
/* the same, storing only the first n_out_frames frames of every utterance (out [B, n_out_frames, n_mels]; the
 * top_db floor is still taken over all frames): the front-end writes the VAE's [B, T, n_mels, 1] input buffer
 * directly (fuel/audio_data.py:236-260 crops the spectrogram to max_length).  workspace: 8 * B floats or NULL;
 * with a workspace the frame blocks of an utterance are dealt to up to 8 workgroups (one workgroup per
 * utterance leaves most of the chip idle at batch 256) and the top_db floor follows in a second launch. */
int odin_stft_mel_db_frames(const float* y, const double* window, const double* twiddles,
                            const double* fb_vals, const int32_t* fb_band, float* out, int B, int n_samples,
                            int frame_length, int step_length, int n_fft, int n_mels, double preemph,
                            double top_db, int log_output, int n_out_frames, float* workspace, void* stream);

/* ---- data parallel (the reference has no distributed path) --------------------
 * Thin RCCL entry points: one process per GPU, every collective is enqueued on the caller's stream.
 * The 128-byte id of rank 0 (odin_comm_unique_id = ncclGetUniqueId) is handed to the other ranks by the
 * launcher (odin_ai_amd/dist.py broadcasts it through the torch.distributed store); odin_comm_init =
 * ncclCommInitRank.  RCCL is bound at the first call (dlopen of librccl; ODIN_RCCL_LIB overrides the
 * name): a process that never calls these needs no RCCL.
 *   odin_allreduce_flat      in-place SUM of the flat fp32 gradient bucket (Networks.optimize would apply
 *                            ONE gradient per variable, base_networks.py:415-624: the bucket makes the
 *                            replicas' gradients the global-batch gradient);
 *   odin_allgather_flat      recv[world * n] <- every rank's send[n] ([B, 3D] posterior rows for
 *                            total_correlation over the global batch, losses.py:136-157; z' rows for
 *                            permute_dims, vi/utils.py:262-267);
 *   odin_reduce_scatter_flat recv[n] <- sum over ranks of send[rank * n ...] (posterior-side TC gradients). */
int odin_comm_unique_id(void* id128);
int odin_comm_init(void** comm_out, const void* id128, int rank, int world_size);
int odin_comm_destroy(void* comm);
/* the RCCL library bound by this process: ODIN_RCCL_LIB, else the librccl the process has already mapped (the one
 * PyTorch bundles -- never a second copy), else the system one; "" before the first odin_comm_* call */
const char* odin_comm_library(void);
int odin_allreduce_flat(void* comm, float* buf, size_t n, void* stream);
int odin_allgather_flat(void* comm, const float* send, float* recv, size_t n_per_rank, void* stream);
int odin_reduce_scatter_flat(void* comm, const float* send, float* recv, size_t n_per_rank, void* stream);

/* diagnostics only: device buffer (>= 64 int64) that receives in-kernel cycle stamps of the
 * conv kernels' workgroup 0 (NULL disables; never set in production) */
int odin_debug_set_stamps(void* buf);
int odin_debug_set_wgrad_stamps(void* buf);
/* diagnostics: workgroup 0 of odin_neck_fwd / _bwd records 100 MHz wall-clock stamps at its phase boundaries into
 * buf[0..6] / buf[8..17] (int64, device memory); NULL: off */
int odin_debug_set_neck_stamps(void* buf);
/* diagnostics: launch shape of the persistent Bernoulli ELBO kernel (workgroups, chunks in flight per wave, 1 = the
 * software-pipelined body); a non-positive / negative field keeps its value (tools/elbo_sweep6.py) */
int odin_debug_elbo_shape(int blocks, int U, int pipelined);
/* diagnostics: workgroup (0, 0) of odin_stft_mel_db_frames records 100 MHz wall-clock stamps (per pass: start, staged,
 * FFT done, power spectrum done; then the end of its last pass) into buf (int64, device memory, >= 64 entries); NULL: off */
int odin_debug_set_mel_stamps(void* buf);
/* tests / A-B runs: 0 = n_fft 512 on the general front-end kernel instead of the register radix-16 one (mel.hip); < 0 = only
 * report.  Returns the previous value. */
int odin_debug_mel_r16(int enable);
/* tests / A-B runs: 0 = the RGB first layer's forward (4x4, 3 -> 32 channels) on the fp32 matrix instructions instead of two
 * f16 planes (smallc_conv.hip); < 0 = only report.  Returns the previous value. */
int odin_debug_smallc_planes(int enable);
/* diagnostics: the largest weight slice igemm_h keeps in LDS, in 16-value steps of 2 KB (default 32 = 64 KB; 64 measured slower);
 * returns the previous value, a negative argument only reads it */
int odin_debug_igemm_h_ldsw_steps(int steps);

/* ---- TwoStageVAE's skip heads (stage2.hip; odin/bay/vi/autoencoder/two_stage_vae.py, odin/bay/layers/latents.py:23-45):
 * Dense over Concatenate([x, h]) without the concatenated tensor,
 *   p [B, N] = x [B, Dx] w[:Dx] + h [B, H] w[Dx:] + bias,   w [(Dx + H), N] row-major (a Dense kernel).
 * mode 0: p only (`Latents2`: odin_latent_fwd follows).
 * mode 1 (`Observation2` as a likelihood): N = 2 E, target t [B, E]; the same launch also writes
 *   llk[b] = sum_e log N(t[b, e]; p[b, e], softplus(p[b, E + e]))   and   dp [B, 2 E] = -scale[0] * d llk / d p
 *   (scale a DEVICE scalar; softplus and its derivative are finite for raw values in [-80, 80]).
 * Limits: B >= 1, 1 <= Dx <= 128, N even with 1 <= N / 2 <= 128, H a multiple of 4 in [4, 4096]; anything else returns
 * -2.  bias may be NULL.  Every sum runs in a fixed order (no float atomics): two calls give the same bits. */
int odin_skip_head_fwd(const float* x, const float* h, const float* w, const float* bias, float* p, int mode,
                       const float* target, const float* scale, float* llk, float* dp, int B, int Dx, int H, int N,
                       void* stream);
/* From dp [B, N]:  dh [B, H] = (dp w[Dx:]^T) * act'(h) with h the activation's OUTPUT (h_act: 0 linear, 1 elu, 2 relu),
 * max |dh| folded into dh_amax (a range word, optional);  dx [B, Dx] = dp w[:Dx]^T (optional: NULL where x is data);
 * slab[g][(Dx + H) N | N]: per-workgroup partial (dW | db), to be summed by odin_slab_reduce -- *slab_rows_out rows, at
 * most 32.  slab == NULL = dry run (the row count only).  Limits and the fixed summation order as odin_skip_head_fwd. */
int odin_skip_head_bwd(const float* x, const float* h, const float* w, const float* dp, int h_act, float* dh,
                       uint32_t* dh_amax, float* dx, float* slab, int* slab_rows_out, int B, int Dx, int H, int N,
                       void* stream);

/* ---- the semi-supervised label head of MultitaskVAE / SkiptaskVAE (label_head.hip; odin/bay/vi/autoencoder/
 * multitask_vae.py:164-207): Dense(D -> K) giving the logits of a OneHotCategorical over a FRESH posterior sample, for the
 * labelled rows [row0, row0 + Bs) of p [B, 2 D] = (loc | raw):
 *   z' = loc + softplus(raw) eps_y;   l = z' w + bias   (w [D, K] row-major: a Dense kernel; bias may be NULL)
 *   llk[b] = sum_k y_k (l_k - logsumexp(l))   (the maximum subtracted first; y [Bs, K] float, one-hot or soft)
 *   g_k = y_k - softmax_k sum_j y_j,  dz' = w g,  and with c = coef[0] (a DEVICE scalar: graph replays see the schedule)
 *   dloc [B, D] = c dz',  dscale [B, D] = c dz' eps_y  -- the gradient inputs of odin_latent_bwd, in the convention of
 *   odin_total_correlation_fwd_bwd (dscale is taken with respect to softplus(raw)); every row outside the labelled block
 *   is written as zero on every launch.
 *   value[0] = (1 / Bs) sum_b llk[b];  value[1] is the launch's ticket word: zero before the first launch, left zero.
 *   logits [Bs, K] is optional (NULL).  eps_y [Bs, D], llk [Bs].
 *   slab[g][D K | K]: per-workgroup partial (dW | db) = c (sum_b z'_b g_b^T | sum_b g_b), to be summed by
 *   odin_slab_reduce -- *slab_rows_out rows, at most 32.  slab == NULL = dry run (the row count only).
 * One wave per sample, one launch, no float atomics: every sum, the batch mean included, runs in a fixed order and two
 * calls give the same bits.  Outputs are finite for logits of magnitude 1e4 and raw scales in [-80, 80]; an all-zero row
 * of y gives llk = 0 and zero gradients.
 * Limits: 1 <= D <= 255, 1 <= K <= 255, 1 <= Bs, 0 <= row0, row0 + Bs <= B; anything else, and a call with a slab but a
 * NULL operand, returns -2, launches nothing and touches no output (*slab_rows_out included). */
int odin_label_head_fwd_bwd(const float* p, const float* eps_y, const float* w, const float* bias, const float* y,
                            const float* coef, float* logits, float* llk, float* value, float* dloc, float* dscale,
                            float* slab, int* slab_rows_out, int B, int row0, int Bs, int D, int K, void* stream);
/* The forward half from a given z [n, D]: logits [n, K] = z w + bias, in the summation order of the fused launch
 * (MultitaskVAE.predict_labels).  Limits: 1 <= D, K <= 255, 1 <= n. */
int odin_label_head_fwd(const float* z, const float* w, const float* bias, float* logits, int n, int D, int K,
                        void* stream);

/* ---- HIP-graph helpers (capture a sequence of the calls above, replay per step) ------- */
int odin_graph_begin(void* stream);
int odin_graph_end(void* stream, void** graph_exec_out);
int odin_graph_launch(void* graph_exec, void* stream);
int odin_graph_destroy(void* graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* ODIN_HIP_H */
