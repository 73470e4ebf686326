// latent_binconcrete.hip -- the relaxed Bernoulli (binary Concrete) posterior q(z|x) = RelaxedBernoulli(temperature tau,
// logits l) (odin/bay/layers/discrete.py:346 ff.; RVconf(D, 'relaxedbern' | 'relaxedsigmoid' | 'relaxedbernoulli',
// projection=True), odin/bay/distribution_alias.py:111-112): D INDEPENDENT binary units, the projection emits l [B, D].
//   n ~ Logistic(0, 1);  u = (l + n) / tau;  z = sigmoid(u)   (z lies in (0, 1)^D)
//   log q(z) = sum_d [ log tau - n_d - 2 softplus(-n_d) + softplus(u_d) + softplus(-u_d) ]
//            = D log tau + sum_d [ S(u_d) - S(n_d) ],   S(x) = softplus(x) + softplus(-x) = |x| + 2 log1p(exp(-|x|))
//   log p(z) = -D log 2                                   (Independent(Bernoulli(logits = 0)), random_variable.py:149-154)
//   KL: analytic = 0  log q(z) + D log 2 at that z;  1  sum_d [pi log pi + (1 - pi) log(1 - pi) + log 2], pi = sigmoid(l)
// All arithmetic stays in u: log z and log(1 - z) are never taken, so a z that rounds to exactly 0 or 1 (tau = 0.1:
// |u| reaches 170) costs nothing; z (1 - z) = e / (1 + e)^2 and 2 z - 1 = sign(u) (1 - e) / (1 + e) with e = exp(-|u|).
// The closed-form KL of one unit is t tanh t - log cosh t with t = l / 2.  Near l = 0 (a fresh projection) the textbook
// form is a difference of terms near log 2; it is taken as |t| th + log1p(-th^2) / 2 with th = tanh |t| from expm1 (a
// factor-2 cancellation, no more) below |t| = 1 and as log 2 - log1p(e) - 2 |t| e / (1 + e) above -- both are
// evaluated and one is selected, no branch diverges.
// ONE WAVE per sample, four samples per workgroup, lane k owns units k, k + 64, k + 128, k + 192; the per-sample sums
// meet in a fixed butterfly over the wave.  No LDS, no float atomics; every output element is written exactly once: two
// runs, and eager versus graph replay, give the same bits.
// backward, with w = klw fbmask_b, G = dz + dz_extra:
//   analytic = 0: dl_d = (G_d z_d (1 - z_d) + w (2 z_d - 1)) / tau
//   analytic = 1: dl_d = G_d z_d (1 - z_d) / tau + w pi_d (1 - pi_d) l_d
// The noise: element e of the stream is component e & 3 of Philox counter e >> 2 (odin_rng_normal's scheme); with
// m = bits >> 8,  m < 2^23:  a = (m + 0.5) 2^-24,        n = log a - log1p(-a)
//                 otherwise: c = (2^24 - m - 0.5) 2^-24,  n = log1p(-c) - log c
// (U = (m + 0.5) 2^-24 has no fp32 pattern of its own in the upper half; its complement c does).  |n| <= 25 ln 2 <
// 17.33, and the stream is exactly antisymmetric in m <-> 2^24 - 1 - m.
// Limits (checked in the entries): 1 <= D <= 255, B >= 1, tau > 0, analytic in {0, 1}.
#include <cmath>

#include "odin_device.h"
#include "odin_internal.h"
#include "odin_latent_math.h"

namespace {

constexpr int BINC_NT = 256;
constexpr int BINC_SPW = BINC_NT / 64;   // samples per workgroup: one per wave
constexpr int BINC_DMAX = 255;

// Logistic(0, 1) noise of the 24 high bits m of a Philox word
__device__ __forceinline__ float binc_logistic_of(unsigned bits) {
  const unsigned m = bits >> 8;
  const bool low = m < (1u << 23);
  // (m + 0.5 and 2^24 - m - 0.5 each have 24 significant bits in their own half)
  const float a = ((float)(low ? m : (1u << 24) - 1u - m) + 0.5f) * (1.f / 16777216.f);
  const float v = logf(a) - log1pf(-a);
  return low ? v : -v;
}

// element e of the logistic stream (k0, k1, step)
__device__ __forceinline__ float binc_logistic_at(size_t e, unsigned step, unsigned k0, unsigned k1) {
  const size_t c = e >> 2;
  unsigned r[4];
  philox4x32_10((unsigned)c, (unsigned)(c >> 32), step, 0u, k0, k1, r);
  const unsigned j = (unsigned)e & 3u;
  return binc_logistic_of(j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3]);
}

__global__ __launch_bounds__(256) void rng_logistic_kernel(float* out, size_t n, unsigned k0, unsigned k1,
                                                           const int* step_dev) {
  const unsigned step = step_dev ? (unsigned)step_dev[0] : 0u;
  const size_t n4 = (n + 3) >> 2, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    unsigned r[4];
    philox4x32_10((unsigned)i, (unsigned)(i >> 32), step, 0u, k0, k1, r);
    for (int j = 0; j < 4; ++j)
      if (i * 4 + j < n) out[i * 4 + j] = binc_logistic_of(r[j]);
  }
}

// S(x) = softplus(x) + softplus(-x) from e = exp(-|x|)
__device__ __forceinline__ float binc_s(float ax, float e) { return fmaf(2.f, log1pf(e), ax); }

// one unit: u -> z = sigmoid(u) and S(u)
__device__ __forceinline__ void binc_relax(float u, float& zz, float& su) {
  const float au = fabsf(u), e = expf(-au);
  const float s = 1.f / (1.f + e);
  zz = u >= 0.f ? s : e * s;
  su = binc_s(au, e);
}

// S(n) of the noise
__device__ __forceinline__ float binc_s_of(float x) {
  const float ax = fabsf(x);
  return binc_s(ax, expf(-ax));
}

// KL(Bernoulli(sigmoid(l)) || Bernoulli(1/2)) = t tanh t - log cosh t, t = l / 2 (see the header)
__device__ __forceinline__ float binc_kl_unit(float l) {
  const float at = 0.5f * fabsf(l);
  const float x = -expm1f(-2.f * at);   // 1 - e, exact in its leading digits near l = 0
  const float e = expf(-2.f * at);
  const float th = x / (2.f - x);       // tanh |t| = (1 - e) / (1 + e)
  const float small = fmaf(at, th, 0.5f * log1pf(-th * th));
  const float large = 0.6931471805599453f - log1pf(e) - 2.f * at * e / (1.f + e);
  return at < 1.f ? small : large;
}

// pi (1 - pi) of pi = sigmoid(l)
__device__ __forceinline__ float binc_var(float l) {
  const float e = expf(-fabsf(l));
  const float s = 1.f / (1.f + e);
  return e * s * s;
}

__global__ __launch_bounds__(BINC_NT) void latent_relaxedbern_fwd_kernel(const float* p, float* nz, float* z, float* kl,
                                                                         float* fbmask, int B, int D, float inv_tau,
                                                                         float c0, int analytic, float free_bits,
                                                                         const float* cap, int draw, unsigned k0,
                                                                         unsigned k1, const int* step_dev) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * BINC_SPW + w;
  if (b >= B) return;   // (wave-uniform, and a wave meets only itself below)
  const unsigned step = draw && step_dev ? (unsigned)step_dev[0] : 0u;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) {
    const size_t o = (size_t)b * D + d;
    const float l = p[o];
    float n;
    if (draw) {
      n = binc_logistic_at(o, step, k0, k1);
      nz[o] = n;
    } else {
      n = nz[o];
    }
    float zz, su;
    binc_relax((l + n) * inv_tau, zz, su);
    z[o] = zz;
    acc += analytic ? binc_kl_unit(l) : su - binc_s_of(n);
  }
  acc = wave_sum64(acc);
  if (lane != 0) return;
  if (!analytic) acc += c0;
  float m = 1.f;
  if (free_bits >= 0.f) {
    const float thr = free_bits * (float)D;
    if (!(acc > thr)) { acc = thr; m = 0.f; }
  }
  if (cap != nullptr) {  // BetaCapacityVAE (beta_vae.py:171-177): |kl - C(step)|, gradient sign(kl - C)
    const float d = acc - cap[0];
    m *= d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    acc = fabsf(d);
  }
  kl[b] = acc;
  fbmask[b] = m;
}

// sample (k, b) = blockIdx.x * 4 + wave of n * B: the rows of p repeat over k
__global__ __launch_bounds__(BINC_NT) void latent_relaxedbern_sample_logprob_kernel(const float* p, const float* nz,
                                                                                    float* z, float* logq, float* logp,
                                                                                    int n, int B, int D, float inv_tau,
                                                                                    float c0, float lp0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * BINC_SPW + w;
  if (i >= (size_t)n * B) return;   // (wave-uniform)
  const float* pr = p + (i % (size_t)B) * D;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) {
    const size_t o = i * D + d;
    const float ns = nz[o];
    float zz, su;
    binc_relax((pr[d] + ns) * inv_tau, zz, su);
    z[o] = zz;
    acc += su - binc_s_of(ns);
  }
  acc = wave_sum64(acc);
  if (lane != 0) return;
  logq[i] = c0 + acc;
  logp[i] = lp0;
}

__global__ __launch_bounds__(BINC_NT) void latent_relaxedbern_bwd_kernel(const float* p, const float* nz, const float* dz,
                                                                         const float* dz2, const float* fbmask,
                                                                         const float* klw, float* dp, int B, int D,
                                                                         float inv_tau, int analytic) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * BINC_SPW + w;
  if (b >= B) return;   // (wave-uniform)
  const float wt = klw[0] * fbmask[b];
  for (int d = lane; d < D; d += 64) {
    const size_t o = (size_t)b * D + d;
    const float l = p[o];
    float G = 0.f;
    if (dz != nullptr) G += dz[o];
    if (dz2 != nullptr) G += dz2[o];
    const float u = (l + nz[o]) * inv_tau;
    const float e = expf(-fabsf(u));
    const float s = 1.f / (1.f + e);
    const float v = G * e * s * s * inv_tau;   // G z (1 - z) / tau
    // (2 z - 1 = sign(u) (1 - e) / (1 + e): exact where z itself has rounded to 0 or 1; 1 - e by expm1 near u = 0)
    const float tz = copysignf(-expm1f(-fabsf(u)) * s, u);
    dp[o] = analytic ? fmaf(wt * binc_var(l), l, v) : fmaf(wt * inv_tau, tz, v);
  }
}

int binc_check(const char* who, long long rows, int D, float tau, int analytic) {
  static char msg[128];
  const char* what = nullptr;
  if (D < 1 || D > BINC_DMAX) what = "D outside [1, 255]";
  else if (rows < 1 || rows > 0x7FFFFFF0ll) what = "batch outside [1, 2^31 - 16]";
  else if (!(tau > 0.f) || !std::isfinite(tau)) what = "the temperature must be positive";
  else if (analytic != 0 && analytic != 1) what = "analytic must be 0 (Monte Carlo) or 1 (the Bernoulli KL)";
  if (what == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return odin_fail(-2, msg);
}

}  // namespace

extern "C" int odin_rng_logistic(float* out, size_t n, uint64_t seed, const int32_t* step_dev, void* stream) {
  if (out == nullptr || n == 0) return odin_fail(-2, "rng_logistic: null output or n = 0");
  int grid = (int)std::min<size_t>(((n + 3) / 4 + 255) / 256, 2048);
  ODIN_LAUNCH(rng_logistic_kernel, dim3(grid), dim3(256), 0, stream, out, n, (unsigned)seed, (unsigned)(seed >> 32),
              (const int*)step_dev);
  return odin_check_launch("rng_logistic");
}

extern "C" int odin_latent_relaxedbern_fwd(const float* p, float* n, float* z, float* kl, float* fbmask, int B, int D,
                                           float tau, int analytic, float free_bits, const float* capacity, int draw,
                                           uint64_t seed, const int32_t* step_dev, void* stream) {
  if (int rc = binc_check("latent_relaxedbern_fwd", B, D, tau, analytic)) return rc;
  if (p == nullptr || n == nullptr || z == nullptr || kl == nullptr || fbmask == nullptr)
    return odin_fail(-2, "latent_relaxedbern_fwd: null argument");
  // D (log tau + log 2): the part of the single-sample KL that depends on neither the logits nor the noise
  const float c0 = (float)(D * (std::log((double)tau) + std::log(2.0)));
  ODIN_LAUNCH(latent_relaxedbern_fwd_kernel, dim3((B + BINC_SPW - 1) / BINC_SPW), dim3(BINC_NT), 0, stream, p, n, z, kl,
              fbmask, B, D, 1.f / tau, c0, analytic, free_bits, capacity, draw != 0 ? 1 : 0, (unsigned)seed,
              (unsigned)(seed >> 32), (const int*)step_dev);
  return odin_check_launch("latent_relaxedbern_fwd");
}

extern "C" int odin_latent_relaxedbern_bwd(const float* p, const float* n, const float* z, const float* dz,
                                           const float* dz_extra, const float* fbmask, const float* klw, float* dp, int B,
                                           int D, float tau, int analytic, void* stream) {
  if (int rc = binc_check("latent_relaxedbern_bwd", B, D, tau, analytic)) return rc;
  (void)z;   // (the gradients are formed in u = (l + n) / tau: z has rounded to 0 or 1 where u is large)
  if (p == nullptr || n == nullptr || fbmask == nullptr || klw == nullptr || dp == nullptr)
    return odin_fail(-2, "latent_relaxedbern_bwd: null argument");
  ODIN_LAUNCH(latent_relaxedbern_bwd_kernel, dim3((B + BINC_SPW - 1) / BINC_SPW), dim3(BINC_NT), 0, stream, p, n, dz,
              dz_extra, fbmask, klw, dp, B, D, 1.f / tau, analytic);
  return odin_check_launch("latent_relaxedbern_bwd");
}

extern "C" int odin_latent_relaxedbern_sample_logprob(const float* p, const float* n, float* z, float* logq, float* logp,
                                                      int n_samples, int B, int D, float tau, void* stream) {
  if (n_samples < 1 || B < 1) return odin_fail(-2, "latent_relaxedbern_sample_logprob: n_samples and B must be positive");
  const long long rows = (long long)n_samples * B;
  if (int rc = binc_check("latent_relaxedbern_sample_logprob", rows, D, tau, 0)) return rc;
  if (p == nullptr || n == nullptr || z == nullptr || logq == nullptr || logp == nullptr)
    return odin_fail(-2, "latent_relaxedbern_sample_logprob: null argument");
  ODIN_LAUNCH(latent_relaxedbern_sample_logprob_kernel, dim3((unsigned)((rows + BINC_SPW - 1) / BINC_SPW)),
              dim3(BINC_NT), 0, stream, p, n, z, logq, logp, n_samples, B, D, 1.f / tau,
              (float)(D * std::log((double)tau)), (float)(-D * std::log(2.0)));
  return odin_check_launch("latent_relaxedbern_sample_logprob");
}
