// latent_concrete.hip -- the relaxed one-hot (Concrete / Gumbel-softmax) posterior q(z|x) =
// RelaxedOneHotCategorical(temperature tau, logits l) (odin/bay/layers/discrete.py:286-343; RVconf(K, 'relaxedonehot',
// projection=True), odin/bay/distribution_alias.py:113-114): ONE K-way variable, the projection emits l [B, K].
//   g ~ Gumbel(0, 1);  u = (l + g) / tau;  y = u - logsumexp(u);  z = exp(y)   (z lies on the simplex)
//   log q(z) = lgamma(K) + (K - 1) log tau + sum_k log_softmax(l - tau y)_k - sum_k y_k
//            = lgamma(K) + (K - 1) log tau - sum_k g_k - K logsumexp(-g) - sum_k y_k       (l - tau y = -g + tau lse(u))
//   log p(z) = -log K sum_k z_k                        (OneHotCategorical with equal logits, random_variable.py:141-146)
//   KL: analytic = 0  log q(z) - log p(z) at that z;  1  sum_k pi_k (log pi_k + log K), pi = softmax(l)  (Jang et al.)
// All arithmetic stays in y: log(z) is never taken, so a z that underflows to 0 (tau = 0.1: y < -87) costs nothing.
// ONE WAVE per sample, four samples per workgroup, lane k owns category k; the max, the sums and the log-sum-exp meet in
// a fixed butterfly over the wave.  No LDS, no float atomics; every output element is written exactly once: two runs,
// and eager versus graph replay, give the same bits.
// backward, with w = klw fbmask_b, G = dz + dz_extra, a_j = G_j - sum_k G_k z_k:
//   analytic = 0: dl_j = (z_j a_j - w (1 - K z_j)) / tau       (log p is constant on the simplex)
//   analytic = 1: dl_j = z_j a_j / tau + w pi_j (log pi_j - sum_k pi_k log pi_k)
// The noise: element e of the stream is component e & 3 of Philox counter e >> 2 (odin_rng_normal's scheme) read as
//   U = ((bits >> 8) + 0.5) 2^-24 in (0, 1),  g = -log(-log U)  in [-2.86, 17.33].
// U's upper half has no fp32 pattern of its own ((2^24 - 1) + 0.5 would round to 2^24, U = 1, g = inf): there -log U is
// taken as -log1p(-(1 - U)), whose argument (2^24 - bits - 0.5) 2^-24 is exact.
// Limits (checked in the entries): 2 <= K <= 64 (a category per lane of a wave64), B >= 1, tau > 0, analytic in {0, 1}.
#include <cmath>

#include "odin_device.h"
#include "odin_internal.h"
#include "odin_latent_math.h"

namespace {

constexpr int CONC_NT = 256;
constexpr int CONC_SPW = CONC_NT / 64;   // samples per workgroup: one per wave
constexpr int CONC_KMAX = 64;

__device__ __forceinline__ float conc_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// -log(-log U) of the 24 high bits x of a Philox word, U = (x + 0.5) 2^-24
__device__ __forceinline__ float conc_gumbel_of(unsigned bits) {
  const unsigned x = bits >> 8;
  float t;   // -log U
  if (x < (1u << 23)) t = -logf(((float)x + 0.5f) * (1.f / 16777216.f));          // (x + 0.5 has 24 significant bits)
  else t = -log1pf(-(((float)((1u << 24) - x) - 0.5f) * (1.f / 16777216.f)));     // (so has 2^24 - x - 0.5)
  return -logf(t);
}

// element e of the Gumbel stream (k0, k1, step)
__device__ __forceinline__ float conc_gumbel_at(size_t e, unsigned step, unsigned k0, unsigned k1) {
  const size_t c = e >> 2;
  unsigned r[4];
  philox4x32_10((unsigned)c, (unsigned)(c >> 32), step, 0u, k0, k1, r);
  const unsigned j = (unsigned)e & 3u;
  return conc_gumbel_of(j == 0 ? r[0] : j == 1 ? r[1] : j == 2 ? r[2] : r[3]);
}

__global__ __launch_bounds__(256) void rng_gumbel_kernel(float* out, size_t n, unsigned k0, unsigned k1,
                                                         const int* step_dev) {
  const unsigned step = step_dev ? (unsigned)step_dev[0] : 0u;
  const size_t n4 = (n + 3) >> 2, stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    unsigned r[4];
    philox4x32_10((unsigned)i, (unsigned)(i >> 32), step, 0u, k0, k1, r);
    for (int j = 0; j < 4; ++j)
      if (i * 4 + j < n) out[i * 4 + j] = conc_gumbel_of(r[j]);
  }
}

// the first lane that holds the wave's maximum m of v (as a float: every lane receives it)
__device__ __forceinline__ float conc_wave_argmax(float v, float m, bool on, int lane) {
  float i = on && v == m ? (float)lane : 64.f;
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) i = fminf(i, __shfl_xor(i, x));
  return i;
}

// log_softmax over the lanes that are `on` (lanes >= K carry u = -inf and receive 0).  The largest entry is left out of
// the sum, log(1 + rest) taken by log1p: where one category dominates, its own value -log1p(rest) keeps its relative
// precision instead of drowning in the rounding of log(1 + rest).
__device__ __forceinline__ float conc_log_softmax(float u, bool on, int lane) {
  const float m = conc_wave_max(u);
  const int top = (int)conc_wave_argmax(u, m, on, lane);
  const float rest = wave_sum64(on && lane != top ? expf(u - m) : 0.f);
  return on ? (u - m) - log1pf(rest) : 0.f;
}

// lane `lane` of one sample: u -> y = u - logsumexp(u), z = exp(y); lanes >= K carry u = -inf, y = 0, z = 0
__device__ __forceinline__ void conc_relax(float u, bool on, int lane, float& y, float& zz) {
  y = conc_log_softmax(u, on, lane);
  zz = on ? expf(y) : 0.f;
}

// log q(z) - the constant lgamma(K) + (K - 1) log tau, from the noise and y (every lane receives it)
__device__ __forceinline__ float conc_logq(float g, float y, bool on, int K) {
  const float ng = on ? -g : -INFINITY;
  const float m = conc_wave_max(ng);
  const float s = wave_sum64(on ? expf(ng - m) : 0.f);
  return -wave_sum64(on ? g + y : 0.f) - (float)K * (m + logf(s));
}

__global__ __launch_bounds__(CONC_NT) void latent_concrete_fwd_kernel(const float* p, float* g, float* z, float* kl,
                                                                      float* fbmask, int B, int K, float inv_tau,
                                                                      float c0, int analytic, float free_bits,
                                                                      const float* cap, int draw, unsigned k0,
                                                                      unsigned k1, const int* step_dev) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * CONC_SPW + w;
  if (b >= B) return;   // (wave-uniform, and a wave meets only itself below)
  const bool on = lane < K;
  const size_t o = (size_t)b * K + (on ? lane : 0);
  const float l = on ? p[o] : 0.f;
  float gn = 0.f;
  if (on) {
    if (draw) {
      gn = conc_gumbel_at(o, step_dev ? (unsigned)step_dev[0] : 0u, k0, k1);
      g[o] = gn;
    } else {
      gn = g[o];
    }
  }
  float y, zz;
  conc_relax(on ? (l + gn) * inv_tau : -INFINITY, on, lane, y, zz);
  if (on) z[o] = zz;
  const float logk = logf((float)K);
  float acc;
  if (analytic) {
    const float lp = conc_log_softmax(on ? l : -INFINITY, on, lane);   // log pi
    acc = wave_sum64(on ? expf(lp) * (lp + logk) : 0.f);
  } else {
    acc = c0 + conc_logq(gn, y, on, K) + logk * wave_sum64(zz);
  }
  if (lane != 0) return;
  float m = 1.f;
  if (free_bits >= 0.f) {
    const float thr = free_bits * (float)K;
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
__global__ __launch_bounds__(CONC_NT) void latent_concrete_sample_logprob_kernel(const float* p, const float* g, float* z,
                                                                                 float* logq, float* logp, int n, int B,
                                                                                 int K, float inv_tau, float c0) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * CONC_SPW + w;
  if (i >= (size_t)n * B) return;   // (wave-uniform)
  const bool on = lane < K;
  const size_t o = i * K + (on ? lane : 0);
  const float l = on ? p[(i % (size_t)B) * K + lane] : 0.f;
  const float gn = on ? g[o] : 0.f;
  float y, zz;
  conc_relax(on ? (l + gn) * inv_tau : -INFINITY, on, lane, y, zz);
  if (on) z[o] = zz;
  const float lq = c0 + conc_logq(gn, y, on, K);
  const float lp = -logf((float)K) * wave_sum64(zz);
  if (lane != 0) return;
  logq[i] = lq;
  logp[i] = lp;
}

__global__ __launch_bounds__(CONC_NT) void latent_concrete_bwd_kernel(const float* p, const float* z, const float* dz,
                                                                      const float* dz2, const float* fbmask,
                                                                      const float* klw, float* dp, int B, int K,
                                                                      float inv_tau, int analytic) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * CONC_SPW + w;
  if (b >= B) return;   // (wave-uniform)
  const bool on = lane < K;
  const size_t o = (size_t)b * K + (on ? lane : 0);
  const float wt = klw[0] * fbmask[b];
  float G = 0.f;
  if (on && dz != nullptr) G += dz[o];
  if (on && dz2 != nullptr) G += dz2[o];
  const float zz = on ? z[o] : 0.f;
  // a_j = G_j - sum_k G_k z_k, taken relative to G at the largest z: (G_j - G_t) - sum_k (G_k - G_t) z_k.  The dominant
  // term of the sum is then exactly 0 and the rest carries small weights: a z_t close to 1 does not cancel a_t away.
  const float Gt = __shfl(G, (int)conc_wave_argmax(zz, conc_wave_max(zz), on, lane) & 63);   // (& 63: a NaN row has no top)
  const float Gr = on ? G - Gt : 0.f;
  const float a = Gr - wave_sum64(Gr * zz);
  float v = zz * a * inv_tau;
  if (analytic) {
    const float lp = conc_log_softmax(on ? p[o] : -INFINITY, on, lane);
    const float pi = on ? expf(lp) : 0.f;
    const float h = wave_sum64(pi * lp);   // sum pi log pi
    v = fmaf(wt * pi, lp - h, v);
  } else {
    v -= wt * (1.f - (float)K * zz) * inv_tau;
  }
  if (on) dp[o] = v;
}

int conc_check(const char* who, long long rows, int K, float tau, int analytic) {
  static char msg[128];
  const char* what = nullptr;
  if (K < 2 || K > CONC_KMAX) what = "K outside [2, 64]";
  else if (rows < 1 || rows > 0x7FFFFFF0ll) what = "batch outside [1, 2^31 - 16]";
  else if (!(tau > 0.f) || !std::isfinite(tau)) what = "the temperature must be positive";
  else if (analytic != 0 && analytic != 1) what = "analytic must be 0 (Monte Carlo) or 1 (the categorical KL)";
  if (what == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return odin_fail(-2, msg);
}

// lgamma(K) + (K - 1) log tau: the part of log q that depends on neither the logits nor the noise
float conc_const(int K, float tau) { return (float)(std::lgamma((double)K) + (K - 1) * std::log((double)tau)); }

}  // namespace

extern "C" int odin_rng_gumbel(float* out, size_t n, uint64_t seed, const int32_t* step_dev, void* stream) {
  if (out == nullptr || n == 0) return odin_fail(-2, "rng_gumbel: null output or n = 0");
  int grid = (int)std::min<size_t>(((n + 3) / 4 + 255) / 256, 2048);
  ODIN_LAUNCH(rng_gumbel_kernel, dim3(grid), dim3(256), 0, stream, out, n, (unsigned)seed, (unsigned)(seed >> 32),
              (const int*)step_dev);
  return odin_check_launch("rng_gumbel");
}

extern "C" int odin_latent_concrete_fwd(const float* p, float* g, float* z, float* kl, float* fbmask, int B, int K,
                                        float tau, int analytic, float free_bits, const float* capacity, int draw,
                                        uint64_t seed, const int32_t* step_dev, void* stream) {
  if (int rc = conc_check("latent_concrete_fwd", B, K, tau, analytic)) return rc;
  if (p == nullptr || g == nullptr || z == nullptr || kl == nullptr || fbmask == nullptr)
    return odin_fail(-2, "latent_concrete_fwd: null argument");
  ODIN_LAUNCH(latent_concrete_fwd_kernel, dim3((B + CONC_SPW - 1) / CONC_SPW), dim3(CONC_NT), 0, stream, p, g, z, kl,
              fbmask, B, K, 1.f / tau, conc_const(K, tau), analytic, free_bits, capacity, draw != 0 ? 1 : 0,
              (unsigned)seed, (unsigned)(seed >> 32), (const int*)step_dev);
  return odin_check_launch("latent_concrete_fwd");
}

extern "C" int odin_latent_concrete_bwd(const float* p, const float* g, const float* z, const float* dz,
                                        const float* dz_extra, const float* fbmask, const float* klw, float* dp, int B,
                                        int K, float tau, int analytic, void* stream) {
  if (int rc = conc_check("latent_concrete_bwd", B, K, tau, analytic)) return rc;
  (void)g;   // (the gradients need z alone: z = exp(y) is what the forward stored)
  if (p == nullptr || z == nullptr || fbmask == nullptr || klw == nullptr || dp == nullptr)
    return odin_fail(-2, "latent_concrete_bwd: null argument");
  ODIN_LAUNCH(latent_concrete_bwd_kernel, dim3((B + CONC_SPW - 1) / CONC_SPW), dim3(CONC_NT), 0, stream, p, z, dz,
              dz_extra, fbmask, klw, dp, B, K, 1.f / tau, analytic);
  return odin_check_launch("latent_concrete_bwd");
}

extern "C" int odin_latent_concrete_sample_logprob(const float* p, const float* g, float* z, float* logq, float* logp,
                                                   int n, int B, int K, float tau, void* stream) {
  if (n < 1 || B < 1) return odin_fail(-2, "latent_concrete_sample_logprob: n and B must be positive");
  if (int rc = conc_check("latent_concrete_sample_logprob", (long long)n * B, K, tau, 0)) return rc;
  if (p == nullptr || g == nullptr || z == nullptr || logq == nullptr || logp == nullptr)
    return odin_fail(-2, "latent_concrete_sample_logprob: null argument");
  const long long rows = (long long)n * B;
  ODIN_LAUNCH(latent_concrete_sample_logprob_kernel, dim3((unsigned)((rows + CONC_SPW - 1) / CONC_SPW)), dim3(CONC_NT),
              0, stream, p, g, z, logq, logp, n, B, K, 1.f / tau, conc_const(K, tau));
  return odin_check_launch("latent_concrete_sample_logprob");
}
