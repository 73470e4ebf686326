// latent_tril.hip -- the full-covariance Gaussian posterior q(z|x) = MultivariateNormalTriL(loc, L)
// (odin/bay/layers/continuous.py:459-474 with covariance='tril'; RVconf(D, 'mvntril', projection=True),
// odin/bay/distribution_alias.py:22-23): the projection emits p [B, D + M], M = D (D + 1) / 2,
//   loc = p[:, :D], r = p[:, D:], L = FillScaleTriL(diag_bijector=softplus, diag_shift=1e-5)(r)
// FillScaleTriL: r[D:] followed by r reversed are D * D values, read row-major as a D x D matrix of which the lower
// triangle is kept.  For j <= i and k = i D + j:  L_raw[i][j] = r[D + k] if k < M - D, else r[D D - 1 - k]
// (r = [1 .. 6] -> [[4, 0, 0], [6, 5, 0], [3, 2, 1]]); L_ii = softplus(L_raw_ii) + 1e-5, off-diagonal entries as they are.
//   z = loc + L eps;  log q(z) = -1/2 |eps|^2 - sum log L_ii - D/2 log 2 pi;  log p(z) = -1/2 |z|^2 - D/2 log 2 pi
//   KL: analytic = 0  log q(z) - log p(z) at that z;  1  1/2 (|L|_F^2 + |loc|^2 - D) - sum log L_ii
// forward / sample_logprob: ONE WAVE per sample, four samples per workgroup.  The sample's D + M <= 2144 floats and its
//   noise are staged in LDS with coalesced loads (wave-private: no workgroup barrier); lane i owns row i of L and walks
//   its i + 1 entries (two contiguous runs of r, one ascending, one descending); the per-row terms meet in a fixed
//   butterfly over the wave.
// backward: with w = klw fbmask_b, g = dz + dz_extra
//   analytic = 0: gz = g + w z; dloc = gz; dL_ij = gz_i eps_j - w delta_ij / L_ii
//   analytic = 1: dloc = g + w loc;        dL_ij = g_i eps_j + w (L_ij - delta_ij / L_ii)
//   dr = dL_ij off the diagonal, dL_ii sigmoid(L_raw_ii) on it
//   one wave per sample again: the D row factors (gz | g) and the noise go to LDS, then thread m takes element m of r
//   THROUGH THE INVERSE of the fill map -- (i, j) from m -- so that the raw value is read and dr is written contiguous
//   in m; no row of L is ever staged.  Every element of dp is written exactly once; no atomics on floats: two runs,
//   and eager versus graph replay, give the same bits.  max |dp| is folded into the optional range word.
// Limits (checked in the entries): 1 <= D <= 64 (a row per lane of a wave64), B >= 1.
#include "odin_device.h"
#include "odin_internal.h"
#include "odin_latent_math.h"

namespace {

constexpr int TRIL_NT = 256;
constexpr int TRIL_SPW = TRIL_NT / 64;   // samples per workgroup: one per wave
constexpr int TRIL_DMAX = 64;
constexpr float TRIL_SHIFT = 1e-5f;      // FillScaleTriL's diag_shift
constexpr float TRIL_LOG2PI = 1.8378770664093453f;

// floats of LDS per wave: the sample's projection row and its noise
__host__ __device__ inline size_t tril_wave_floats(int D) { return (size_t)D + (size_t)D * (D + 1) / 2 + D; }

// row `lane` of L against the staged sample (sp: loc | r, se: eps): z_i, the row's squared norm and L_ii
__device__ __forceinline__ void tril_row(const float* sp, const float* se, int D, int i, float& zz, float& sq,
                                         float& ld) {
  const float* r = sp + D;
  const int thr = D * (D + 1) / 2 - D, top = D * D - 1;
  zz = sp[i];
  sq = 0.f;
  int k = i * D;
  for (int j = 0; j < i; ++j, ++k) {
    const float l = r[k < thr ? D + k : top - k];
    zz = fmaf(l, se[j], zz);
    sq = fmaf(l, l, sq);
  }
  ld = softplus_f(r[k < thr ? D + k : top - k]) + TRIL_SHIFT;
  zz = fmaf(ld, se[i], zz);
  sq = fmaf(ld, ld, sq);
}

// stage row `row` of p [., D + M] and row `erow` of eps [., D] into this wave's LDS
__device__ __forceinline__ void tril_stage(const float* p, const float* eps, size_t row, size_t erow, int D, int lane,
                                           float* sp, float* se) {
  const int W = D + D * (D + 1) / 2;
  const float* pb = p + row * W;
  for (int e = lane; e < W; e += 64) sp[e] = pb[e];
  if (lane < D) se[lane] = eps[erow * D + lane];
  odin_wave_sync();
}

__global__ __launch_bounds__(TRIL_NT) void latent_tril_fwd_kernel(const float* p, const float* eps, float* z,
                                                                  float* kl, float* fbmask, int B, int D,
                                                                  int analytic, float free_bits, const float* cap) {
  ODIN_DYN_SMEM(float, smem);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * TRIL_SPW + w;
  if (b >= B) return;   // (wave-uniform, and a wave meets only itself below)
  float* sp = smem + (size_t)w * tril_wave_floats(D);
  float* se = sp + D + D * (D + 1) / 2;
  tril_stage(p, eps, (size_t)b, (size_t)b, D, lane, sp, se);
  float acc = 0.f;
  if (lane < D) {
    float zz, sq, ld;
    tril_row(sp, se, D, lane, zz, sq, ld);
    z[(size_t)b * D + lane] = zz;
    const float e = se[lane], loc = sp[lane], ll = odin_log(ld);
    acc = analytic ? 0.5f * (sq + loc * loc - 1.f) - ll : 0.5f * (zz * zz - e * e) - ll;
  }
  acc = wave_sum64(acc);
  if (lane != 0) return;
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
__global__ __launch_bounds__(TRIL_NT) void latent_tril_sample_logprob_kernel(const float* p, const float* eps, float* z,
                                                                             float* logq, float* logp, int n, int B,
                                                                             int D) {
  ODIN_DYN_SMEM(float, smem);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t i = (size_t)blockIdx.x * TRIL_SPW + w;
  if (i >= (size_t)n * B) return;   // (wave-uniform)
  float* sp = smem + (size_t)w * tril_wave_floats(D);
  float* se = sp + D + D * (D + 1) / 2;
  tril_stage(p, eps, i % (size_t)B, i, D, lane, sp, se);
  float lq = 0.f, lp = 0.f;
  if (lane < D) {
    float zz, sq, ld;
    tril_row(sp, se, D, lane, zz, sq, ld);
    z[i * D + lane] = zz;
    const float e = se[lane];
    lq = -0.5f * e * e - odin_log(ld);
    lp = -0.5f * zz * zz;
  }
  lq = wave_sum64(lq);
  lp = wave_sum64(lp);
  if (lane != 0) return;
  const float c = 0.5f * TRIL_LOG2PI * (float)D;
  logq[i] = lq - c;
  logp[i] = lp - c;
}

__global__ __launch_bounds__(TRIL_NT) void latent_tril_bwd_kernel(const float* p, const float* eps, const float* z,
                                                                  const float* dz, const float* dz2,
                                                                  const float* fbmask, const float* klw, float* dp,
                                                                  unsigned* dp_amax, int B, int D, int analytic) {
  __shared__ float sa[TRIL_SPW][TRIL_DMAX];   // the row factors of dL: gz (Monte Carlo) | g (closed form)
  __shared__ float se[TRIL_SPW][TRIL_DMAX];
  __shared__ float red[16];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * TRIL_SPW + w;
  const bool live = b < B;   // (wave-uniform; every thread reaches the range-word commit)
  const int M = D * (D + 1) / 2, W = D + M;
  const float* pb = p + (size_t)(live ? b : 0) * W;
  float* dpb = dp + (size_t)(live ? b : 0) * W;
  float wt = 0.f, amx = 0.f;
  if (live) {
    wt = klw[0] * fbmask[b];
    if (lane < D) {
      const size_t o = (size_t)b * D + lane;
      float g = 0.f;
      if (dz != nullptr) g += dz[o];
      if (dz2 != nullptr) g += dz2[o];
      const float a = analytic ? g : fmaf(wt, z[o], g);
      const float dloc = analytic ? fmaf(wt, pb[lane], g) : a;
      sa[w][lane] = a;
      se[w][lane] = eps[o];
      dpb[lane] = dloc;
      amx = fabsf(dloc);
    }
  }
  odin_wave_sync();
  if (live) {
    for (int m = lane; m < M; m += 64) {
      // the inverse of the fill map: r[m] sits at k = m - D (the head of the matrix, from r[D:]) or at k = D D - 1 - m
      // (from r reversed); exactly one of the two lies in the lower triangle
      int k = m - D, i = 0, j = 1;
      if (k >= 0) { i = k / D; j = k - i * D; }
      if (j > i) { k = D * D - 1 - m; i = k / D; j = k - i * D; }
      const float raw = pb[D + m];
      float v = sa[w][i] * se[w][j];
      if (i == j) {
        const float ld = softplus_f(raw) + TRIL_SHIFT;
        v = (v + wt * ((analytic ? ld : 0.f) - 1.f / ld)) * sigmoid_f(raw);
      } else if (analytic) {
        v = fmaf(wt, raw, v);
      }
      dpb[D + m] = v;
      amx = fmaxf(amx, fabsf(v));
    }
  }
  odin_amax_commit_wg(dp_amax, amx, tid, TRIL_NT, red, blockIdx.x);
}

int tril_check(const char* who, long long rows, int D) {
  static char msg[96];
  const char* what = nullptr;
  if (D < 1 || D > TRIL_DMAX) what = "D outside [1, 64]";
  else if (rows < 1 || rows > 0x7FFFFFF0ll) what = "batch outside [1, 2^31 - 16]";
  if (what == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return odin_fail(-2, msg);
}

}  // namespace

extern "C" int odin_latent_tril_fwd(const float* p, const float* eps, float* z, float* kl, float* fbmask, int B,
                                    int D, int analytic, float free_bits, const float* capacity, void* stream) {
  if (int rc = tril_check("latent_tril_fwd", B, D)) return rc;
  if (p == nullptr || eps == nullptr || z == nullptr || kl == nullptr || fbmask == nullptr)
    return odin_fail(-2, "latent_tril_fwd: null argument");
  if (analytic != 0 && analytic != 1)
    return odin_fail(-2, "latent_tril_fwd: analytic must be 0 (Monte Carlo) or 1 (KL(q || p)); KL(p || q) needs the inverse of L");
  const size_t lds = TRIL_SPW * tril_wave_floats(D) * sizeof(float);   // <= 35328 bytes
  ODIN_LAUNCH(latent_tril_fwd_kernel, dim3((B + TRIL_SPW - 1) / TRIL_SPW), dim3(TRIL_NT), lds, stream, p, eps, z, kl,
              fbmask, B, D, analytic, free_bits, capacity);
  return odin_check_launch("latent_tril_fwd");
}

extern "C" int odin_latent_tril_bwd(const float* p, const float* eps, const float* z, const float* dz,
                                    const float* dz_extra, const float* fbmask, const float* klw, float* dp,
                                    uint32_t* dp_amax, int B, int D, int analytic, void* stream) {
  if (int rc = tril_check("latent_tril_bwd", B, D)) return rc;
  if (p == nullptr || eps == nullptr || z == nullptr || fbmask == nullptr || klw == nullptr || dp == nullptr)
    return odin_fail(-2, "latent_tril_bwd: null argument");
  if (analytic != 0 && analytic != 1) return odin_fail(-2, "latent_tril_bwd: analytic must be 0 or 1");
  ODIN_LAUNCH(latent_tril_bwd_kernel, dim3((B + TRIL_SPW - 1) / TRIL_SPW), dim3(TRIL_NT), 0, stream, p, eps, z, dz,
              dz_extra, fbmask, klw, dp, (unsigned*)dp_amax, B, D, analytic);
  return odin_check_launch("latent_tril_bwd");
}

extern "C" int odin_latent_tril_sample_logprob(const float* p, const float* eps, float* z, float* logq, float* logp,
                                               int n, int B, int D, void* stream) {
  if (n < 1 || B < 1) return odin_fail(-2, "latent_tril_sample_logprob: n and B must be positive");
  if (int rc = tril_check("latent_tril_sample_logprob", (long long)n * B, D)) return rc;
  if (p == nullptr || eps == nullptr || z == nullptr || logq == nullptr || logp == nullptr)
    return odin_fail(-2, "latent_tril_sample_logprob: null argument");
  const size_t lds = TRIL_SPW * tril_wave_floats(D) * sizeof(float);
  const long long rows = (long long)n * B;
  ODIN_LAUNCH(latent_tril_sample_logprob_kernel, dim3((unsigned)((rows + TRIL_SPW - 1) / TRIL_SPW)), dim3(TRIL_NT), lds,
              stream, p, eps, z, logq, logp, n, B, D);
  return odin_check_launch("latent_tril_sample_logprob");
}
