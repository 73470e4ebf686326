// elbo_counts.hip -- the count observations of the gene-expression stacks: Independent(NegativeBinomial(total_count =
// exp(a), logits = l)).log_prob(x) ('nb'; NegativeBinomialLayer, odin/bay/layers/count_layers.py:75-163), its
// zero-inflated form ('zinb'; ZINegativeBinomialLayer, :311-416; ZeroInflated.log_prob, odin/bay/distributions/
// zero_inflated.py:216-230), forward + backward in one pass, and LogNorm (odin/networks/image_networks.py:138-151), the
// encoder's first layer of those stacks.
//
// One element, with r = e^a (nb1 below):
//   llk      = [lgamma(r + x) - lgamma(r)] - lgamma(1 + x) - r softplus(l) - x softplus(-l)
//   dllk/da  = r ([psi(r + x) - psi(r)] - softplus(l))
//   dllk/dl  = x sigmoid(-l) - r sigmoid(l)
// The two bracketed terms are never formed from their two halves: lgamma(r) grows like r log r, so at r = e^9 the halves
// carry 7e4 and their float32 difference has lost every digit of a log-likelihood of order 1.  Both are
// DIFFERENCES from the start.  With y = r lifted to y >= 8 (y = r + 8 where r < 8; P(t) = t (t + 1) ... (t + 7)) and
// u = x / y:
//   lgamma(r + x) - lgamma(r) = x log y + (y + x - 1/2) log1p(u) - x + [S(y + x) - S(y)] - log(P(r + x) / P(r))
//   psi(r + x) - psi(r)       = log1p(u) - [T(y + x) - T(y)] + x sum_{k < 8} 1 / ((r + k) (r + x + k))
// S(t) = 1/(12 t) - 1/(360 t^3) + 1/(1260 t^5) - 1/(1680 t^7) and T(t) = 1/(2 t) + 1/(12 t^2) - 1/(120 t^4) + 1/(252 t^6)
// are the Stirling tails (first dropped terms at t = 8: 6e-12 and 2.5e-10); the lifting terms are taken only where
// r < 8 (both forms are evaluated, one is selected: no divergent branch).  Every term carries a factor x, log1p(u) or a
// difference of equal expressions, so x = 0 gives exactly 0 for both, at any r.
//
// Domain: the element is float64, where e^a overflows only near a = 709 and the lifting products are formed from a
// harmless r = 1 wherever r >= 8; what overflows first are the float32 OUTPUTS: past a = 88 r = e^a exceeds the float32
// range, and with it r softplus(l) and r sigmoid(l) unless l is correspondingly negative (the reference's float32 e^a
// overflows there itself).  |a| <= 30 is tested, nothing is promised beyond a = 80.
//
// The element function runs in float64.  This kernel is latency-sized (the pbmc batch is 256 x 2019 elements), the
// domain is wide (|a| <= 30: r from 1e-13 to 1e13, where a float32 e^a alone is 30 ulp off and r psi(r) -> -1 needs
// 1 / r kept to full precision), and in float64 the forms above need no further case analysis; DESIGN 3.20 has the cost.
//
// Layout: params [B, P G] = (a | l) or (a | l | pi) as PLANES of G floats per sample (split(params, P, axis=-1)), x
// [B, G].  One workgroup of 256 threads per 256 consecutive genes of a sample, lane-linear 4-byte accesses (the planes
// start at p G floats: 8-byte aligned for G = 558, 4-byte aligned for G = 2019 -- there is no vector path to guard),
// n_part = ceil(G / 256) partials per sample, reduced in a fixed order; every output written once; one atomicMax per
// workgroup into the range word.
#include "odin_device.h"
#include "odin_internal.h"
#include <cmath>
#include <cstdint>

namespace {

// log-likelihood of one NB element and its derivatives with respect to a and l
__device__ __forceinline__ void nb1(double a, double l, double x, double& llk, double& ga, double& gl) {
  const double r = exp(a);
  const bool lift = r < 8.0;
  const double rs = lift ? r : 1.0;       // (the lifting terms are formed from a harmless r where they are not taken)
  const double y = lift ? r + 8.0 : r;
  double p0 = rs, p1 = rs + x, hs = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double t0 = rs + (double)k, t1 = t0 + x;
    if (k > 0) {
      p0 *= t0;
      p1 *= t1;
    }
    hs += 1.0 / (t0 * t1);
  }
  const double yx = y + x;
  const double lu = log1p(x / y);
  const double iy = 1.0 / y, iyx = 1.0 / yx, iy2 = iy * iy, iyx2 = iyx * iyx;
  const double Sy = iy * (1.0 / 12 + iy2 * (-1.0 / 360 + iy2 * (1.0 / 1260 - iy2 * (1.0 / 1680))));
  const double Syx = iyx * (1.0 / 12 + iyx2 * (-1.0 / 360 + iyx2 * (1.0 / 1260 - iyx2 * (1.0 / 1680))));
  const double Ty = iy * (0.5 + iy * (1.0 / 12 + iy2 * (-1.0 / 120 + iy2 * (1.0 / 252))));
  const double Tyx = iyx * (0.5 + iyx * (1.0 / 12 + iyx2 * (-1.0 / 120 + iyx2 * (1.0 / 252))));
  const double dlg = x * log(y) + (yx - 0.5) * lu - x + (Syx - Sy) - (lift ? log(p1 / p0) : 0.0);
  const double dpsi = lu - (Tyx - Ty) + (lift ? x * hs : 0.0);
  // softplus(+-l) = max(+-l, 0) + log1p(e^-|l|), sigmoid(+-l) from the same exponential
  const double e = exp(-fabs(l));
  const double L = log1p(e);
  const double spl = fmax(l, 0.0) + L, spn = fmax(-l, 0.0) + L;
  const double q = 1.0 / (1.0 + e);
  const double sgl = l >= 0.0 ? q : e * q, sgn = l >= 0.0 ? e * q : q;
  llk = dlg - lgamma(1.0 + x) - r * spl - x * spn;
  ga = r * (dpsi - spl);
  gl = x * sgn - r * sgl;
}

// ZI = 0: params (a | l); ZI = 1: (a | l | pi) with pi the inflation logit
template <int ZI>
__global__ __launch_bounds__(256) void elbo_nb_kernel(const float* __restrict__ params, const float* __restrict__ x,
                                                      float* __restrict__ llk_part, float* __restrict__ dparams,
                                                      const float* __restrict__ scale, int G, int n_part,
                                                      unsigned* __restrict__ g_amax) {
  __shared__ float red[8];   // the four waves' log-likelihood sums | their maxima of |dparams|
  const unsigned b = blockIdx.x / (unsigned)n_part, part = blockIdx.x - b * (unsigned)n_part;
  const int i = (int)part * 256 + (int)threadIdx.x;
  const size_t pb = (size_t)b * (size_t)(2 + ZI) * (size_t)G + (size_t)i;
  const float sc = scale[0];
  float acc = 0.f, amx = 0.f;
  if (i < G) {
    const double a = (double)params[pb], l = (double)params[pb + (size_t)G];
    const double xv = (double)x[(size_t)b * G + i];
    double llk, ga, gl;
    nb1(a, l, xv, llk, ga, gl);
    float da, dl;
    if (ZI) {
      const double pi = (double)params[pb + 2 * (size_t)G];
      const double ep = exp(-fabs(pi));
      const double t2 = fmax(-pi, 0.0) + log1p(ep);             // softplus(-pi)
      const double qp = 1.0 / (1.0 + ep);
      const double sgp = pi >= 0.0 ? qp : ep * qp, sgnp = pi >= 0.0 ? ep * qp : qp;   // sigmoid(pi), sigmoid(-pi)
      const double t1 = llk - pi;
      const double et = exp(-fabs(t1));
      const double sp1 = fmax(t1, 0.0) + log1p(et);             // softplus(t1)
      const double qt = 1.0 / (1.0 + et);
      const double s = t1 >= 0.0 ? qt : et * qt;                // sigmoid(t1)
      // both branches evaluated, one selected
      const bool pos = xv > 1e-8;
      const double w = pos ? 1.0 : s;
      acc = (float)((pos ? t1 : sp1) - t2);
      da = (float)(-(double)sc * (w * ga));
      dl = (float)(-(double)sc * (w * gl));
      const float dpi = (float)(-(double)sc * (pos ? -sgp : sgnp - s));
      dparams[pb + 2 * (size_t)G] = dpi;
      amx = fabsf(dpi);
    } else {
      acc = (float)llk;
      da = (float)(-(double)sc * ga);
      dl = (float)(-(double)sc * gl);
    }
    dparams[pb] = da;
    dparams[pb + (size_t)G] = dl;
    amx = odin_amax3(amx, da, dl);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the waves' maxima ride in the LDS round of the partial sum: ONE atomicMax per workgroup (odin_device.h: range words)
  const float wmx = g_amax != nullptr ? odin_wave_max64(amx) : 0.f;
  acc = wave_sum64(acc);
  if (lane == 0) {
    red[wave] = acc;
    red[4 + wave] = wmx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    llk_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (g_amax != nullptr)
      atomicMax(g_amax + (blockIdx.x & (ODIN_RANGE_SLOTS - 1)) * ODIN_RANGE_STRIDE,
                odin_fbits(fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]))));
  }
}

// one workgroup per row: the row total in float64 (thread-strided sums, then a fixed tree through LDS), then
// y = log1p(1e4 x / (total + 1e-8)) with the argument scaled in float64 and the logarithm taken in float32
__global__ __launch_bounds__(256) void lognorm_kernel(const float* __restrict__ x, float* __restrict__ y, int G,
                                                      unsigned* __restrict__ g_amax) {
  __shared__ double red[256];
  __shared__ float redf[16];
  const size_t base = (size_t)blockIdx.x * (size_t)G;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < G; i += 256) s += (double)x[base + i];
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double k = 1e4 / (red[0] + 1e-8);
  float amx = 0.f;
  for (int i = tid; i < G; i += 256) {
    const float v = log1pf((float)((double)x[base + i] * k));
    y[base + i] = v;
    amx = fmaxf(amx, fabsf(v));
  }
  odin_amax_commit_wg(g_amax, amx, tid, 256, redf, blockIdx.x);
}

}  // namespace

extern "C" int odin_elbo_nb_fwd_bwd(const float* params, const float* x, float* llk_part, float* dparams,
                                    const float* scale, int B, int G, int zero_inflated, int* n_part_out,
                                    uint32_t* dparams_amax, void* stream) {
  if (B < 1 || G < 1) return odin_fail(-2, "elbo_nb: B and G must be positive");
  if (G > (1 << 28)) return odin_fail(-2, "elbo_nb: more than 2^28 genes per sample");
  if (zero_inflated != 0 && zero_inflated != 1) return odin_fail(-2, "elbo_nb: zero_inflated must be 0 or 1");
  const int n_part = (G + 255) / 256;
  const size_t n_blocks = (size_t)B * n_part;
  if (n_blocks > 0x7fffffffull) return odin_fail(-2, "elbo_nb: too many partial sums for one launch");
  if (n_part_out) *n_part_out = n_part;
  if (params == nullptr) return 0;  // dry run: reports the partial count
  unsigned* g_amax = reinterpret_cast<unsigned*>(dparams_amax);
  if (zero_inflated)
    ODIN_LAUNCH(elbo_nb_kernel<1>, dim3((unsigned)n_blocks), dim3(256), 0, stream, params, x, llk_part, dparams, scale,
                G, n_part, g_amax);
  else
    ODIN_LAUNCH(elbo_nb_kernel<0>, dim3((unsigned)n_blocks), dim3(256), 0, stream, params, x, llk_part, dparams, scale,
                G, n_part, g_amax);
  return odin_check_launch("elbo_nb");
}

extern "C" int odin_lognorm_fwd(const float* x, float* y, int B, int G, uint32_t* y_amax, void* stream) {
  if (B < 1 || G < 1) return odin_fail(-2, "lognorm: B and G must be positive");
  if (G > (1 << 28)) return odin_fail(-2, "lognorm: more than 2^28 genes per row");
  ODIN_LAUNCH(lognorm_kernel, dim3((unsigned)B), dim3(256), 0, stream, x, y, G, reinterpret_cast<unsigned*>(y_amax));
  return odin_check_launch("lognorm");
}
