// vamprior.hip -- the VampPrior of VampriorVAE (odin/bay/vi/autoencoder/vamprior.py:25-107, Tomczak & Welling 2018):
// a uniform mixture of the encoder's own posteriors at K learned pseudo-inputs,
//   log p(z_b) = logsumexp_k [ sum_d log N(z_bd; loc_kd, sigma_kd) ] - log K,   sigma = softplus(raw),
// as a CORRECTION to the standard-normal KL every fused latent kernel already computes:
//   c_b = log N(z_b; 0, I) - log p(z_b)        (kl_vamp,b = kl_std,b + c_b; the -D/2 log 2 pi of both sides cancels)
// and the gradients of sum_b c_b with respect to z, loc and raw (responsibilities r_bk = softmax_k):
//   dz_bd   = -z_bd + sum_k r_bk (z_bd - loc_kd) / sigma_kd^2
//   dloc_kd = -sum_b r_bk (z_bd - loc_kd) / sigma_kd^2
//   dsig_kd = -sum_b r_bk ((z_bd - loc_kd)^2 / sigma_kd^3 - 1 / sigma_kd),   draw = dsig * sigmoid(raw)
//
// Three launches inside the one entry, ordered by the stream:
//   prep : the component table (loc, 1 / sigma, sum_d log sigma) in float64, once per component, in both layouts
//   rows : one workgroup per R rows of z: log densities, row maximum, lse[b], c[b], the responsibilities (LDS only), dz
//   comps: one workgroup per component: the responsibilities of its column again from lse[b], the sums over b;
//          workgroup 0 also leaves coef * mean(c)
// Nothing of size [B, K] or [B, K, D] reaches HBM; lse[B] is what the second phase re-reads.  Every sum over k (rows)
// and over b (comps) runs in float64 inside ONE workgroup: a thread walks a fixed subset, the partials meet in a fixed
// order.  No atomics at all, so two runs (and eager versus graph replay) give the same bits.
//
// Why float64: with sigma = 1e-3 and |z - loc| = 30 a log density is near -4e8, where one float32 ulp is 32 -- the
// responsibilities of two components that compete there would be noise.  The arithmetic is B K D fused multiply-adds
// (1.3 M for the dSprites step), far below what the double-precision vector rate makes visible.
#include "odin_device.h"
#include "odin_internal.h"

namespace {

constexpr int VP_NT = 256;
constexpr int VP_DMAX = 64;
constexpr int VP_KMAX = 1024;
constexpr int VP_BMAX = 4096;
constexpr int VP_RMAX = 4;   // rows of z per workgroup of the rows phase

// workspace (doubles, behind the 8 leading floats [value | spare ...]):
//   tab  [K][2D]  (loc | 1 / sigma) per component      -- the per-dimension phases read a component's row
//   tabT [2D][K]  the same, transposed                  -- the per-component phases read a dimension's row (coalesced)
//   lsig [K]      sum_d log sigma_kd
//   lse  [B]      logsumexp_k of the unnormalised log densities
struct VpWs {
  double* tab;
  double* tabT;
  double* lsig;
  double* lse;
};

__host__ __device__ inline size_t vp_ws_doubles(int B, int K, int D) {
  return (size_t)4 * K * D + (size_t)K + (size_t)B;
}

inline VpWs vp_ws(float* ws, int K, int D) {
  VpWs w;
  w.tab = reinterpret_cast<double*>(ws + 8);
  w.tabT = w.tab + (size_t)2 * K * D;
  w.lsig = w.tabT + (size_t)2 * K * D;
  w.lse = w.lsig + K;
  return w;
}

__device__ __forceinline__ double softplus_d(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// Fixed-shape tree over VP_NT doubles in LDS; every thread returns the result.
template <bool MAX>
__device__ __forceinline__ double block_red_d(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll 1
  for (int s = VP_NT / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] = MAX ? fmax(red[tid], red[tid + s]) : red[tid] + red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(VP_NT) void vamp_prep_kernel(const float* pu, int K, int D, VpWs w) {
  const int k = blockIdx.x * VP_NT + threadIdx.x;
  if (k >= K) return;
  double ls = 0.0;
  for (int d = 0; d < D; ++d) {
    const double loc = (double)pu[(size_t)k * 2 * D + d];
    const double sg = softplus_d((double)pu[(size_t)k * 2 * D + D + d]);
    const double is = 1.0 / sg;
    ls += log(sg);
    w.tab[(size_t)k * 2 * D + d] = loc;
    w.tab[(size_t)k * 2 * D + D + d] = is;
    w.tabT[(size_t)d * K + k] = loc;
    w.tabT[(size_t)(D + d) * K + k] = is;
  }
  w.lsig[k] = ls;
}

struct VpArgs {
  const float* z;          // [B, D]
  const float* pu;         // [K, 2D]
  int B, K, D, R;
  const float* coef;
  const float* coef_grad;
  float* c;                // [B]
  float* out;              // out[0] = coef * mean_b c_b
  float* dz;               // [B, D] or NULL
  float* dpu;              // [K, 2D] or NULL
  VpWs w;
};

// rows b0 .. b0 + R of z against every component
__global__ __launch_bounds__(VP_NT) void vamp_rows_kernel(VpArgs g) {
  __shared__ double lk[VP_RMAX * VP_KMAX];   // log densities, then responsibilities
  __shared__ double zr[VP_RMAX * VP_DMAX];
  __shared__ double red[VP_NT];
  __shared__ double lse_s[VP_RMAX];
  const int tid = threadIdx.x, D = g.D, K = g.K;
  const int b0 = blockIdx.x * g.R;
  const int nr = g.B - b0 < g.R ? g.B - b0 : g.R;
  for (int e = tid; e < nr * D; e += VP_NT) {
    const int r = e / D, d = e - r * D;
    zr[r * VP_DMAX + d] = (double)g.z[(size_t)(b0 + r) * D + d];
  }
  __syncthreads();
  for (int k = tid; k < K; k += VP_NT) {
    double s[VP_RMAX] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d) {
      const double loc = g.w.tabT[(size_t)d * K + k], is = g.w.tabT[(size_t)(D + d) * K + k];
#pragma unroll
      for (int r = 0; r < VP_RMAX; ++r) {
        if (r < nr) {
          const double t = (zr[r * VP_DMAX + d] - loc) * is;
          s[r] = fma(t, t, s[r]);
        }
      }
    }
    const double ls = g.w.lsig[k];
#pragma unroll
    for (int r = 0; r < VP_RMAX; ++r)
      if (r < nr) lk[r * VP_KMAX + k] = -0.5 * s[r] - ls;
  }
  __syncthreads();
  for (int r = 0; r < nr; ++r) {
    double m = -INFINITY;
    for (int k = tid; k < K; k += VP_NT) m = fmax(m, lk[r * VP_KMAX + k]);
    m = block_red_d<true>(m, red);
    double a = 0.0;
    for (int k = tid; k < K; k += VP_NT) a += exp(lk[r * VP_KMAX + k] - m);
    a = block_red_d<false>(a, red);
    const double lse = m + log(a);
    if (tid == 0) {
      double zz = 0.0;
      for (int d = 0; d < D; ++d) zz = fma(zr[r * VP_DMAX + d], zr[r * VP_DMAX + d], zz);
      g.c[b0 + r] = (float)(-0.5 * zz - lse + log((double)K));
      g.w.lse[b0 + r] = lse;
      lse_s[r] = lse;
    }
  }
  if (g.dz == nullptr) return;   // (a kernel argument: uniform)
  __syncthreads();
  for (int r = 0; r < nr; ++r)
    for (int k = tid; k < K; k += VP_NT) lk[r * VP_KMAX + k] = exp(lk[r * VP_KMAX + k] - lse_s[r]);
  __syncthreads();
  // thread (q, d) = (tid >> 6, tid & 63) walks the components k = q, q + 4, ...; the four partials meet in a fixed order
  const int gd = tid & 63, gq = tid >> 6;
  const double cg = g.coef_grad != nullptr ? (double)g.coef_grad[0] : 1.0;
  for (int r = 0; r < nr; ++r) {
    double a = 0.0;
    if (gd < D) {
      const double zd = zr[r * VP_DMAX + gd];
      for (int k = gq; k < K; k += 4) {
        const double is = g.w.tab[(size_t)k * 2 * D + D + gd];
        a = fma(lk[r * VP_KMAX + k] * (zd - g.w.tab[(size_t)k * 2 * D + gd]), is * is, a);
      }
    }
    red[tid] = a;
    __syncthreads();
    if (tid < D) {
      const double v = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
      g.dz[(size_t)(b0 + r) * D + tid] = (float)(cg * (v - zr[r * VP_DMAX + tid]));
    }
    __syncthreads();
  }
}

// component k = blockIdx.x against every row of z; workgroup 0 also sums c[B]
__global__ __launch_bounds__(VP_NT) void vamp_comps_kernel(VpArgs g) {
  __shared__ double rb[VP_BMAX];   // responsibilities of this component's column
  __shared__ double red[3 * VP_NT];
  const int tid = threadIdx.x, D = g.D, K = g.K, B = g.B, k = blockIdx.x;
  if (k == 0) {
    double a = 0.0;
    for (int b = tid; b < B; b += VP_NT) a += (double)g.c[b];
    a = block_red_d<false>(a, red);
    if (tid == 0) g.out[0] = (float)((g.coef != nullptr ? (double)g.coef[0] : 1.0) * (a / (double)B));
  }
  if (g.dpu == nullptr) return;   // (forward only: this launch has one workgroup)
  const double* tk = g.w.tab + (size_t)k * 2 * D;
  const double ls = g.w.lsig[k];
  for (int b = tid; b < B; b += VP_NT) {
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
      const double t = ((double)g.z[(size_t)b * D + d] - tk[d]) * tk[D + d];
      s = fma(t, t, s);
    }
    rb[b] = exp(-0.5 * s - ls - g.w.lse[b]);
  }
  __syncthreads();
  const int gd = tid & 63, gq = tid >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (gd < D) {
    const double loc = tk[gd];
    for (int b = gq; b < B; b += 4) {
      const double r = rb[b], t = (double)g.z[(size_t)b * D + gd] - loc;
      a0 += r;
      a1 = fma(r, t, a1);
      a2 = fma(r * t, t, a2);
    }
  }
  red[tid] = a0; red[VP_NT + tid] = a1; red[2 * VP_NT + tid] = a2;
  __syncthreads();
  if (tid < D) {
    const double* r1 = red + VP_NT;
    const double* r2 = red + 2 * VP_NT;
    const double s0 = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
    const double s1 = (r1[tid] + r1[64 + tid]) + (r1[128 + tid] + r1[192 + tid]);
    const double s2 = (r2[tid] + r2[64 + tid]) + (r2[128 + tid] + r2[192 + tid]);
    const double cg = g.coef_grad != nullptr ? (double)g.coef_grad[0] : 1.0;
    const double is = tk[D + tid];
    const double raw = (double)g.pu[(size_t)k * 2 * D + D + tid];
    const double sgm = 1.0 / (1.0 + exp(-raw));   // d softplus / d raw
    g.dpu[(size_t)k * 2 * D + tid] = (float)(-cg * is * is * s1);
    g.dpu[(size_t)k * 2 * D + D + tid] = (float)(-cg * (is * is * is * s2 - is * s0) * sgm);
  }
}

}  // namespace

// workspace in floats: [0] = coef * mean_b c_b | [1..7] spare | the float64 tables (8-byte aligned)
extern "C" int odin_vamprior_workspace(int B, int K, int D) {
  if (B < 1 || K < 1 || D < 1) return 0;
  return 8 + 2 * (int)vp_ws_doubles(B, K, D);
}

extern "C" int odin_vamprior_fwd_bwd(const float* z, const float* pu, float* ws, float* c, float* dz, float* dpu,
                                     const float* coef, const float* coef_grad, int B, int K, int D, void* stream) {
  if (D < 1 || D > VP_DMAX) return odin_fail(-2, "vamprior: D outside [1, 64]");
  if (B < 1 || B > VP_BMAX) return odin_fail(-2, "vamprior: B outside [1, 4096]");
  if (K < 1 || K > VP_KMAX) return odin_fail(-2, "vamprior: K outside [1, 1024]");
  if (z == nullptr || pu == nullptr || ws == nullptr || c == nullptr) return odin_fail(-2, "vamprior: null argument");
  if ((((size_t)ws) & 7) != 0) return odin_fail(-2, "vamprior: workspace must be 8-byte aligned");
  if ((dz == nullptr) != (dpu == nullptr)) return odin_fail(-2, "vamprior: dz and dpu go together");
  VpArgs g;
  g.z = z; g.pu = pu; g.B = B; g.K = K; g.D = D;
  // rows per workgroup of the rows phase: the component table is read once per workgroup -- share it between a few
  // rows once there are enough workgroups for every compute unit
  g.R = B >= 4 * 256 ? 4 : (B >= 2 * 256 ? 2 : 1);
  g.coef = coef; g.coef_grad = coef_grad; g.c = c; g.out = ws; g.dz = dz; g.dpu = dpu;
  g.w = vp_ws(ws, K, D);
  ODIN_LAUNCH(vamp_prep_kernel, dim3((K + VP_NT - 1) / VP_NT), dim3(VP_NT), 0, stream, pu, K, D, g.w);
  if (int rc = odin_check_launch("vamprior_prep")) return rc;
  ODIN_LAUNCH(vamp_rows_kernel, dim3((B + g.R - 1) / g.R), dim3(VP_NT), 0, stream, g);
  if (int rc = odin_check_launch("vamprior_rows")) return rc;
  ODIN_LAUNCH(vamp_comps_kernel, dim3(dpu != nullptr ? K : 1), dim3(VP_NT), 0, stream, g);
  return odin_check_launch("vamprior_comps");
}

// u = clip(w, lo, hi) (vamprior.py: hard_probs = clip_by_value of the pseudo-input variable)
namespace {
__global__ __launch_bounds__(256) void clip_fwd_kernel(const float* w, float* u, size_t n, float lo, float hi) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) u[i] = fminf(fmaxf(w[i], lo), hi);
}
// clip_by_value's gradient, in place: g = scale * g * [lo < w < hi]  (TF: 1 strictly inside, 0 elsewhere)
__global__ __launch_bounds__(256) void clip_bwd_kernel(const float* w, float* g, size_t n, float lo, float hi,
                                                       float scale) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) g[i] = (w[i] > lo && w[i] < hi) ? scale * g[i] : 0.f;
}
}  // namespace

extern "C" int odin_clip_range_fwd(const float* w, float* u, size_t n, float lo, float hi, void* stream) {
  if (n == 0) return 0;
  if (w == nullptr || u == nullptr) return odin_fail(-2, "clip_range_fwd: null argument");
  ODIN_LAUNCH(clip_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, u, n, lo, hi);
  return odin_check_launch("clip_range_fwd");
}

extern "C" int odin_clip_range_bwd(const float* w, float* g, size_t n, float lo, float hi, float scale, void* stream) {
  if (n == 0) return 0;
  if (w == nullptr || g == nullptr) return odin_fail(-2, "clip_range_bwd: null argument");
  ODIN_LAUNCH(clip_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, g, n, lo, hi, scale);
  return odin_check_launch("clip_range_bwd");
}
