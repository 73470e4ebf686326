// latent_reg.hip -- batch-coupled latent regularisers of InfoVAE and DIPVAE, forward and backward in one launch each:
//   maximum_mean_discrepancy          : odin/bay/vi/losses.py:163-276 (info_vae.py:28-91, q_sample_shape=None)
//   disentangled_inferred_prior_loss  : odin/bay/vi/losses.py:39-98   (dip_vae.py)
//
// Both are one scalar of the whole batch of latents; the gradients reach the step only through z (MMD) or
// (loc, scale) (DIP), i.e. the dz_extra / dloc_x / dscale_x inputs every latent backward form accepts.
//
// Reduction order.  Every cross-row sum runs in float64 in a fixed order: a thread walks a fixed subset of rows,
// the threads' partials meet in an LDS tree of fixed shape.  The MMD estimate (a small difference of three means
// of size ~0.5) leaves each workgroup as ONE 64-bit fixed-point word (2^-32 units) added with an integer atomic --
// integer addition is associative, so the order in which workgroups arrive cannot change a bit -- and the last
// workgroup to take an arrival ticket converts the total.  No float atomics anywhere.
#include "odin_device.h"
#include "odin_internal.h"
#include "odin_latent_math.h"

namespace {

constexpr int MMD_NT = 256;      // threads of an MMD workgroup
constexpr int MMD_T = 256;       // at most this many rows of the other operand staged in LDS per chunk (T * D <= 8192)
constexpr int MMD_DMAX = 64;
constexpr int MMD_NMAX = 4096;
constexpr int MMD_MMAX = 512;
constexpr double MMD_FX = 4294967296.0;   // fixed point: 2^32 units per 1.0
constexpr int MMD_TB = 13;                // arrival-count bits below the fixed-point sum

constexpr int DIP_NT = 1024;
constexpr int DIP_DMAX = 64;
constexpr int DIP_T = 128;       // centred rows staged in LDS per chunk (DIP_T * D <= 8192 floats)

__device__ __forceinline__ float softplus_r(float x) { return fmaxf(x, 0.f) + log1pf(odin_exp(-fabsf(x))); }

// Fixed-shape tree over NT doubles in LDS (NT a power of two); every thread returns the total.
template <int NT>
__device__ __forceinline__ double block_sum_d(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll 1
  for (int s = NT / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Rows [r0, r0 + nr) of the prior sample y into dst[nr][D]: the explicit tensor, or elements r0*D .. of the stream
// odin_rng_normal(prior_seed, step) writes (element e = component e & 3 of Philox counter e >> 2).
__device__ void mmd_stage_y(float* dst, const float* y, int r0, int nr, int D, unsigned k0, unsigned k1,
                            unsigned step) {
  const int e0 = r0 * D, e1 = (r0 + nr) * D;
  if (y != nullptr) {
    for (int e = e0 + (int)threadIdx.x; e < e1; e += MMD_NT) dst[e - e0] = y[e];
    return;
  }
  for (int c = (e0 >> 2) + (int)threadIdx.x; c <= ((e1 - 1) >> 2); c += MMD_NT) {
    float v[4];
    odin_normal4((unsigned)c, 0u, step, k0, k1, v);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = 4 * c + u;
      if (e >= e0 && e < e1) dst[e - e0] = v[u];
    }
  }
}

struct MmdArgs {
  const float* xs;      // [Bl, D] rows whose gradient this launch forms (this rank's)
  const float* xall;    // [Bg, D] every row of q's sample (== xs on one GPU)
  const float* y;       // [M, D] prior sample, or NULL: drawn from Philox (k0, k1, step)
  int Bl, Bg, M, D, kind, include_yy;
  unsigned k0, k1;
  const int* step_dev;
  const float* coef;       // value scale (NULL: 1)
  const float* coef_grad;  // gradient scale (NULL: 1)
  float* dz;               // [Bl, D] or NULL (forward only)
  float* out;              // out[0]: this launch's share of coef * MMD
  unsigned long long* acc; // fixed-point sum | arrival count (zero between launches: the last arrival clears it)
};

// Workgroup r < Bl: row a = xs[r] against every x_j and every y_m (value terms k(x, x), k(x, y) and dz[r]);
// workgroup Bl + m (include_yy): row a = y_m against every y (value term k(y, y) only).
//   gaussian (kind 0): k = exp(-|a - b|^2 / D)      dk/da = -2/D (a - b) k
//   linear   (kind 1): k = |sum_d (a_d - b_d)|      dk/da_d = sign(sum_d (a_d - b_d))   (sign(0) = 0, TF's abs)
// Distances are formed as differences, so the diagonal gives exactly k = 1 (gaussian) / 0 (linear).
__global__ __launch_bounds__(MMD_NT) void mmd_rows_kernel(MmdArgs g) {
  __shared__ float cb[8192];               // staged rows of the other operand
  __shared__ float wk[MMD_T];              // per staged row: k (gaussian) or sign (linear)
  __shared__ float arow[MMD_DMAX];
  __shared__ double red[MMD_NT];
  const int tid = threadIdx.x, D = g.D, r = blockIdx.x;
  const bool xrow = r < g.Bl;
  const unsigned step = g.step_dev != nullptr ? (unsigned)g.step_dev[0] : 0u;
  if (xrow) {
    for (int d = tid; d < D; d += MMD_NT) arow[d] = g.xs[(size_t)r * D + d];
  } else {
    mmd_stage_y(arow, g.y, r - g.Bl, 1, D, g.k0, g.k1, step);
  }
  __syncthreads();
  const float gam = 1.f / (float)D;
  const bool want_grad = xrow && g.dz != nullptr;
  // gradient lanes: thread (q, d) = (tid >> 6, tid & 63) walks the staged rows j = q, q + 4, ...
  const int gd = tid & 63, gq = tid >> 6;
  double gxx = 0.0, gxy = 0.0, kxx = 0.0, kxy = 0.0;
  const int T = 8192 / D < MMD_T ? 8192 / D : MMD_T;
  // pass 0: against x (x rows only), pass 1: against y
  for (int pass = xrow ? 0 : 1; pass < 2; ++pass) {
    const int nrows = pass == 0 ? g.Bg : g.M;
    for (int c0 = 0; c0 < nrows; c0 += T) {
      const int nr = nrows - c0 < T ? nrows - c0 : T;
      if (pass == 0) {
        for (int e = tid; e < nr * D; e += MMD_NT) cb[e] = g.xall[(size_t)c0 * D + e];
      } else {
        mmd_stage_y(cb, g.y, c0, nr, D, g.k0, g.k1, step);
      }
      __syncthreads();
      for (int j = tid; j < nr; j += MMD_NT) {
        const float* b = cb + j * D;
        float s = 0.f, kv, w;
        if (g.kind == 0) {
          for (int d = 0; d < D; ++d) {
            const float t = arow[d] - b[d];
            s = fmaf(t, t, s);
          }
          kv = odin_exp(-s * gam);
          w = kv;
        } else {
          for (int d = 0; d < D; ++d) s += arow[d] - b[d];
          kv = fabsf(s);
          w = s > 0.f ? 1.f : (s < 0.f ? -1.f : 0.f);
        }
        if (pass == 0) kxx += (double)kv; else kxy += (double)kv;
        wk[j] = w;
      }
      __syncthreads();
      if (want_grad && gd < D) {
        double a = 0.0;
        const double ad = (double)arow[gd];
        if (g.kind == 0) {
          for (int j = gq; j < nr; j += 4) a += (double)wk[j] * (ad - (double)cb[j * D + gd]);
        } else {
          for (int j = gq; j < nr; j += 4) a += (double)wk[j];
        }
        if (pass == 0) gxx += a; else gxy += a;
      }
      __syncthreads();
    }
  }
  if (want_grad) {
    // d/dx_r of (1/Bg^2) sum k(x, x) - (2/(Bg M)) sum k(x, y): x_r sits on both sides of k(x, x)
    const double Bg = (double)g.Bg, M = (double)g.M;
    const double dk = g.kind == 0 ? -2.0 / (double)D : 1.0;
    const double cg = g.coef_grad != nullptr ? (double)g.coef_grad[0] : 1.0;
    // the four q-partials of each d meet in a fixed order
    red[tid] = (gd < D) ? (2.0 / (Bg * Bg)) * gxx - (2.0 / (Bg * M)) * gxy : 0.0;
    __syncthreads();
    if (tid < D) {
      const double v = (red[tid] + red[64 + tid]) + (red[128 + tid] + red[192 + tid]);
      g.dz[(size_t)r * D + tid] = (float)(cg * dk * v);
    }
    __syncthreads();
  }
  const double sxx = block_sum_d<MMD_NT>(kxx, red);
  const double sxy = block_sum_d<MMD_NT>(kxy, red);
  if (tid == 0) {
    const double Bg = (double)g.Bg, M = (double)g.M;
    const double part = xrow ? sxx / (Bg * Bg) - 2.0 * sxy / (Bg * M) : sxy / (M * M);
    // one atomic per workgroup: the share in 2^-32 units above a 13-bit arrival count; the old value names the last
    // arrival and, with its own share, the total (|MMD| < 2^18, at most 8191 workgroups)
    const long long fx = (long long)rint(part * MMD_FX);
    const unsigned long long mine = ((unsigned long long)fx << MMD_TB) + 1ull;
    const unsigned long long old = atomicAdd(g.acc, mine);
    if ((old & ((1ull << MMD_TB) - 1ull)) == (unsigned long long)gridDim.x - 1ull) {
      (void)atomicExch(g.acc, 0ull);
      const long long tot = (long long)(old + mine - (unsigned long long)gridDim.x) >> MMD_TB;
      const double cf = g.coef != nullptr ? (double)g.coef[0] : 1.0;
      g.out[0] = (float)(cf * ((double)tot / MMD_FX));
    }
  }
}

// ---- DIP ---------------------------------------------------------------------------------------------------------
// A moment block (one per rank): [n | mean[D] | M2[D][D] (centred: sum_i (mu_i - mean)(mu_i - mean)^T) | sum_i scale^2 [D]]
__host__ __device__ constexpr int dip_block(int D) { return 1 + 2 * D + D * D; }

// One workgroup: the moment block of rows p[0 .. N) (loc = p[:, :D], scale = softplus(p[:, D:])) into blk.
__device__ void dip_moments_body(const float* p, int N, int D, float* blk, double* red, double* mean, float* cs) {
  const int tid = threadIdx.x;
  const int G = DIP_NT / D;   // row groups of the column sums
  double s1 = 0.0, s2 = 0.0;
  if (tid < G * D) {
    const int d = tid % D, q = tid / D;
    for (int i = q; i < N; i += G) {
      s1 += (double)p[(size_t)i * 2 * D + d];
      const double sg = (double)softplus_r(p[(size_t)i * 2 * D + D + d]);
      s2 += sg * sg;
    }
  }
  red[tid] = s1;
  __syncthreads();
  if (tid < D) {
    double a = 0.0;
    for (int q = 0; q < G; ++q) a += red[q * D + tid];
    mean[tid] = a / (double)N;
  }
  __syncthreads();
  red[tid] = s2;
  __syncthreads();
  if (tid < D) {
    double a = 0.0;
    for (int q = 0; q < G; ++q) a += red[q * D + tid];
    blk[1 + D + D * D + tid] = (float)a;
    blk[1 + tid] = (float)mean[tid];
  }
  if (tid == 0) blk[0] = (float)N;
  __syncthreads();
  // centred second moments over pairs k <= l: slots = pairs x row replicas
  const int P = D * (D + 1) / 2;
  const int R = P >= DIP_NT ? 1 : DIP_NT / P;
  int sk[3], sl[3], nslot = 0, rep = 0;
  for (int s = tid; s < P * R && nslot < 3; s += DIP_NT) {
    int pr = s % P, k = 0;
    rep = s / P;
    while (pr >= D - k) { pr -= D - k; ++k; }
    sk[nslot] = k; sl[nslot] = k + pr; ++nslot;
  }
  double acc[3] = {0.0, 0.0, 0.0};
  const int T = (8192 / D) < DIP_T ? (8192 / D) : DIP_T;
  for (int c0 = 0; c0 < N; c0 += T) {
    const int nr = N - c0 < T ? N - c0 : T;
    for (int e = tid; e < nr * D; e += DIP_NT) {
      const int i = e / D, d = e - i * D;
      cs[e] = (float)((double)p[(size_t)(c0 + i) * 2 * D + d] - mean[d]);
    }
    __syncthreads();
    for (int u = 0; u < nslot; ++u) {
      double a = acc[u];
      const int k = sk[u], l = sl[u];
      for (int i = rep; i < nr; i += R) a += (double)cs[i * D + k] * (double)cs[i * D + l];
      acc[u] = a;
    }
    __syncthreads();
  }
  if (R == 1) {
    for (int u = 0; u < nslot; ++u) {
      const float v = (float)acc[u];
      blk[1 + D + sk[u] * D + sl[u]] = v;
      blk[1 + D + sl[u] * D + sk[u]] = v;
    }
  } else {
    red[tid] = nslot > 0 ? acc[0] : 0.0;
    __syncthreads();
    if (tid < P) {
      double a = 0.0;
      for (int q = 0; q < R; ++q) a += red[q * P + tid];
      const float v = (float)a;
      blk[1 + D + sk[0] * D + sl[0]] = v;
      blk[1 + D + sl[0] * D + sk[0]] = v;
    }
  }
  __syncthreads();
}

struct DipArgs {
  const float* blocks;   // [W][dip_block(D)]
  int W;
  const float* p;        // [Bl, 2D] this rank's rows
  int Bl, D, type2;
  float lam_diag, lam_off;
  const float* coef;
  const float* coef_grad;
  float* out;            // out[0] = coef * DIP (the whole batch's value: the same on every rank)
  float* dloc;           // [Bl, D] or NULL
  float* dscale;         // [Bl, D] or NULL (zeros for type I)
};

// One workgroup: combine the W blocks (Chan et al.: M2 = sum_r M2_r + n_r (mean_r - mean)(mean_r - mean)^T, in rank
// order), Cov = M2 / N (+ diag(sum scale^2 / N) for type II), the value, G = dvalue/dCov and the row gradients
//   dloc_i = (2/N) G (mu_i - mean),   dscale_ik = G_kk 2 scale_ik / N.
__device__ void dip_finish_body(const DipArgs& a, double* red, double* mean, float* Gs) {
  const int tid = threadIdx.x, D = a.D, bs = dip_block(D);
  double n = 0.0;
  for (int r = 0; r < a.W; ++r) n += (double)a.blocks[(size_t)r * bs];
  if (tid < D) {
    double m = 0.0;
    for (int r = 0; r < a.W; ++r) m += (double)a.blocks[(size_t)r * bs] * (double)a.blocks[(size_t)r * bs + 1 + tid];
    mean[tid] = m / n;
  }
  __syncthreads();
  double v = 0.0;
  for (int e = tid; e < D * D; e += DIP_NT) {
    const int k = e / D, l = e - k * D;
    double m2 = 0.0;
    for (int r = 0; r < a.W; ++r) {
      const float* b = a.blocks + (size_t)r * bs;
      const double nr = (double)b[0];
      m2 += (double)b[1 + D + e] + nr * ((double)b[1 + k] - mean[k]) * ((double)b[1 + l] - mean[l]);
    }
    double c = m2 / n;
    if (k == l && a.type2) {
      double ss = 0.0;
      for (int r = 0; r < a.W; ++r) ss += (double)a.blocks[(size_t)r * bs + 1 + D + D * D + k];
      c += ss / n;
    }
    double gkl;
    if (k == l) {
      v += (double)a.lam_diag * (c - 1.0) * (c - 1.0);
      gkl = 2.0 * (double)a.lam_diag * (c - 1.0);
    } else {
      v += (double)a.lam_off * c * c;
      gkl = 2.0 * (double)a.lam_off * c;
    }
    Gs[e] = (float)gkl;
  }
  const double val = block_sum_d<DIP_NT>(v, red);   // (also the barrier that publishes Gs)
  if (tid == 0 && a.out != nullptr) a.out[0] = (float)((a.coef != nullptr ? (double)a.coef[0] : 1.0) * val);
  const float cg = (a.coef_grad != nullptr ? a.coef_grad[0] : 1.f) * (float)(2.0 / n);
  for (int e = tid; e < a.Bl * D; e += DIP_NT) {
    const int i = e / D, k = e - i * D;
    const float* row = a.p + (size_t)i * 2 * D;
    if (a.dloc != nullptr) {
      float s = 0.f;
      for (int l = 0; l < D; ++l) s = fmaf(Gs[k * D + l], (float)((double)row[l] - mean[l]), s);
      a.dloc[e] = cg * s;
    }
    if (a.dscale != nullptr) a.dscale[e] = a.type2 ? cg * Gs[k * D + k] * softplus_r(row[D + k]) : 0.f;
  }
}

// LDS of the DIP kernels: red[DIP_NT] + mean[DIP_DMAX] doubles, then the centred chunk (8192 floats) / G (D*D floats)
constexpr size_t DIP_LDS = (DIP_NT + DIP_DMAX) * 8 + 8192 * 4;

__global__ __launch_bounds__(DIP_NT) void dip_moments_kernel(const float* p, int N, int D, float* blk) {
  ODIN_DYN_SMEM(double, sm);
  dip_moments_body(p, N, D, blk, sm, sm + DIP_NT, (float*)(sm + DIP_NT + DIP_DMAX));
}

__global__ __launch_bounds__(DIP_NT) void dip_finish_kernel(DipArgs a) {
  ODIN_DYN_SMEM(double, sm);
  dip_finish_body(a, sm, sm + DIP_NT, (float*)(sm + DIP_NT + DIP_DMAX));
}

// single device: moments into the workspace block, then the finish pass over that one block (same workgroup: the
// barrier that ends the moments orders the block's global stores before the finish reads them)
__global__ __launch_bounds__(DIP_NT) void dip_fused_kernel(DipArgs a, float* blk) {
  ODIN_DYN_SMEM(double, sm);
  dip_moments_body(a.p, a.Bl, a.D, blk, sm, sm + DIP_NT, (float*)(sm + DIP_NT + DIP_DMAX));
  dip_finish_body(a, sm, sm + DIP_NT, (float*)(sm + DIP_NT + DIP_DMAX));
}

}  // namespace

// ---- MMD ---------------------------------------------------------------------------------------------------------
// workspace (floats, zeroed once; every launch leaves it so): [0] = value | [1] spare | [2..3] the 64-bit
// accumulator | pad to 8
extern "C" int odin_mmd_workspace(int B_local, int B_global, int M, int D) {
  (void)B_local; (void)B_global; (void)M; (void)D;
  return 8;
}

static int mmd_launch(const float* xs, const float* xall, const float* y, float* ws, float* dz, const float* coef,
                      const float* coef_grad, int Bl, int Bg, int M, int D, int kernel, int include_yy,
                      uint64_t prior_seed, const int32_t* step_dev, void* stream) {
  if (kernel != 0 && kernel != 1) return odin_fail(-2, "mmd: kernel must be 0 (gaussian) or 1 (linear)");
  if (D < 1 || D > MMD_DMAX) return odin_fail(-2, "mmd: D outside [1, 64]");
  if (Bg < 1 || Bg > MMD_NMAX || Bl < 1 || Bl > Bg) return odin_fail(-2, "mmd: rows outside [1, 4096]");
  if (M < 1 || M > MMD_MMAX) return odin_fail(-2, "mmd: prior samples outside [1, 512]");
  if (ws == nullptr || xs == nullptr || xall == nullptr) return odin_fail(-2, "mmd: null argument");
  if ((((size_t)ws) & 7) != 0) return odin_fail(-2, "mmd: workspace must be 8-byte aligned");
  MmdArgs g;
  g.xs = xs; g.xall = xall; g.y = y;
  g.Bl = Bl; g.Bg = Bg; g.M = M; g.D = D; g.kind = kernel; g.include_yy = include_yy;
  g.k0 = (unsigned)prior_seed; g.k1 = (unsigned)(prior_seed >> 32);
  g.step_dev = (const int*)step_dev;
  g.coef = coef; g.coef_grad = coef_grad; g.dz = dz; g.out = ws;
  g.acc = reinterpret_cast<unsigned long long*>(ws + 2);
  const int grid = Bl + (include_yy ? M : 0);
  ODIN_LAUNCH(mmd_rows_kernel, dim3(grid), dim3(MMD_NT), 0, stream, g);
  return odin_check_launch("mmd");
}

extern "C" int odin_mmd_fwd_bwd(const float* x, const float* y, float* ws, float* dz, const float* coef,
                                const float* coef_grad, int N, int M, int D, int kernel, uint64_t prior_seed,
                                const int32_t* step_dev, void* stream) {
  return mmd_launch(x, x, y, ws, dz, coef, coef_grad, N, N, M, D, kernel, 1, prior_seed, step_dev, stream);
}

extern "C" int odin_mmd_shard(const float* x_local, const float* x_all, const float* y, float* ws, float* dz_local,
                              const float* coef, const float* coef_grad, int B_local, int B_global, int M, int D,
                              int kernel, int include_yy, uint64_t prior_seed, const int32_t* step_dev, void* stream) {
  return mmd_launch(x_local, x_all, y, ws, dz_local, coef, coef_grad, B_local, B_global, M, D, kernel, include_yy,
                    prior_seed, step_dev, stream);
}

// ---- DIP ---------------------------------------------------------------------------------------------------------
// workspace (floats): [0] = value | [1..3] spare | [4, 4 + bs) this rank's moment block | then W gathered blocks
extern "C" int odin_dip_workspace(int world, int D) {
  return 4 + (world + 1) * dip_block(D);
}

static int dip_check(int N, int D) {
  if (D < 1 || D > DIP_DMAX) return odin_fail(-2, "dip: D outside [1, 64]");
  if (N < 1) return odin_fail(-2, "dip: no rows");
  return 0;
}

static void dip_args(DipArgs& a, const float* p, int N, int D, int type2, float ld, float lo, const float* coef,
                     const float* coef_grad, float* out, float* dloc, float* dscale) {
  a.p = p; a.Bl = N; a.D = D; a.type2 = type2; a.lam_diag = ld; a.lam_off = lo;
  a.coef = coef; a.coef_grad = coef_grad; a.out = out; a.dloc = dloc; a.dscale = dscale;
}

extern "C" int odin_dip_fwd_bwd(const float* p, float* ws, float* dloc, float* dscale, const float* coef,
                                const float* coef_grad, int N, int D, int type2, float lambda_diag,
                                float lambda_offdiag, void* stream) {
  if (int rc = dip_check(N, D)) return rc;
  if (p == nullptr || ws == nullptr) return odin_fail(-2, "dip: null argument");
  DipArgs a;
  dip_args(a, p, N, D, type2, lambda_diag, lambda_offdiag, coef, coef_grad, ws, dloc, dscale);
  a.blocks = ws + 4;
  a.W = 1;
  ODIN_LAUNCH(dip_fused_kernel, dim3(1), dim3(DIP_NT), DIP_LDS, stream, a, ws + 4);
  return odin_check_launch("dip");
}

extern "C" int odin_dip_moments(const float* p_local, float* block, int B_local, int D, void* stream) {
  if (int rc = dip_check(B_local, D)) return rc;
  ODIN_LAUNCH(dip_moments_kernel, dim3(1), dim3(DIP_NT), DIP_LDS, stream, p_local, B_local, D, block);
  return odin_check_launch("dip_moments");
}

extern "C" int odin_dip_finish(const float* blocks, int world, const float* p_local, float* ws, float* dloc,
                               float* dscale, const float* coef, const float* coef_grad, int B_local, int D,
                               int type2, float lambda_diag, float lambda_offdiag, void* stream) {
  if (int rc = dip_check(B_local, D)) return rc;
  if (world < 1) return odin_fail(-2, "dip_finish: world < 1");
  DipArgs a;
  dip_args(a, p_local, B_local, D, type2, lambda_diag, lambda_offdiag, coef, coef_grad, ws, dloc, dscale);
  a.blocks = blocks;
  a.W = world;
  ODIN_LAUNCH(dip_finish_kernel, dim3(1), dim3(DIP_NT), DIP_LDS, stream, a);
  return odin_check_launch("dip_finish");
}
