// vq.hip -- the vector quantiser of VQVAE (odin/bay/distributions/vector_quantizer.py, odin/bay/vi/autoencoder/
// vq_vae.py; van den Oord et al. 2017): N codes c_n [Cs] against a codebook e [K, Cs],
//   idx_n = argmin_k sum_d (c_nd - e_kd)^2   (ties: the smallest k, tf.argmax of the negated distances)
//   z_q   = e[idx]                            (the value of the straight-through sample)
//   m     = mean over all N Cs elements of (c - z_q)^2      (commitment = weight * m, latents = m)
// and the backward half
//   dcodes    = (dz_q + 2 weight / (N Cs) (c - z_q)) * act'(c)         (straight through + commitment)
//   dcodebook = 2 / (N Cs) sum_{n: idx_n = k} (e_k - c_n)              (the `latents` term; codebook trained by gradient)
//   or the moving averages (ema_update=True): cnt_k, sum_k = sum c_n;  counts <- d counts + (1 - d) cnt,
//   means <- d means + (1 - d) sum, codebook <- means / (counts + epsilon)   (no zero-debias)
//
// odin_vq_assign, two launches:
//   assign: the codebook staged in LDS once per workgroup (row stride Cs | 1: lanes that walk different codes at the
//           same d hit different banks); a wave takes one code row at a time, lane l the codebook rows l, l + 64, ...;
//           the distance is sum (c - e)^2 in fp32 -- NOT |c|^2 - 2 c.e + |e|^2, which cancels; the argmin carries its
//           index through a butterfly over the wave's lanes ((distance, k) pairs: smaller distance, then smaller k;
//           no workgroup barrier inside the row loop); z_q is copied out of LDS and (c - z_q)^2 is summed per thread
//           in float64, the workgroup's total leaves as ONE double
//   finish: one workgroup sums the per-workgroup doubles in a fixed tree (m) and counts idx per code (integer LDS
//           atomics: exact, any order)
// odin_vq_bwd, two launches:
//   dcodes: elementwise, keeps the range word of its result
//   codes : one workgroup per codebook row k walks idx in chunks staged in LDS; thread (q, d) takes the rows
//           n = q, q + G, ... of a chunk and sums c_nd of the members in float64; the G partials meet in a fixed order
// No float atomics anywhere: two runs, and eager versus graph replay, give the same bits.
//
// Limits (checked in the entries): K <= 1024, Cs <= 256, K Cs 4 B <= 64 KB (the LDS budgeted for the codebook; the
// assign kernel's whole LDS image is at most 71 KB of the CU's 160), N <= 65536.
#include "odin_device.h"
#include "odin_internal.h"

namespace {

constexpr int VQ_NT = 256;
constexpr int VQ_KMAX = 1024;
constexpr int VQ_CSMAX = 256;
constexpr int VQ_NMAX = 65536;
constexpr int VQ_CB_BYTES = 64 * 1024;   // K * Cs * 4 within this
constexpr int VQ_GMAX = 256;             // workgroups of the assign launch (= per-workgroup partials of m)
constexpr int VQ_ROWS = VQ_NT / 64;      // code rows a workgroup holds at a time: one per wave
constexpr int VQ_CHUNK = 1024;           // idx entries a workgroup of the codes phase stages at a time

__host__ __device__ inline int vq_stride(int Cs) { return Cs | 1; }
inline int vq_grid(int N) {
  const int g = (N + VQ_ROWS - 1) / VQ_ROWS;
  return g < VQ_GMAX ? g : VQ_GMAX;
}
inline size_t vq_assign_lds(int K, int Cs) {
  return (size_t)VQ_NT * 8 + 64 + (size_t)VQ_ROWS * Cs * 4 + (size_t)K * vq_stride(Cs) * 4;
}

struct VqAssign {
  const float* codes;      // [N, Cs]
  const float* codebook;   // [K, Cs]
  int* idx;                // [N]
  float* zq;               // [N, Cs]
  double* part;            // [gridDim.x]
  unsigned* zq_amax;       // range word of z_q or NULL
  int N, K, Cs;
};

__global__ __launch_bounds__(VQ_NT) void vq_assign_kernel(VqAssign g) {
  ODIN_DYN_SMEM(unsigned char, smem);
  double* red = reinterpret_cast<double*>(smem);        // [VQ_NT]
  float* scr = reinterpret_cast<float*>(red + VQ_NT);   // [16] scratch of the range-word commit
  float* crow = scr + 16;                               // [VQ_ROWS][Cs] the rows in flight, one per wave
  float* cb = crow + VQ_ROWS * g.Cs;                    // [K][S]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int N = g.N, K = g.K, Cs = g.Cs, S = vq_stride(Cs);
  for (int e = tid; e < K * Cs; e += VQ_NT) {
    const int k = e / Cs, d = e - k * Cs;
    cb[k * S + d] = g.codebook[e];
  }
  __syncthreads();   // the codebook is staged; from here on a wave meets only itself
  double acc = 0.0;
  float amx = 0.f;
  const int per = VQ_ROWS * (int)gridDim.x;
  const int iters = (N + per - 1) / per;
  for (int it = 0; it < iters; ++it) {
    const int n = (it * (int)gridDim.x + (int)blockIdx.x) * VQ_ROWS + w;
    const bool live = n < N;   // (wave-uniform)
    odin_wave_sync();          // this wave is done with its previous row
    if (live)
      for (int d = lane; d < Cs; d += 64) crow[w * Cs + d] = g.codes[(size_t)n * Cs + d];
    odin_wave_sync();
    float bd = INFINITY;
    int bk = K;   // (no candidate: a lane beyond K, or distances that are all inf / NaN)
    if (live) {
      const float* c = crow + w * Cs;
      for (int k = lane; k < K; k += 64) {
        const float* e = cb + k * S;
        float s = 0.f;
        for (int d = 0; d < Cs; ++d) {
          const float t = c[d] - e[d];
          s = fmaf(t, t, s);
        }
        if (s < bd) { bd = s; bk = k; }   // (k ascends: the first minimum of this lane stays)
      }
    }
    // the wave's 64 (distance, k) pairs meet in a butterfly: smaller distance, then smaller k -- a total order, so
    // every lane ends with the same pair whatever the pairing; no LDS, no workgroup barrier
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const float od = __shfl_xor(bd, s);
      const int ok = __shfl_xor(bk, s);
      if (od < bd || (od == bd && ok < bk)) { bd = od; bk = ok; }
    }
    int best = bk;
    if (best >= K) best = 0;
    if (live) {
      if (lane == 0) g.idx[n] = best;
      for (int d = lane; d < Cs; d += 64) {
        const float e = cb[best * S + d];
        g.zq[(size_t)n * Cs + d] = e;
        const float t = crow[w * Cs + d] - e;
        acc += (double)t * (double)t;
        amx = fmaxf(amx, fabsf(e));
      }
    }
  }
  __syncthreads();
  red[tid] = acc;
  __syncthreads();
#pragma unroll 1
  for (int s = VQ_NT / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) g.part[blockIdx.x] = red[0];
  odin_amax_commit_wg(g.zq_amax, amx, tid, VQ_NT, scr, blockIdx.x);
}

// m = (sum of the G partials) / (N Cs) in a fixed tree; cnt[k] = #{n: idx_n = k}
__global__ __launch_bounds__(VQ_NT) void vq_finish_kernel(const double* part, int G, const int* idx, int N, int K,
                                                          double inv, float* m_out, int* cnt) {
  __shared__ double red[VQ_NT];
  __shared__ int hist[VQ_KMAX];
  const int tid = threadIdx.x;
  red[tid] = tid < G ? part[tid] : 0.0;
  __syncthreads();
#pragma unroll 1
  for (int s = VQ_NT / 2; s >= 1; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) m_out[0] = (float)(red[0] * inv);
  if (cnt == nullptr) return;   // (a kernel argument: uniform)
  for (int k = tid; k < K; k += VQ_NT) hist[k] = 0;
  __syncthreads();
  for (int n = tid; n < N; n += VQ_NT) {
    const int i = idx[n];
    if ((unsigned)i < (unsigned)K) (void)atomicAdd(&hist[i], 1);
  }
  __syncthreads();
  for (int k = tid; k < K; k += VQ_NT) cnt[k] = hist[k];
}

__global__ __launch_bounds__(VQ_NT) void vq_dcodes_kernel(const float* codes, const float* zq, const float* dzq,
                                                          float* dcodes, size_t n, float coef, int act,
                                                          unsigned* amax) {
  __shared__ float red[16];
  const int tid = threadIdx.x;
  float amx = 0.f;
  for (size_t i = (size_t)blockIdx.x * VQ_NT + tid; i < n; i += (size_t)gridDim.x * VQ_NT) {
    const float c = codes[i];
    const float v = (dzq[i] + coef * (c - zq[i])) * odin_act_grad(act, c);
    dcodes[i] = v;
    amx = fmaxf(amx, fabsf(v));
  }
  odin_amax_commit_wg(amax, amx, tid, VQ_NT, red, blockIdx.x);
}

struct VqCodes {
  const float* codes;   // [N, Cs]
  const int* idx;       // [N]
  float* codebook;      // [K, Cs]: read; written under the moving average
  float* dcodebook;     // [K, Cs] or NULL
  float* ema_counts;    // [K] or NULL
  float* ema_means;     // [K, Cs] or NULL
  int N, K, Cs;
  int lg;               // log2 of the threads per row of a group: 2^lg >= Cs
  double scale;         // 2 / (N Cs)
  double decay, epsilon;
};

// codebook row k = blockIdx.x against every assignment
__global__ __launch_bounds__(VQ_NT) void vq_codes_kernel(VqCodes g) {
  __shared__ int idx_s[VQ_CHUNK];
  __shared__ double red[VQ_NT];
  __shared__ int cnt_s[VQ_NT];
  const int tid = threadIdx.x, k = blockIdx.x, N = g.N, Cs = g.Cs;
  const int W = 1 << g.lg, G = VQ_NT >> g.lg;   // threads per row | rows in flight
  const int q = tid >> g.lg, d = tid & (W - 1);
  const bool ema = g.ema_counts != nullptr;
  const double oc = ema ? (double)g.ema_counts[k] : 0.0;   // (read by every thread before thread 0 overwrites it)
  double sum = 0.0;
  int cnt = 0;
  for (int n0 = 0; n0 < N; n0 += VQ_CHUNK) {
    __syncthreads();
    for (int j = tid; j < VQ_CHUNK; j += VQ_NT) idx_s[j] = n0 + j < N ? g.idx[n0 + j] : -1;
    __syncthreads();
    const int lim = N - n0 < VQ_CHUNK ? N - n0 : VQ_CHUNK;
    for (int j = q; j < lim; j += G) {
      if (idx_s[j] == k) {
        ++cnt;
        if (d < Cs) sum += (double)g.codes[(size_t)(n0 + j) * Cs + d];
      }
    }
  }
  red[tid] = sum;
  cnt_s[tid] = cnt;
  __syncthreads();
  if (tid < Cs) {   // (Cs <= W: thread (0, d))
    double s = 0.0;
    int c = 0;
    for (int r = 0; r < G; ++r) {
      s += red[r * W + tid];
      c += cnt_s[r * W + tid];
    }
    const size_t o = (size_t)k * Cs + tid;
    if (g.dcodebook != nullptr) g.dcodebook[o] = (float)(g.scale * ((double)c * (double)g.codebook[o] - s));
    if (ema) {
      const float nc = (float)(g.decay * oc + (1.0 - g.decay) * (double)c);
      const float nm = (float)(g.decay * (double)g.ema_means[o] + (1.0 - g.decay) * s);
      g.ema_means[o] = nm;
      g.codebook[o] = (float)((double)nm / ((double)nc + g.epsilon));
      if (tid == 0) g.ema_counts[k] = nc;
    }
  }
}

int vq_check_dims(const char* who, int N, int K, int Cs) {
  static char msg[96];
  const char* what = nullptr;
  if (N < 1 || N > VQ_NMAX) what = "N outside [1, 65536]";
  else if (K < 1 || K > VQ_KMAX) what = "K outside [1, 1024]";
  else if (Cs < 1 || Cs > VQ_CSMAX) what = "Cs outside [1, 256]";
  else if ((size_t)K * Cs * 4 > (size_t)VQ_CB_BYTES) what = "K * Cs * 4 bytes beyond the 64 KB of LDS for the codebook";
  if (what == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return odin_fail(-2, msg);
}

}  // namespace

// workspace in floats (8-byte aligned, no initialisation needed): the per-workgroup float64 partials of m
extern "C" int odin_vq_workspace(int N) {
  if (N < 1) return 0;
  return 2 * vq_grid(N < VQ_NMAX ? N : VQ_NMAX);
}

extern "C" int odin_vq_assign(const float* codes, const float* codebook, int32_t* idx, float* z_q, float* ws,
                              float* m_out, int32_t* cnt, uint32_t* zq_amax, int N, int K, int Cs, void* stream) {
  if (int rc = vq_check_dims("vq_assign", N, K, Cs)) return rc;
  if (codes == nullptr || codebook == nullptr || idx == nullptr || z_q == nullptr || ws == nullptr || m_out == nullptr)
    return odin_fail(-2, "vq_assign: null argument");
  if ((((size_t)ws) & 7) != 0) return odin_fail(-2, "vq_assign: workspace must be 8-byte aligned");
  VqAssign g;
  g.codes = codes; g.codebook = codebook; g.idx = idx; g.zq = z_q;
  g.part = reinterpret_cast<double*>(ws); g.zq_amax = zq_amax;
  g.N = N; g.K = K; g.Cs = Cs;
  const int G = vq_grid(N);
  const size_t lds = vq_assign_lds(K, Cs);
#ifndef ODIN_SIM
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&vq_assign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds) != hipSuccess)
    return odin_fail(-4, "vq_assign: cannot raise the dynamic LDS limit");
#endif
  ODIN_LAUNCH(vq_assign_kernel, dim3(G), dim3(VQ_NT), lds, stream, g);
  if (int rc = odin_check_launch("vq_assign")) return rc;
  ODIN_LAUNCH(vq_finish_kernel, dim3(1), dim3(VQ_NT), 0, stream, (const double*)g.part, G, (const int*)idx, N, K,
              1.0 / ((double)N * (double)Cs), m_out, cnt);
  return odin_check_launch("vq_finish");
}

extern "C" int odin_vq_bwd(const float* codes, const float* z_q, const int32_t* idx, const float* dz_q,
                           float* codebook, float* dcodes, float* dcodebook, float* ema_counts, float* ema_means,
                           float commitment, double decay, double epsilon, int act, uint32_t* dcodes_amax, int N,
                           int K, int Cs, void* stream) {
  if (int rc = vq_check_dims("vq_bwd", N, K, Cs)) return rc;
  if (codes == nullptr || z_q == nullptr || idx == nullptr || dz_q == nullptr || codebook == nullptr ||
      dcodes == nullptr)
    return odin_fail(-2, "vq_bwd: null argument");
  if ((ema_counts == nullptr) != (ema_means == nullptr)) return odin_fail(-2, "vq_bwd: ema_counts and ema_means go together");
  if (dcodebook != nullptr && ema_counts != nullptr)
    return odin_fail(-2, "vq_bwd: the codebook is trained by gradient OR by the moving average");
  if (act < 0 || act > 2) return odin_fail(-2, "vq_bwd: unknown activation");
  const size_t n = (size_t)N * Cs;
  const double scale = 2.0 / ((double)N * (double)Cs);
  size_t blocks = (n + VQ_NT - 1) / VQ_NT;
  if (blocks > 1024) blocks = 1024;
  ODIN_LAUNCH(vq_dcodes_kernel, dim3((unsigned)blocks), dim3(VQ_NT), 0, stream, codes, z_q, dz_q, dcodes, n,
              (float)((double)commitment * scale), act, (unsigned*)dcodes_amax);
  if (int rc = odin_check_launch("vq_dcodes")) return rc;
  if (dcodebook == nullptr && ema_counts == nullptr) return 0;
  VqCodes g;
  g.codes = codes; g.idx = idx; g.codebook = codebook; g.dcodebook = dcodebook;
  g.ema_counts = ema_counts; g.ema_means = ema_means;
  g.N = N; g.K = K; g.Cs = Cs;
  g.lg = 0;
  while ((1 << g.lg) < Cs) ++g.lg;
  g.scale = scale; g.decay = decay; g.epsilon = epsilon;
  ODIN_LAUNCH(vq_codes_kernel, dim3(K), dim3(VQ_NT), 0, stream, g);
  return odin_check_launch("vq_codes");
}
