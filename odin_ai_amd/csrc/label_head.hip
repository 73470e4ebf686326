// label_head.hip -- the semi-supervised label head of MultitaskVAE / SkiptaskVAE (odin/bay/vi/autoencoder/
// multitask_vae.py:164-207): labels = RVconf(K, 'onehot', projection=True) is Dense(D -> K) giving the logits of a
// OneHotCategorical over a FRESH sample of the posterior (predict_labels calls z.sample(()), multitask_vae.py:106):
//   z' = loc + softplus(raw) eps_y                      (p [B, 2 D] = (loc | raw); noise of its own, not the decoder's z)
//   l  = z' W + b                                       (W [D, K] row-major: a Dense kernel)
//   llk_b = sum_k y_k (l_k - logsumexp(l))              (TFP's OneHotCategorical._log_prob: valid for soft labels too)
//   g_k = y_k - softmax_k sum_j y_j;  dz' = W g
// The loss term is coef' * mean_b llk_b; with c = coef[0] (a DEVICE scalar: -alpha / Bs on a labelled step):
//   dloc = c dz',  dscale = c dz' eps_y   (gradient with respect to the scale softplus(raw), as odin_total_correlation_fwd_bwd
//   hands its tc_dloc / tc_dscale to odin_latent_bwd),  dW = c sum_b z'_b g_b^T,  db = c sum_b g_b.
// ONE WAVE per sample, four samples per workgroup.  Lane j owns columns j, j + 64, j + 128, j + 192 of the logits (k
// ascending over the rows of W: coalesced reads of a row, through L2 -- a 255 x 255 W does not fit LDS beside anything
// else) and, for dz', rows j, j + 64, ... of W (k ascending).  z' and c g of the workgroup's four samples sit in LDS
// (handed from lane to lane across workgroup barriers, all of them in uniform control flow);
// after every round of four the 256 threads add the round's outer products to the workgroup's OWN slab row, each thread
// its own elements, waves ascending: no float atomics, every sum in a fixed order, two calls give the same bits.
// A workgroup owns a chunk of max(4, ceil(Bs / 32) rounded up to 4) samples: at most 32 slab rows.
// The batch mean: every workgroup takes a ticket (an integer atomic) once its llk values are out; the one that draws
// the last ticket sums llk[0 .. Bs) in a fixed order -- whichever workgroup that is -- writes value[0] and puts the
// ticket word back to zero.
// The rows of dloc / dscale outside [row0, row0 + Bs) are zeroed by the same launch (grid-stride).
// Limits (checked in the entries): 1 <= D <= 255, 1 <= K <= 255, 1 <= Bs, 0 <= row0, row0 + Bs <= B.
#include <cmath>

#include "odin_device.h"
#include "odin_internal.h"

namespace {

constexpr int LH_NT = 256;
constexpr int LH_SPW = LH_NT / 64;   // samples per round: one per wave
constexpr int LH_MAX = 255;          // D and K
constexpr int LH_PAD = 256;
constexpr int LH_ROWS = 32;          // at most this many workgroups (= slab rows)

struct LHParams {
  const float* p;       // [B, 2 D]
  const float* eps;     // [Bs, D]
  const float* w;       // [D, K]
  const float* bias;    // [K]
  const float* y;       // [Bs, K]
  const float* coef;    // device scalar
  float* logits;        // [Bs, K] or null
  float* llk;           // [Bs]
  float* value;         // [2]: the mean | the ticket word
  float* dloc;          // [B, D]
  float* dscale;        // [B, D]
  float* slab;          // [rows][D K + K]
  int B, row0, Bs, D, K, chunk;
};

__device__ __forceinline__ float lh_softplus(float v) { return fmaxf(v, 0.f) + log1pf(expf(-fabsf(v))); }

__device__ __forceinline__ float lh_wave_max64(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// the logits of one sample: lane owns columns lane + 64 j; zs = its z' in LDS; rows of W ascending, then the bias
__device__ __forceinline__ void lh_logits(const float* zs, const float* __restrict__ w, const float* __restrict__ bias,
                                          int D, int K, int lane, float (&l)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) l[j] = 0.f;
  // (four rows of W requested together, then used in order: the sum runs d ascending, the loads do not wait for one
  // another -- one dependent L2 round trip per row measured 14 us at D = 32)
  const int nj = (K + 63) >> 6;
  int d = 0;
  for (; d + 4 <= D; d += 4) {
    float wv[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        wv[u][j] = (j < nj && k < K) ? w[(size_t)(d + u) * K + k] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float zv = zs[d + u];   // (the same address in every lane)
#pragma unroll
      for (int j = 0; j < 4; ++j) l[j] = fmaf(zv, wv[u][j], l[j]);
    }
  }
  for (; d < D; ++d) {
    const float zv = zs[d];
    const float* wr = w + (size_t)d * K;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = lane + 64 * j;
      if (k < K) l[j] = fmaf(zv, wr[k], l[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = lane + 64 * j;
    if (k < K) l[j] += bias != nullptr ? bias[k] : 0.f;
  }
}

__global__ __launch_bounds__(LH_NT) void label_head_fwd_bwd_kernel(LHParams a) {
  __shared__ float zs[LH_SPW * LH_PAD];
  __shared__ float gs[LH_SPW * LH_PAD];
  __shared__ float red[LH_SPW];
  __shared__ int last_sh;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int D = a.D, K = a.K, Bs = a.Bs;
  // ---- the rows outside the labelled block: zero, every launch ----
  {
    const size_t n0 = (size_t)a.row0 * D, n1 = (size_t)(a.B - a.row0 - Bs) * D, skip = (size_t)Bs * D;
    const size_t stride = (size_t)gridDim.x * LH_NT;
    for (size_t e = (size_t)blockIdx.x * LH_NT + tid; e < n0 + n1; e += stride) {
      const size_t o = e < n0 ? e : e + skip;
      a.dloc[o] = 0.f;
      a.dscale[o] = 0.f;
    }
  }
  const float c = a.coef[0];
  const int c0 = blockIdx.x * a.chunk;
  const int cn = Bs - c0 < a.chunk ? Bs - c0 : a.chunk;   // (> 0: the grid is ceil(Bs / chunk))
  float* __restrict__ row = a.slab + (size_t)blockIdx.x * ((size_t)D * K + K);
  float* zw = zs + wv * LH_PAD;
  float* gw = gs + wv * LH_PAD;
  for (int s0 = 0; s0 < cn; s0 += LH_SPW) {
    const int bs = c0 + s0 + wv;          // this wave's sample within the labelled block
    const bool active = s0 + wv < cn;     // (wave-uniform: a wave meets only itself inside)
    __syncthreads();                      // (the round before this one has been read)
    const size_t r = (size_t)a.row0 + (active ? bs : 0);
    float ev[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const float* pb = a.p + r * 2 * D;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if (d < D) {
          ev[j] = a.eps[(size_t)bs * D + d];
          zw[d] = fmaf(lh_softplus(pb[D + d]), ev[j], pb[d]);
        }
      }
    } else {
      for (int i = lane; i < LH_PAD; i += 64) { zw[i] = 0.f; gw[i] = 0.f; }
    }
    __syncthreads();
    if (active) {
      float l[4], yv[4];
      lh_logits(zw, a.w, a.bias, D, K, lane, l);
      float mx = -3.0e38f, sy = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        yv[j] = 0.f;
        if (k < K) {
          yv[j] = a.y[(size_t)bs * K + k];
          mx = fmaxf(mx, l[j]);
          sy += yv[j];
          if (a.logits != nullptr) a.logits[(size_t)bs * K + k] = l[j];
        }
      }
      mx = lh_wave_max64(mx);
      sy = wave_sum64(sy);
      float ex[4], se = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ex[j] = lane + 64 * j < K ? expf(l[j] - mx) : 0.f;
        se += ex[j];
      }
      se = wave_sum64(se);   // (>= 1: the maximum contributes exp(0))
      const float lse = mx + logf(se), inv = 1.f / se;
      float ll = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        if (k < K) {
          ll = fmaf(yv[j], l[j] - lse, ll);
          gw[k] = c * (yv[j] - ex[j] * inv * sy);
        }
      }
      ll = wave_sum64(ll);
      if (lane == 0) {
        a.llk[bs] = ll;
        __threadfence();   // (out before this workgroup takes its ticket)
      }
    }
    __syncthreads();
    if (active) {
      // dz' = W (c g): lane owns rows lane + 64 j of W, columns ascending
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if (d < D) {
          const float* wr = a.w + (size_t)d * K;
          float acc = 0.f;
          int k = 0;
          for (; k + 8 <= K; k += 8) {   // (eight loads in flight, the sum k ascending)
            float w8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) w8[u] = wr[k + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(w8[u], gw[k + u], acc);
          }
          for (; k < K; ++k) acc = fmaf(wr[k], gw[k], acc);
          a.dloc[r * D + d] = acc;
          a.dscale[r * D + d] = acc * ev[j];
        }
      }
    }
    // ---- the round's share of (dW | db) into this workgroup's slab row: waves ascending ----
    const bool first = s0 == 0;
    const int nw = D * K;
    int d = tid / K, k = tid - d * K;
    const int dd = LH_NT / K, dk = LH_NT - dd * K;
    for (int e = tid; e < nw; e += LH_NT) {
      float v = zs[d] * gs[k];
      v = fmaf(zs[LH_PAD + d], gs[LH_PAD + k], v);
      v = fmaf(zs[2 * LH_PAD + d], gs[2 * LH_PAD + k], v);
      v = fmaf(zs[3 * LH_PAD + d], gs[3 * LH_PAD + k], v);
      row[e] = first ? v : row[e] + v;   // (this thread's own element: rounds ascending)
      d += dd; k += dk;
      if (k >= K) { k -= K; ++d; }
    }
    if (tid < K) {
      const float v = ((gs[tid] + gs[LH_PAD + tid]) + gs[2 * LH_PAD + tid]) + gs[3 * LH_PAD + tid];
      row[nw + tid] = first ? v : row[nw + tid] + v;
    }
  }
  // ---- the batch mean, by the workgroup that draws the last ticket ----
  __syncthreads();
  unsigned* ticket = reinterpret_cast<unsigned*>(a.value + 1);
  if (tid == 0) {
    __threadfence();
    last_sh = atomicAdd(ticket, 1u) + 1u == gridDim.x ? 1 : 0;
  }
  __syncthreads();
  if (!last_sh) return;   // (uniform over the workgroup)
  __threadfence();
  const volatile float* lv = a.llk;
  float acc = 0.f;
  for (int i = tid; i < Bs; i += LH_NT) acc += lv[i];
  acc = wave_sum64(acc);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  if (tid == 0) {
    a.value[0] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)Bs;
    *ticket = 0u;
  }
}

// the forward half from a given z [n, D]
__global__ __launch_bounds__(LH_NT) void label_head_fwd_kernel(const float* z, const float* w, const float* bias,
                                                               float* logits, int n, int D, int K) {
  __shared__ float zs[LH_SPW * LH_PAD];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t b = (size_t)blockIdx.x * LH_SPW + wv;
  const bool active = b < (size_t)n;   // (wave-uniform)
  float* zw = zs + wv * LH_PAD;
  if (active)
    for (int d = lane; d < D; d += 64) zw[d] = z[b * D + d];
  __syncthreads();
  if (!active) return;
  float l[4];
  lh_logits(zw, w, bias, D, K, lane, l);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = lane + 64 * j;
    if (k < K) logits[b * K + k] = l[j];
  }
}

int lh_check(const char* who, long long B, long long row0, long long Bs, int D, int K) {
  static thread_local char msg[192];
  const char* why = nullptr;
  if (D < 1 || D > LH_MAX) why = "1 <= D <= 255";
  else if (K < 1 || K > LH_MAX) why = "1 <= K <= 255";
  else if (Bs < 1) why = "1 <= Bs";
  else if (row0 < 0 || row0 + Bs > B) why = "0 <= row0, row0 + Bs <= B";
  if (why == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: outside its limits (%s): B = %lld, row0 = %lld, Bs = %lld, D = %d, K = %d", who, why, B,
           row0, Bs, D, K);
  return odin_fail(-2, msg);
}

}  // namespace

extern "C" int odin_label_head_fwd_bwd(const float* p, const float* eps_y, const float* w, const float* bias,
                                       const float* y, const float* coef, float* logits, float* llk, float* value,
                                       float* dloc, float* dscale, float* slab, int* slab_rows_out, int B, int row0,
                                       int Bs, int D, int K, void* stream) {
  if (int rc = lh_check("label_head_fwd_bwd", B, row0, Bs, D, K)) return rc;
  int chunk = (Bs + LH_ROWS - 1) / LH_ROWS;
  chunk = (chunk + LH_SPW - 1) / LH_SPW * LH_SPW;
  const int rows = (Bs + chunk - 1) / chunk;
  // (a real call with a missing operand touches no output either: checked ahead of the row count)
  if (slab != nullptr && (p == nullptr || eps_y == nullptr || w == nullptr || y == nullptr || coef == nullptr ||
                          llk == nullptr || value == nullptr || dloc == nullptr || dscale == nullptr))
    return odin_fail(-2, "label_head_fwd_bwd: null argument");
  if (slab_rows_out) *slab_rows_out = rows;
  if (slab == nullptr) return 0;   // dry run
  LHParams a;
  a.p = p; a.eps = eps_y; a.w = w; a.bias = bias; a.y = y; a.coef = coef; a.logits = logits; a.llk = llk; a.value = value;
  a.dloc = dloc; a.dscale = dscale; a.slab = slab;
  a.B = B; a.row0 = row0; a.Bs = Bs; a.D = D; a.K = K; a.chunk = chunk;
  ODIN_LAUNCH(label_head_fwd_bwd_kernel, dim3(rows), dim3(LH_NT), 0, stream, a);
  return odin_check_launch("label_head_fwd_bwd");
}

extern "C" int odin_label_head_fwd(const float* z, const float* w, const float* bias, float* logits, int n, int D, int K,
                                   void* stream) {
  if (int rc = lh_check("label_head_fwd", n, 0, n, D, K)) return rc;
  if (z == nullptr || w == nullptr || logits == nullptr) return odin_fail(-2, "label_head_fwd: null argument");
  ODIN_LAUNCH(label_head_fwd_kernel, dim3((unsigned)((n + LH_SPW - 1) / LH_SPW)), dim3(LH_NT), 0, stream, z, w, bias,
              logits, n, D, K);
  return odin_check_launch("label_head_fwd");
}
