// stage2.hip -- the two skip heads of TwoStageVAE's second stage (Dai & Wipf; two_stage_vae.py, layers/latents.py:23-45).
//
// encoder2 and decoder2 end in Concatenate([input, last hidden]) -> Dense(2 E): a projection over K = Dx + H columns
// (1034 on dSprites) that is thin on the other side as well (N = 2 E, 12 to 90).  Materialised, the [B, Dx + H] row costs
// a copy and lands on the small-GEMM family; here the two operands stay where they are:
//   p[b, n] = sum_{k < Dx} x[b, k] W[k, n] + sum_{k < H} h[b, k] W[Dx + k, n] + bias[n]
// W (up to 4224 x 256 floats) does not fit LDS: every kernel walks it in TILES of kt = min(512, 8192 / N) & ~3 rows -- a flat,
// contiguous run of kt N floats, fetched with independent coalesced loads (16 bytes per lane where W is so aligned) into
// registers while the tile before it is being used (the first version read W per thread, one dependent L2 round trip
// after the other: 18 to 60 us forward, 28 to 119 us backward at B = 256).
// forward  grid = ceil(B / 4): a workgroup owns 4 rows.  Thread = (column n, k-slice s) with NPAD = N rounded up to a
//          power of two and KS = 256 / NPAD slices of a tile; a thread sums its k ascending over the tiles, the slices are
//          added ascending by one thread per (row, column): fixed order, no atomics.
//          mode 1 (Observation2 as a likelihood): N = 2 E, the same launch evaluates
//            llk[b] = sum_e log N(t[b, e]; p[b, e], softplus(p[b, E + e]))  and  dp = -scale[0] dllk/dp
// backward grid = (slab rows, 2): a workgroup owns a chunk of rows, 8 at a time, in one of two roles.
//          y = 0  dx / dh: W tile in LDS with rows padded to N + 1 (a thread owns a row: odd stride, no bank conflicts),
//                 thread = (row k, column slice q); the slices are added ascending; dh times act'(h), max |dh| into the
//                 range word
//          y = 1  (dW | db): needs no W.  Thread = (column n, k-slice) with its 8 dp values in registers; the 8 inputs of a
//                 k come from LDS as two 16-byte broadcasts; stores are coalesced along n.  One slab row per workgroup,
//                 summed by odin_slab_reduce.
#include "odin_device.h"
#include "odin_internal.h"

namespace {

constexpr int SH_DMAX = 128;   // Dx and E = N / 2
constexpr int SH_HMAX = 4096;
constexpr int SH_RB = 4;       // forward: rows per workgroup
constexpr int SH_BR = 8;       // backward: rows per round
constexpr int SH_ROWS = 32;    // backward: at most this many workgroups per role (= slab rows)
constexpr int SH_WT = 8192;    // floats of W per tile (32 per thread)
constexpr int SH_KT = 512;     // at most this many rows of W per tile
constexpr int SH_KC = 1024;    // weight gradient: columns of the concatenated row staged per round
constexpr float SH_HALF_LOG2PI = 0.91893853320467274178f;

struct SHParams {
  const float* x;       // [B, Dx]
  const float* h;       // [B, H]
  const float* w;       // [Dx + H, N]
  const float* bias;    // [N]
  float* p;             // [B, N]
  const float* target;  // [B, E] (mode 1)
  const float* scale;   // device scalar (mode 1)
  float* llk;           // [B] (mode 1)
  float* dp;            // [B, N]: written in forward mode 1, read by the backward
  float* dh;            // [B, H]
  float* dx;            // [B, Dx] or null
  float* slab;          // [rows][(Dx + H) N + N]
  unsigned* dh_amax;
  int B, Dx, H, N, mode, h_act, chunk;
  int npad, lg;         // columns rounded up to a power of two; thread = (n = tid & (npad - 1), s = tid >> lg)
  int kt, kper;         // rows of W per tile; forward: rows of a tile per k-slice (a multiple of 4)
  int kl, lgk, cper;    // backward y = 0: row lanes (a power of two <= 256), columns per column slice
};

__device__ __forceinline__ float sh_softplus(float v) { return fmaxf(v, 0.f) + log1pf(odin_exp(-fabsf(v))); }
__device__ __forceinline__ float sh_sigmoid(float v) {
  const float e = odin_exp(-fabsf(v)), s = 1.f / (1.f + e);
  return v >= 0.f ? s : e * s;
}
// element k of row b of Concatenate([x, h]) (one load through a selected address)
__device__ __forceinline__ float sh_cat(const SHParams& p, int b, int k) {
  const float* src = k < p.Dx ? p.x + (size_t)b * p.Dx + k : p.h + (size_t)b * p.H + (k - p.Dx);
  return *src;
}
// `cnt` consecutive floats of W into registers.  V4 (src 16-byte aligned, cnt >= 4): 16-byte loads, floats
// 4 (tid + 256 j) .. + 3 in wreg[4 j ..], the cnt & 3 floats behind the last whole quad in `wtail` of threads 0 .. 2 --
// a dword per lane moved 14 GB/s per CU out of L2 here, a quad per lane is the form the cache path is built for.
// Otherwise float tid + 256 j in wreg[j].  Clamped copies beyond cnt: every load is unconditional, all are in flight
// together.
template <bool V4>
__device__ __forceinline__ void sh_fetch_w(const float* __restrict__ src, int cnt, int tid, float (&wreg)[32], float& wtail) {
  if (V4 && cnt >= 4) {
    const int n4 = cnt >> 2, t = cnt & 3;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e4 = tid + 256 * j;
      const float4 v = reinterpret_cast<const float4*>(src)[e4 < n4 ? e4 : n4 - 1];
      wreg[4 * j] = v.x; wreg[4 * j + 1] = v.y; wreg[4 * j + 2] = v.z; wreg[4 * j + 3] = v.w;
    }
    wtail = src[(t > 0 && tid < t) ? 4 * n4 + tid : cnt - 1];
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const int e = tid + 256 * j;
      wreg[j] = src[e < cnt ? e : cnt - 1];
    }
    wtail = 0.f;
  }
}
// the registers of sh_fetch_w into a flat LDS tile
template <bool V4>
__device__ __forceinline__ void sh_store_flat(float* wt, int cnt, int tid, const float (&wreg)[32], float wtail) {
  if (V4 && cnt >= 4) {
    const int n4 = cnt >> 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e4 = tid + 256 * j;
      if (e4 < n4) *reinterpret_cast<float4*>(wt + 4 * e4) = make_float4(wreg[4 * j], wreg[4 * j + 1], wreg[4 * j + 2], wreg[4 * j + 3]);
    }
    if (tid < (cnt & 3)) wt[4 * n4 + tid] = wtail;
  } else {
#pragma unroll
    for (int j = 0; j < 32; ++j) wt[tid + 256 * j] = wreg[j];
  }
}
// ... and into a tile whose rows of N floats are N + 1 apart
template <bool V4>
__device__ __forceinline__ void sh_store_padded(float* wt, int cnt, int N, int tid, const float (&wreg)[32], float wtail) {
  const int NP = N + 1;
  if (V4 && cnt >= 4) {
    const int n4 = cnt >> 2, dk = 1024 / N, dc = 1024 - dk * N;   // a step of 1024 elements in (row, column)
    int kk = (4 * tid) / N, c = 4 * tid - kk * N;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (tid + 256 * j < n4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int cc = c + i, kq = kk;
          if (cc >= N) { cc -= N; ++kq; }
          if (cc >= N) { cc -= N; ++kq; }   // (N = 2: a quad spans two rows)
          wt[kq * NP + cc] = wreg[4 * j + i];
        }
      }
      kk += dk; c += dc;
      if (c >= N) { c -= N; ++kk; }
    }
    if (tid < (cnt & 3)) {
      const int e = 4 * n4 + tid, tk = e / N;
      wt[tk * NP + (e - tk * N)] = wtail;
    }
  } else {
    const int dk = 256 / N, dc = 256 - dk * N;
    int kk = tid / N, c = tid - kk * N;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      if (tid + 256 * j < cnt) wt[kk * NP + c] = wreg[j];
      kk += dk; c += dc;
      if (c >= N) { c -= N; ++kk; }
    }
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void skip_head_fwd_kernel(SHParams p) {
  __shared__ __attribute__((aligned(16))) float wt[SH_WT];
  __shared__ __attribute__((aligned(16))) float xs[SH_RB * SH_KT];
  __shared__ float part[SH_RB * 256];
  __shared__ float ps[SH_RB * 2 * SH_DMAX];
  __shared__ float lls[SH_RB * SH_DMAX];
  const int tid = threadIdx.x, b0 = blockIdx.x * SH_RB;
  const int nb = p.B - b0 < SH_RB ? p.B - b0 : SH_RB;
  const int N = p.N, K = p.Dx + p.H, KT = p.kt;
  const int n = tid & (p.npad - 1), s = tid >> p.lg, KS = 256 >> p.lg;
  const int nt = (K + KT - 1) / KT;
  float acc[SH_RB], wreg[32], xreg[SH_RB * 2], wtail;
#pragma unroll
  for (int r = 0; r < SH_RB; ++r) acc[r] = 0.f;
  int ktc = K < KT ? K : KT;   // rows of the tile held in registers
  sh_fetch_w<V4>(p.w, ktc * N, tid, wreg, wtail);
#pragma unroll
  for (int r = 0; r < SH_RB; ++r)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = tid + 256 * j;
      xreg[2 * r + j] = sh_cat(p, b0 + (r < nb ? r : nb - 1), k < ktc ? k : ktc - 1);
    }
  for (int i = 0; i < nt; ++i) {
    const int kt = ktc;
    __syncthreads();   // (the tile before this one has been read)
    sh_store_flat<V4>(wt, kt * N, tid, wreg, wtail);
#pragma unroll
    for (int r = 0; r < SH_RB; ++r)
#pragma unroll
      for (int j = 0; j < 2; ++j) xs[r * SH_KT + tid + 256 * j] = xreg[2 * r + j];
    __syncthreads();
    if (i + 1 < nt) {   // the next tile travels while this one is used
      const int k1 = (i + 1) * KT;
      ktc = K - k1 < KT ? K - k1 : KT;
      sh_fetch_w<V4>(p.w + (size_t)k1 * N, ktc * N, tid, wreg, wtail);
#pragma unroll
      for (int r = 0; r < SH_RB; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = tid + 256 * j;
          xreg[2 * r + j] = sh_cat(p, b0 + (r < nb ? r : nb - 1), k1 + (k < ktc ? k : ktc - 1));
        }
    }
    if (n < N) {
      const int kbeg = s * p.kper, kend = kbeg + p.kper < kt ? kbeg + p.kper : kt;
      int k = kbeg;
      for (; k + 4 <= kend; k += 4) {
        const float w0 = wt[k * N + n], w1 = wt[(k + 1) * N + n], w2 = wt[(k + 2) * N + n], w3 = wt[(k + 3) * N + n];
#pragma unroll
        for (int r = 0; r < SH_RB; ++r) {
          const float4 xq = *reinterpret_cast<const float4*>(xs + r * SH_KT + k);   // (the same address in every lane of a slice)
          acc[r] = fmaf(xq.x, w0, acc[r]); acc[r] = fmaf(xq.y, w1, acc[r]);
          acc[r] = fmaf(xq.z, w2, acc[r]); acc[r] = fmaf(xq.w, w3, acc[r]);
        }
      }
      for (; k < kend; ++k) {
        const float wv = wt[k * N + n];
#pragma unroll
        for (int r = 0; r < SH_RB; ++r) acc[r] = fmaf(xs[r * SH_KT + k], wv, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SH_RB; ++r) part[r * 256 + tid] = acc[r];
  __syncthreads();
  for (int e = tid; e < SH_RB * N; e += 256) {
    const int r = e / N, c = e - r * N;
    float v = 0.f;
    for (int q = 0; q < KS; ++q) v += part[r * 256 + (q << p.lg) + c];
    v += p.bias != nullptr ? p.bias[c] : 0.f;
    ps[e] = v;
    if (r < nb) p.p[(size_t)(b0 + r) * N + c] = v;
  }
  if (p.mode != 1) return;
  __syncthreads();
  const int E = N >> 1;
  const float sc = p.scale[0];
  for (int e = tid; e < SH_RB * E; e += 256) {
    const int r = e / E, c = e - r * E;
    float ll = 0.f;
    if (r < nb) {
      const float loc = ps[r * N + c], raw = ps[r * N + E + c];
      const float sd = sh_softplus(raw), rs = 1.f / sd;
      const float d = (p.target[(size_t)(b0 + r) * E + c] - loc) * rs;
      ll = -0.5f * d * d - odin_log(sd) - SH_HALF_LOG2PI;
      // d llk / d loc = d / sd;  d llk / d raw = (d^2 - 1) / sd * sigmoid(raw)
      p.dp[(size_t)(b0 + r) * N + c] = -sc * (d * rs);
      p.dp[(size_t)(b0 + r) * N + E + c] = -sc * ((d * d - 1.f) * (sh_sigmoid(raw) * rs));
    }
    lls[e] = ll;
  }
  __syncthreads();
  if (tid < nb) {
    float v = 0.f;
    for (int c = 0; c < E; ++c) v += lls[tid * E + c];
    p.llk[b0 + tid] = v;
  }
}

// ---- backward, role y = 0: dx [B, Dx] and dh [B, H] of this workgroup's rows ----
template <bool V4>
__device__ __forceinline__ void sh_bwd_dgrad(const SHParams& p, float* wt /* SH_WT + SH_KT */, float* red /* 8 * SH_KT */,
                                             float* dps8 /* 8 * 2 SH_DMAX */, float* ared) {
  const int tid = threadIdx.x;
  const int Dx = p.Dx, H = p.H, N = p.N, K = Dx + H, KT = p.kt, NP = N + 1;
  const int c0 = blockIdx.x * p.chunk;
  const int cn = p.B - c0 < p.chunk ? p.B - c0 : p.chunk;   // (> 0: the grid is ceil(B / chunk))
  const int kq = tid & (p.kl - 1), q = tid >> p.lgk, Q = 256 >> p.lgk;
  const int cbeg = q * p.cper, cend = cbeg + p.cper < N ? cbeg + p.cper : N;
  const int nt = (K + KT - 1) / KT;
  float wreg[32], wtail;
  float amx = 0.f;
  const float* __restrict__ hsrc = p.h;
  for (int s0 = 0; s0 < cn; s0 += SH_BR) {
    const int nb = cn - s0 < SH_BR ? cn - s0 : SH_BR, b0 = c0 + s0;
    int ktc = K < KT ? K : KT;
    sh_fetch_w<V4>(p.w, ktc * N, tid, wreg, wtail);
    __syncthreads();
    for (int e = tid; e < N * SH_BR; e += 256) {   // dps8[c][r]
      const int c = e >> 3, r = e & 7;
      dps8[e] = r < nb ? p.dp[(size_t)(b0 + r) * N + c] : 0.f;
    }
    for (int i = 0; i < nt; ++i) {
      const int kt = ktc, k0 = i * KT, cnt = kt * N;
      __syncthreads();   // (the tile before this one and its partial sums have been read)
      sh_store_padded<V4>(wt, cnt, N, tid, wreg, wtail);
      __syncthreads();
      if (i + 1 < nt) {
        const int k1 = (i + 1) * KT;
        ktc = K - k1 < KT ? K - k1 : KT;
        sh_fetch_w<V4>(p.w + (size_t)k1 * N, ktc * N, tid, wreg, wtail);
      }
      // the activations act' is taken from, requested here: in the epilogue below a load behind every store of dh was a
      // chain of 16 dependent round trips per tile (22 us of the launch at B = 256, N = 20)
      float hv[SH_BR][2];
#pragma unroll
      for (int r = 0; r < SH_BR; ++r)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = tid + 256 * j, hk = k0 + (k < kt ? k : kt - 1) - Dx;
          hv[r][j] = hsrc[(size_t)(b0 + (r < nb ? r : nb - 1)) * H + (hk > 0 ? hk : 0)];
        }
      for (int k = kq; k < kt; k += p.kl) {   // (kl < 256: kt <= kl, one row per thread; else up to two)
        float acc[SH_BR];
#pragma unroll
        for (int r = 0; r < SH_BR; ++r) acc[r] = 0.f;
        const float* wr = wt + k * NP;
        for (int c = cbeg; c < cend; ++c) {
          const float wv = wr[c];
          const float4 ga = *reinterpret_cast<const float4*>(dps8 + c * 8);       // (the same address in every lane)
          const float4 gb = *reinterpret_cast<const float4*>(dps8 + c * 8 + 4);
          acc[0] = fmaf(ga.x, wv, acc[0]); acc[1] = fmaf(ga.y, wv, acc[1]);
          acc[2] = fmaf(ga.z, wv, acc[2]); acc[3] = fmaf(ga.w, wv, acc[3]);
          acc[4] = fmaf(gb.x, wv, acc[4]); acc[5] = fmaf(gb.y, wv, acc[5]);
          acc[6] = fmaf(gb.z, wv, acc[6]); acc[7] = fmaf(gb.w, wv, acc[7]);
        }
#pragma unroll
        for (int r = 0; r < SH_BR; ++r) red[r * SH_KT + q * p.kl + k] = acc[r];
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < SH_BR; ++r) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {   // (kt <= 512: two rows of the tile per thread)
          const int k = tid + 256 * j;
          if (r < nb && k < kt) {
            float v = 0.f;
            for (int u = 0; u < Q; ++u) v += red[r * SH_KT + u * p.kl + k];   // column slices ascending
            const int kk = k0 + k;
            if (kk < Dx) {
              if (p.dx != nullptr) p.dx[(size_t)(b0 + r) * Dx + kk] = v;
            } else {
              v *= odin_act_grad(p.h_act, hv[r][j]);
              p.dh[(size_t)(b0 + r) * H + (kk - Dx)] = v;
              amx = fmaxf(amx, fabsf(v));
            }
          }
        }
      }
    }
  }
  odin_amax_commit_wg(p.dh_amax, amx, tid, 256, ared, blockIdx.x);
}

// ---- backward, role y = 1: this workgroup's slab row of (dW | db) ----
// The concatenated axis in pieces: the x part (Dx <= 128 columns), then h in chunks of SH_KC columns.  V4 (h 16-byte
// aligned; H is a multiple of 4): a thread fetches four columns of the 8 rows with 16-byte loads.
template <bool V4>
__device__ __forceinline__ void sh_bwd_wgrad(const SHParams& p, float* xs8 /* SH_KC * 8 */) {
  const int tid = threadIdx.x;
  const int Dx = p.Dx, H = p.H, N = p.N, K = Dx + H;
  const int c0 = blockIdx.x * p.chunk;
  const int cn = p.B - c0 < p.chunk ? p.B - c0 : p.chunk;
  const int n = tid & (p.npad - 1), s = tid >> p.lg, KS = 256 >> p.lg;
  const bool on = n < N;
  const int npiece = 1 + (H + SH_KC - 1) / SH_KC;
  float* __restrict__ row = p.slab + (size_t)blockIdx.x * ((size_t)K * N + N);
  for (int s0 = 0; s0 < cn; s0 += SH_BR) {
    const int nb = cn - s0 < SH_BR ? cn - s0 : SH_BR, b0 = c0 + s0;
    const bool first = s0 == 0;
    float g[SH_BR];
#pragma unroll
    for (int r = 0; r < SH_BR; ++r) {
      const float v = p.dp[(size_t)(b0 + (r < nb ? r : nb - 1)) * N + (on ? n : 0)];
      g[r] = (on && r < nb) ? v : 0.f;
    }
    for (int pc = 0; pc < npiece; ++pc) {
      const bool isx = pc == 0;
      const int hk0 = isx ? 0 : (pc - 1) * SH_KC;
      const int kc = isx ? Dx : (H - hk0 < SH_KC ? H - hk0 : SH_KC);
      const int kbase = isx ? 0 : Dx + hk0;
      __syncthreads();
      // xs8[k][r]: the 8 inputs of a k side by side
      if (isx) {
        float xv[SH_BR];
#pragma unroll
        for (int r = 0; r < SH_BR; ++r) {
          const float v = p.x[(size_t)(b0 + (r < nb ? r : nb - 1)) * Dx + (tid < Dx ? tid : Dx - 1)];
          xv[r] = r < nb ? v : 0.f;
        }
        if (tid < Dx) {
          *reinterpret_cast<float4*>(xs8 + tid * 8) = make_float4(xv[0], xv[1], xv[2], xv[3]);
          *reinterpret_cast<float4*>(xs8 + tid * 8 + 4) = make_float4(xv[4], xv[5], xv[6], xv[7]);
        }
      } else if (V4) {
        const int n4 = kc >> 2, k4 = tid < n4 ? tid : n4 - 1;
        float4 hv[SH_BR];
#pragma unroll
        for (int r = 0; r < SH_BR; ++r) {
          hv[r] = *reinterpret_cast<const float4*>(p.h + (size_t)(b0 + (r < nb ? r : nb - 1)) * H + hk0 + 4 * k4);
          if (r >= nb) hv[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < n4) {
          float* d = xs8 + tid * 32;
          *reinterpret_cast<float4*>(d) = make_float4(hv[0].x, hv[1].x, hv[2].x, hv[3].x);
          *reinterpret_cast<float4*>(d + 4) = make_float4(hv[4].x, hv[5].x, hv[6].x, hv[7].x);
          *reinterpret_cast<float4*>(d + 8) = make_float4(hv[0].y, hv[1].y, hv[2].y, hv[3].y);
          *reinterpret_cast<float4*>(d + 12) = make_float4(hv[4].y, hv[5].y, hv[6].y, hv[7].y);
          *reinterpret_cast<float4*>(d + 16) = make_float4(hv[0].z, hv[1].z, hv[2].z, hv[3].z);
          *reinterpret_cast<float4*>(d + 20) = make_float4(hv[4].z, hv[5].z, hv[6].z, hv[7].z);
          *reinterpret_cast<float4*>(d + 24) = make_float4(hv[0].w, hv[1].w, hv[2].w, hv[3].w);
          *reinterpret_cast<float4*>(d + 28) = make_float4(hv[4].w, hv[5].w, hv[6].w, hv[7].w);
        }
      } else {
#pragma unroll
        for (int j = 0; j < SH_KC / 256; ++j) {
          const int k = tid + 256 * j;
          float xv[SH_BR];
#pragma unroll
          for (int r = 0; r < SH_BR; ++r) {
            const float v = p.h[(size_t)(b0 + (r < nb ? r : nb - 1)) * H + hk0 + (k < kc ? k : kc - 1)];
            xv[r] = r < nb ? v : 0.f;
          }
          if (k < kc) {
            *reinterpret_cast<float4*>(xs8 + k * 8) = make_float4(xv[0], xv[1], xv[2], xv[3]);
            *reinterpret_cast<float4*>(xs8 + k * 8 + 4) = make_float4(xv[4], xv[5], xv[6], xv[7]);
          }
        }
      }
      __syncthreads();
      if (on) {
        const int kper = (kc + KS - 1) / KS, kbeg = s * kper, kend = kbeg + kper < kc ? kbeg + kper : kc;
        for (int k = kbeg; k < kend; ++k) {
          const float4 xa = *reinterpret_cast<const float4*>(xs8 + k * 8);
          const float4 xb = *reinterpret_cast<const float4*>(xs8 + k * 8 + 4);
          float dw = xa.x * g[0];
          dw = fmaf(xa.y, g[1], dw); dw = fmaf(xa.z, g[2], dw); dw = fmaf(xa.w, g[3], dw);
          dw = fmaf(xb.x, g[4], dw); dw = fmaf(xb.y, g[5], dw); dw = fmaf(xb.z, g[6], dw); dw = fmaf(xb.w, g[7], dw);
          const size_t idx = (size_t)(kbase + k) * N + n;
          row[idx] = first ? dw : row[idx] + dw;   // (this thread's own element: rounds ascending)
        }
      }
    }
    if (on && s == 0) {   // bias gradient: the column sums of dp, rows ascending
      float v = 0.f;
#pragma unroll
      for (int r = 0; r < SH_BR; ++r) v += g[r];
      const size_t idx = (size_t)K * N + n;
      row[idx] = first ? v : row[idx] + v;
    }
  }
}

template <bool V4>
__global__ __launch_bounds__(256) void skip_head_bwd_kernel(SHParams p) {
  __shared__ __attribute__((aligned(16))) float lds[SH_WT + SH_KT + 8 * SH_KT + 8 * 2 * SH_DMAX];
  __shared__ float ared[16];
  if (blockIdx.y == 0) sh_bwd_dgrad<V4>(p, lds, lds + SH_WT + SH_KT, lds + SH_WT + SH_KT + 8 * SH_KT, ared);
  else sh_bwd_wgrad<V4>(p, lds);
}

// 0 when (Dx, H, N) lies inside the heads' regime, else the bad-argument code with the limit named
int sh_check(const char* who, int B, int Dx, int H, int N) {
  static thread_local char msg[160];
  const char* why = nullptr;
  if (B < 1) why = "B >= 1";
  else if (Dx < 1 || Dx > SH_DMAX) why = "1 <= Dx <= 128";
  else if (N < 2 || (N & 1) || N > 2 * SH_DMAX) why = "N even, 1 <= N / 2 <= 128";
  else if (H < 4 || (H & 3) || H > SH_HMAX) why = "H a multiple of 4 in [4, 4096]";
  else if ((long)B * (H > N ? H : N) >= (1L << 31)) why = "B * max(H, N) < 2^31";
  if (why == nullptr) return 0;
  snprintf(msg, sizeof(msg), "%s: outside its limits (%s): B = %d, Dx = %d, H = %d, N = %d", who, why, B, Dx, H, N);
  return odin_fail(-2, msg);
}

bool sh_al16(const void* q) { return (((size_t)q) & 15) == 0; }

int sh_chunk(int B) {
  int chunk = (B + SH_ROWS - 1) / SH_ROWS;
  return chunk < SH_BR ? SH_BR : chunk;
}

void sh_fill(SHParams& a, int B, int Dx, int H, int N) {
  memset(&a, 0, sizeof(a));
  a.B = B; a.Dx = Dx; a.H = H; a.N = N;
  a.lg = 1;
  while ((1 << a.lg) < N) ++a.lg;
  a.npad = 1 << a.lg;
  a.kt = (SH_WT / N < SH_KT ? SH_WT / N : SH_KT) & ~3;   // a multiple of 4 (tiles start 16-byte aligned), >= 32 (N <= 256)
  const int KS = 256 >> a.lg;
  a.kper = (((a.kt + KS - 1) / KS) + 3) & ~3;
  a.lgk = 0;
  while ((1 << a.lgk) < a.kt && a.lgk < 8) ++a.lgk;
  a.kl = 1 << a.lgk;
  const int Q = 256 >> a.lgk;
  a.cper = (N + Q - 1) / Q;
}

}  // namespace

extern "C" int odin_skip_head_fwd(const float* x, const float* h, const float* w, const float* bias, float* p, int mode,
                                  const float* target, const float* scale, float* llk, float* dp, int B, int Dx, int H,
                                  int N, void* stream) {
  const int rc = sh_check("skip_head_fwd", B, Dx, H, N);
  if (rc != 0) return rc;
  if (mode != 0 && mode != 1) return odin_fail(-2, "skip_head_fwd: mode must be 0 (projection) or 1 (Gaussian likelihood)");
  if (x == nullptr || h == nullptr || w == nullptr || p == nullptr) return odin_fail(-2, "skip_head_fwd: x / h / w / p");
  if (mode == 1 && (target == nullptr || scale == nullptr || llk == nullptr || dp == nullptr))
    return odin_fail(-2, "skip_head_fwd: mode 1 needs target, scale, llk and dp");
  SHParams a;
  sh_fill(a, B, Dx, H, N);
  a.x = x; a.h = h; a.w = w; a.bias = bias; a.p = p; a.target = target; a.scale = scale; a.llk = llk; a.dp = dp;
  a.mode = mode;
  // (16-byte loads of W where it starts on such a boundary: tiles are multiples of 4 rows)
  if (sh_al16(w)) ODIN_LAUNCH(skip_head_fwd_kernel<true>, dim3((B + SH_RB - 1) / SH_RB), dim3(256), 0, stream, a);
  else ODIN_LAUNCH(skip_head_fwd_kernel<false>, dim3((B + SH_RB - 1) / SH_RB), dim3(256), 0, stream, a);
  return odin_check_launch("skip_head_fwd");
}

extern "C" int odin_skip_head_bwd(const float* x, const float* h, const float* w, const float* dp, int h_act, float* dh,
                                  uint32_t* dh_amax, float* dx, float* slab, int* slab_rows_out, int B, int Dx, int H,
                                  int N, void* stream) {
  const int rc = sh_check("skip_head_bwd", B, Dx, H, N);
  if (rc != 0) return rc;
  if (h_act != ODIN_ACT_LINEAR && h_act != ODIN_ACT_ELU && h_act != ODIN_ACT_RELU)
    return odin_fail(-2, "skip_head_bwd: h_act must be linear, elu or relu");
  const int chunk = sh_chunk(B), rows = (B + chunk - 1) / chunk;
  if (slab_rows_out) *slab_rows_out = rows;
  if (slab == nullptr) return 0;   // dry run
  if (x == nullptr || h == nullptr || w == nullptr || dp == nullptr || dh == nullptr)
    return odin_fail(-2, "skip_head_bwd: x / h / w / dp / dh");
  SHParams a;
  sh_fill(a, B, Dx, H, N);
  a.x = x; a.h = h; a.w = w; a.dp = const_cast<float*>(dp); a.dh = dh; a.dx = dx; a.slab = slab; a.dh_amax = dh_amax;
  a.h_act = h_act; a.chunk = chunk;
  if (sh_al16(w) && sh_al16(h)) ODIN_LAUNCH(skip_head_bwd_kernel<true>, dim3(rows, 2), dim3(256), 0, stream, a);
  else ODIN_LAUNCH(skip_head_bwd_kernel<false>, dim3(rows, 2), dim3(256), 0, stream, a);
  return odin_check_launch("skip_head_bwd");
}
