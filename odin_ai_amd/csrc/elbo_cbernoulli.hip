// elbo_cbernoulli.hip -- Independent(ContinuousBernoulli(logits), 3).log_prob(x) forward + backward in one pass
// ('cbernoulli', odin/bay/distribution_alias.py:108; ContinuousBernoulliLayer, odin/bay/layers/discrete.py:82-121):
// the observation kernel of real-valued pixels in [0, 1].  12 B per element (read logits, x; write dlogits); the
// element's arithmetic is cbern1 (odin_cbern.h).  Contract of odin_elbo_bernoulli_fwd_bwd_ranged: per-sample partial
// sums in the layout odin_elbo_finalize sums, every element of dlogits written once, fixed-order reductions (no float
// atomics: two launches give the same bits), max |dlogits| folded into the optional range word.
//
// Launch forms (the partial count depends on the SHAPE alone, so the dry run reports what any real run uses):
//   n_per_sample % 256 == 0 and B * n_per_sample >= 2^20: one partial per 256-element chunk.  Pointers 16-byte aligned:
//     the persistent grid-stride kernel (64 lanes x float4 per chunk, the next chunk's loads issued before this one is
//     evaluated, streaming stores); otherwise the chunk kernel below with one wave per 256-element chunk.
//   every other shape: the chunk kernel, one workgroup of 256 threads per 1024 elements of a sample
//     (n_part = ceil(n_per_sample / 1024)); 16-byte accesses where n_per_sample % 4 == 0 and the pointers are aligned,
//     a scalar path otherwise.
#include "odin_device.h"
#include "odin_internal.h"
#include "odin_cbern.h"
#include <cstdint>

namespace {

// one workgroup of blockDim.x (64 or 256) threads per 4 * blockDim.x consecutive elements of one sample
__global__ __launch_bounds__(256) void elbo_cbern_chunk_kernel(const float* __restrict__ logits,
                                                               const float* __restrict__ x,
                                                               float* __restrict__ llk_part,
                                                               float* __restrict__ dlogits,
                                                               const float* __restrict__ scale, int N, int n_part,
                                                               int vec, unsigned* __restrict__ g_amax) {
  __shared__ float red[4];
  const unsigned b = blockIdx.x / (unsigned)n_part, part = blockIdx.x - b * (unsigned)n_part;
  const size_t base = (size_t)b * N;
  const int i0 = (int)part * (int)(blockDim.x * 4) + (int)threadIdx.x * 4;
  const float sc = scale[0];
  float acc = 0.f, amx = 0.f;
  if (vec) {
    // (n_per_sample % 4 == 0: a lane's four elements lie inside the sample together or not at all)
    if (i0 + 3 < N) {
      const float4 l = *reinterpret_cast<const float4*>(logits + base + i0);
      const float4 t = *reinterpret_cast<const float4*>(x + base + i0);
      float4 g;
      cbern1(l.x, t.x, sc, acc, g.x);
      cbern1(l.y, t.y, sc, acc, g.y);
      cbern1(l.z, t.z, sc, acc, g.z);
      cbern1(l.w, t.w, sc, acc, g.w);
      *reinterpret_cast<float4*>(dlogits + base + i0) = g;
      amx = odin_amax3(odin_amax3(amx, g.x, g.y), g.z, g.w);
    }
  } else {
    // scalar path: lane-linear, consecutive lanes read consecutive floats (one 256-byte run per wave and access)
    const int c0 = (int)part * (int)(blockDim.x * 4) + (int)threadIdx.x;
    for (int j = 0; j < 4; ++j) {
      const int i = c0 + j * (int)blockDim.x;
      if (i < N) {
        float g;
        cbern1(logits[base + i], x[base + i], sc, acc, g);
        dlogits[base + i] = g;
        amx = fmaxf(amx, fabsf(g));
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  odin_amax_commit_wave(g_amax, amx, lane, blockIdx.x * (blockDim.x >> 6) + wave);
  acc = wave_sum64(acc);
  if (blockDim.x == 64) {
    if (lane == 0) llk_part[blockIdx.x] = acc;
    return;
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) llk_part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// persistent grid: the workgroups' waves walk the 256-element chunks (a chunk lies inside one sample) grid-stride; the
// loads of a wave's NEXT chunk are issued, unconditionally (past the end: chunk 0 again), before the current one is
// evaluated and stored; only the stores and the partial are guarded.  One partial per chunk.
__global__ __launch_bounds__(256) void elbo_cbern_gs_kernel(const float4* __restrict__ logits,
                                                            const float4* __restrict__ x,
                                                            float* __restrict__ llk_part, float4* __restrict__ dlogits,
                                                            const float* __restrict__ scale, size_t n_chunks,
                                                            unsigned* __restrict__ g_amax) {
  const size_t nw = (size_t)gridDim.x * 4;
  const int lane = threadIdx.x & 63;
  const float sc = scale[0];
  size_t c0 = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c0 >= n_chunks) return;
  float amx = 0.f;
  const f32x4* lg = reinterpret_cast<const f32x4*>(logits);
  const f32x4* xg = reinterpret_cast<const f32x4*>(x);
  f32x4 l = lg[c0 * 64 + lane], t = xg[c0 * 64 + lane];
  for (;;) {
    const size_t c1 = c0 + nw;
    const bool more = c1 < n_chunks;   // (wave-uniform)
    const size_t cn = more ? c1 : 0;
    const f32x4 ln = lg[cn * 64 + lane], tn = xg[cn * 64 + lane];
    float4 g;
    float acc = 0.f;
    cbern1(l.x, t.x, sc, acc, g.x);
    cbern1(l.y, t.y, sc, acc, g.y);
    cbern1(l.z, t.z, sc, acc, g.z);
    cbern1(l.w, t.w, sc, acc, g.w);
    amx = odin_amax3(odin_amax3(amx, g.x, g.y), g.z, g.w);
    odin_store4_stream(dlogits + c0 * 64 + lane, g);
    acc = odin_wave_sum64_valu(acc);
    if (lane == 0) llk_part[c0] = acc;
    if (!more) break;
    l = ln;
    t = tn;
    c0 = c1;
  }
  odin_amax_commit_wave(g_amax, amx, lane, blockIdx.x * 4 + (threadIdx.x >> 6));
}

}  // namespace

extern "C" int odin_elbo_cbernoulli_fwd_bwd(const float* logits, const float* x, float* llk_part, float* dlogits,
                                            const float* scale, int B, int n_per_sample, int* n_part_out,
                                            uint32_t* dlogits_amax, void* stream) {
  if (B < 1 || n_per_sample < 1) return odin_fail(-2, "elbo_cbernoulli: B and n_per_sample must be positive");
  if (n_per_sample > (1 << 30)) return odin_fail(-2, "elbo_cbernoulli: more than 2^30 elements per sample");
  unsigned* g_amax = reinterpret_cast<unsigned*>(dlogits_amax);
  const bool aligned = (((uintptr_t)logits | (uintptr_t)x | (uintptr_t)dlogits) & 15) == 0;
  const bool per256 = n_per_sample % 256 == 0 && (size_t)B * n_per_sample >= (1u << 20);
  const int n_part = per256 ? n_per_sample / 256 : (n_per_sample + 1023) / 1024;
  const size_t n_chunks = (size_t)B * n_part;
  if (n_chunks > 0x7fffffffull) return odin_fail(-2, "elbo_cbernoulli: too many partial sums for one launch");
  if (n_part_out) *n_part_out = n_part;
  if (logits == nullptr) return 0;  // dry run: reports the partial count
  if (per256 && aligned) {
    // (the Bernoulli kernel's measured shape: 1.5 chunks per wave, 512 .. 4096 workgroups)
    int blocks = (int)((n_chunks / 6 + 511) / 512) * 512;
    blocks = blocks < 512 ? 512 : blocks > 4096 ? 4096 : blocks;
    ODIN_LAUNCH(elbo_cbern_gs_kernel, dim3(blocks), dim3(256), 0, stream, (const float4*)logits, (const float4*)x,
                llk_part, (float4*)dlogits, scale, n_chunks, g_amax);
    return odin_check_launch("elbo_cbernoulli");
  }
  const int vec = (aligned && n_per_sample % 4 == 0) ? 1 : 0;
  ODIN_LAUNCH(elbo_cbern_chunk_kernel, dim3((unsigned)n_chunks), dim3(per256 ? 64 : 256), 0, stream, logits, x, llk_part,
              dlogits, scale, n_per_sample, n_part, vec, g_amax);
  return odin_check_launch("elbo_cbernoulli");
}
