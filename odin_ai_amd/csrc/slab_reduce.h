// slab_reduce.h -- the slab reduction's job table and its workgroup body, shared by the reduction launch (wgrad.hip) and
// the launch that runs part of the same plan beside other work (neck.hip: the reducing role of neck_bwd_kernel).
#pragma once
#include <cstdint>
#include "odin_device.h"
#include "odin_internal.h"

constexpr int MAX_JOBS = 64;
struct ReduceJobs {
  odin_reduce_job j[MAX_JOBS];
  // odin_slab_reduce_sumsq: the squared norm of what the launch writes, as one partial per ACTIVE workgroup --
  // part[poff[j] + blockIdx.x] for blockIdx.x < pcnt[j]; poff[j] < 0: job j's result is not part of the gradient
  // (the range-word reset).  stage_src / stage_dst: `stage_n` floats copied by workgroup (0, 0) (the step's
  // hyper-parameter row, read by the Adam launch after `hyper` itself was advanced).
  float* part;
  int poff[MAX_JOBS];
  int pcnt[MAX_JOBS];
  const float* stage_src;
  float* stage_dst;
  int stage_n;
};

// One plan for a job list (at most MAX_JOBS jobs), as every launch that executes a part of it must see it: the grid width
// `gx` over ALL jobs, and for every job its slice poff / pcnt of the norm partials (g_lo == nullptr: no partials).
// The jobs in `skip` (bit j = job j) keep their slices but are left out of `rj`, which holds the others in their order:
// a launch (gx, *nj_out) over `rj` writes exactly what the full launch writes for them, at the same indices.
// *n_parts_out: partials of the whole list.  (wgrad.hip)
int odin_slab_reduce_plan(const odin_reduce_job* jobs, int n_jobs, uint64_t skip, const float* g_lo, size_t g_n,
                          float* part, ReduceJobs* rj, int* nj_out, int* gx_out, int* n_parts_out);
// workgroups of job jb that write results (the body's three paths), for a launch gx wide; *trips_out (optional): the
// largest number of column steps one of them takes
int odin_reduce_active_blocks(const odin_reduce_job& jb, int gx, int* trips_out);

// The squares of a result float4 for the norm partial.  Which product of a pair is rounded before the other is fused
// onto it is spelled out: left to the compiler's contraction of (x x + y y) + (z z + w w) it differed between the two
// vector paths and changed with the code around them -- two launches that execute one plan (and two builds of the
// library) must give the same bits.  The two paths differ (WIDE rounds y y and w w first, VEC x x and z z) for no
// numerical reason: these are the forms the kernel has always computed, kept so that trained weights do not move by an ulp.
#define SLAB_SQ4_WIDE(t) (fmaf((t).x, (t).x, (t).y * (t).y) + fmaf((t).z, (t).z, (t).w * (t).w))
#define SLAB_SQ4_VEC(t) (fmaf((t).y, (t).y, (t).x * (t).x) + fmaf((t).w, (t).w, (t).z * (t).z))

// the body's scratch in LDS: 256 float4 (wide path), 256 float4 (narrow vector path), 256 floats (odd path), 4 floats
// (the partial); a path uses its own array only, and every use ends behind a barrier, so the three may be one buffer
struct SlabLds {
  float4* wide;
  float4* vec;
  float* odd;
  float* ssw;
};

// The work of virtual block (vbx, by) of a launch vgx wide over `jobs`, by the 256 threads tid = 0 .. 255 of one
// virtual block.
// Vector jobs (n, stride multiples of 4, 16-byte aligned): a block owns 64 consecutive floats of
// the result; thread (tx = tid & 15, ty = tid >> 4) sums rows ty, ty + 16, ... of float4 column tx
// with four independent partial sums, the 16 row phases are combined through LDS in a fixed
// order.  Parallelism is rows x n, not n: a 16 K-float gradient over 256 slab rows is 256 blocks
// of 16-byte loads instead of 64 blocks of serial 4-byte loads.  Other jobs (bias rows, the
// tail's 65-float row): one thread per result element.
// UNI = false: the 256 threads are the workgroup (slab_reduce_kernel); `trips` and `live` are not read.
// UNI = true: several virtual blocks share one workgroup and therefore its barriers: each runs `trips` column steps
// whatever its job (loads and stores beyond its own range are guarded, as beyond n4), a virtual block that is not
// `live` only keeps the barriers, and the barrier of the norm partial is taken by all.
// (The hyper row is staged by the reduction kernel itself, not here.)
template <bool UNI>
__device__ __forceinline__ void slab_reduce_body(const ReduceJobs& jobs, unsigned by, unsigned vbx, unsigned vgx,
                                                 unsigned tid, int trips, bool live, const SlabLds L) {
  const odin_reduce_job jb = jobs.j[by];
  const int jn = (UNI && !live) ? 0 : jb.n, jrows = (UNI && !live) ? 0 : jb.rows;
  const size_t st = jb.stride > 0 ? (size_t)jb.stride : (size_t)jn;
  float ss = 0.f;   // squares of what this thread writes (odin_slab_reduce_sumsq)
  const bool vec = ((jn & 3) == 0) && ((st & 3) == 0) &&
                   ((((size_t)jb.src | (size_t)jb.dst) & 15) == 0);
  if (vec && (jn >> 2) >= 1024) {
    // wide jobs (weight tensors): a block owns 256 consecutive floats; every wave-instruction
    // reads one full KB of a slab row, 8 rows in flight per lane, the 4 waves split the rows
    float4* partw = L.wide;
    const int tx = tid & 63, ty = tid >> 6;
    const int n4 = jn >> 2;
    const size_t st4 = st >> 2;
    int t_ = 0;
    for (int c0 = vbx * 64; UNI ? t_ < trips : c0 < n4; c0 += vgx * 64, ++t_) {  // block-uniform
      const int c = c0 + tx;
      float4 a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < n4) {
        const float4* s = reinterpret_cast<const float4*>(jb.src) + c;
        int g = ty;
        for (; g + 28 < jrows; g += 32) {
          float4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(g + 4 * u) * st4];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            a[u].x += v[u].x; a[u].y += v[u].y; a[u].z += v[u].z; a[u].w += v[u].w;
          }
        }
        for (; g < jrows; g += 4) {
          const float4 v0 = s[(size_t)g * st4];
          a[0].x += v0.x; a[0].y += v0.y; a[0].z += v0.z; a[0].w += v0.w;
        }
      }
      float4 t;
      t.x = ((a[0].x + a[1].x) + (a[2].x + a[3].x)) + ((a[4].x + a[5].x) + (a[6].x + a[7].x));
      t.y = ((a[0].y + a[1].y) + (a[2].y + a[3].y)) + ((a[4].y + a[5].y) + (a[6].y + a[7].y));
      t.z = ((a[0].z + a[1].z) + (a[2].z + a[3].z)) + ((a[4].z + a[5].z) + (a[6].z + a[7].z));
      t.w = ((a[0].w + a[1].w) + (a[2].w + a[3].w)) + ((a[4].w + a[5].w) + (a[6].w + a[7].w));
      partw[tid] = t;
      __syncthreads();
      if (ty == 0 && c < n4) {
        const float4 q1 = partw[64 + tx], q2 = partw[128 + tx], q3 = partw[192 + tx];
        t.x = (t.x + q1.x) + (q2.x + q3.x);
        t.y = (t.y + q1.y) + (q2.y + q3.y);
        t.z = (t.z + q1.z) + (q2.z + q3.z);
        t.w = (t.w + q1.w) + (q2.w + q3.w);
        reinterpret_cast<float4*>(jb.dst)[c] = t;
        ss += SLAB_SQ4_WIDE(t);
      }
      __syncthreads();
    }
  } else if (vec) {
    float4* part = L.vec;
    const int tx = tid & 15, ty = tid >> 4;
    const int n4 = jn >> 2;
    int t_ = 0;
    for (int c0 = vbx * 16; UNI ? t_ < trips : c0 < n4; c0 += vgx * 16, ++t_) {  // block-uniform
      const int c = c0 + tx;
      float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0, a2 = a0, a3 = a0;
      if (c < n4) {
        const float4* s = reinterpret_cast<const float4*>(jb.src) + c;
        const size_t st4 = st >> 2;
        int g = ty;
        for (; g + 112 < jrows; g += 128) {  // 8 rows in flight
          const float4 v0 = s[(size_t)g * st4], v1 = s[(size_t)(g + 16) * st4];
          const float4 v2 = s[(size_t)(g + 32) * st4], v3 = s[(size_t)(g + 48) * st4];
          const float4 v4 = s[(size_t)(g + 64) * st4], v5 = s[(size_t)(g + 80) * st4];
          const float4 v6 = s[(size_t)(g + 96) * st4], v7 = s[(size_t)(g + 112) * st4];
          a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
          a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
          a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
          a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
          a0.x += v4.x; a0.y += v4.y; a0.z += v4.z; a0.w += v4.w;
          a1.x += v5.x; a1.y += v5.y; a1.z += v5.z; a1.w += v5.w;
          a2.x += v6.x; a2.y += v6.y; a2.z += v6.z; a2.w += v6.w;
          a3.x += v7.x; a3.y += v7.y; a3.z += v7.z; a3.w += v7.w;
        }
        for (; g + 48 < jrows; g += 64) {
          const float4 v0 = s[(size_t)g * st4], v1 = s[(size_t)(g + 16) * st4];
          const float4 v2 = s[(size_t)(g + 32) * st4], v3 = s[(size_t)(g + 48) * st4];
          a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
          a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
          a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
          a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
        }
        for (; g < jrows; g += 16) {
          const float4 v0 = s[(size_t)g * st4];
          a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        }
      }
      part[tid] = make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y),
                              (a0.z + a1.z) + (a2.z + a3.z), (a0.w + a1.w) + (a2.w + a3.w));
      __syncthreads();
      if (ty == 0 && c < n4) {
        float4 t = part[tx];
#pragma unroll
        for (int u = 1; u < 16; ++u) {
          const float4 q = part[u * 16 + tx];
          t.x += q.x; t.y += q.y; t.z += q.z; t.w += q.w;
        }
        reinterpret_cast<float4*>(jb.dst)[c] = t;
        ss += SLAB_SQ4_VEC(t);
      }
      __syncthreads();
    }
  } else
  // odd-sized jobs (the fused tail's 65-float rows, 33-float heads): 32 result elements per block,
  // 8 row phases per element, 8 loads in flight per thread -- a one-thread-per-element loop walks
  // 256+ rows serially (dozens of dependent L2 round trips: it set the duration of the whole launch)
  {
    float* parts = L.odd;
    const int tx = tid & 31, ty = tid >> 5;
    int t_ = 0;
    for (int i0 = vbx * 32; UNI ? t_ < trips : i0 < jn; i0 += vgx * 32, ++t_) {  // block-uniform
      const int i = i0 + tx;
      float a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = 0.f;
      if (i < jn) {
        const float* s = jb.src + i;
        int g = ty;
        for (; g + 56 < jrows; g += 64) {
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = s[(size_t)(g + 8 * u) * st];
#pragma unroll
          for (int u = 0; u < 8; ++u) a[u] += v[u];
        }
        for (; g < jrows; g += 8) a[0] += s[(size_t)g * st];
      }
      parts[tid] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
      __syncthreads();
      if (ty == 0 && i < jn) {
        float t = parts[tx];
#pragma unroll
        for (int u = 1; u < 8; ++u) t += parts[u * 32 + tx];
        jb.dst[i] = t;
        ss = fmaf(t, t, ss);
      }
      __syncthreads();
    }
  }
  if (UNI || (jobs.part != nullptr && jobs.poff[by] >= 0 && (int)vbx < jobs.pcnt[by])) {
    // one partial per active workgroup, fixed order inside the workgroup: wave sums by shuffles, then the four waves
    float* ssw = L.ssw;
    float v = ss;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((tid & 63) == 0) ssw[tid >> 6] = v;
    __syncthreads();
    if (tid == 0 && (!UNI || (live && jobs.part != nullptr && jobs.poff[by] >= 0 && (int)vbx < jobs.pcnt[by])))
      jobs.part[jobs.poff[by] + vbx] = (ssw[0] + ssw[1]) + (ssw[2] + ssw[3]);
  }
}
