// Global gradient norm and the clip coefficient, on the device (tf.clip_by_global_norm / tf.global_norm).
//
// The fused optimizer kernels (optim.hip) read {lr, lr_t, grad_scale} from a device buffer ``dyn``.  Clipping by
// global norm multiplies grad_scale by coef = clip_norm / max(norm, clip_norm), so it is two small launches in
// front of the unchanged update kernels and no host read of the norm (the step stays hipGraph-capturable):
//
//   grad_sumsq     one launch over every update target's fp32 gradient buffer (<= 8 segments by value): each
//                  block owns a contiguous range of 16 KiB chunks, issues every 16-B load of a chunk before the
//                  math, accumulates in fp32, reduces over the wave (wave_sum) and over the waves through LDS and
//                  writes one partial with a plain store.  No atomics: bitwise repeatable in every mode.
//                  Plain (cached) loads: the optimizer re-reads the same gradient right after, and in the step
//                  they measured faster than nontemporal ones; a grid capped at 2048 blocks per segment keeps the
//                  finalize short (both A/Bs: profiles/clip_norm.md).
//   clip_finalize  one block: partials summed in a fixed order in fp64, norm = grad_scale * sqrt(sumsq), the
//                  effective {lr, lr_t, grad_scale * coef} buffer handed to the update kernels as ``dyn`` and the
//                  {norm, coef} stats.  The sharded path all-reduces sumsq between the reduce and the coefficient
//                  half (mode argument).
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kThreads = 256;
constexpr int kVpt = 4;                          // float4s per thread per chunk
constexpr int kChunk4 = kThreads * kVpt;         // float4s per chunk (16 KiB)
constexpr int kMaxSeg = 8;
constexpr int kGridCap = 2048;                   // blocks per segment (8 per CU); larger segments loop over chunks

struct SumsqSegs {
  const float* p[kMaxSeg];
  long long n4[kMaxSeg];       // float4s in the segment
  int first[kMaxSeg];          // first block of the segment
  int cpb[kMaxSeg];            // chunks per block
};

__global__ void __launch_bounds__(kThreads) grad_sumsq_kernel(SumsqSegs s, int nseg, float* __restrict__ partials) {
  const int b = blockIdx.x;
  const float* __restrict__ p = s.p[0];
  long long n4 = s.n4[0];
  int first = 0, cpb = s.cpb[0];
#pragma unroll
  for (int i = 1; i < kMaxSeg; ++i) {
    if (i < nseg && b >= s.first[i]) {
      p = s.p[i];
      n4 = s.n4[i];
      first = s.first[i];
      cpb = s.cpb[i];
    }
  }
  long long base = (long long)(b - first) * cpb * kChunk4;
  float acc = 0.f;
  for (int c = 0; c < cpb && base < n4; ++c, base += kChunk4) {
    float4 v[kVpt];
#pragma unroll
    for (int u = 0; u < kVpt; ++u) {
      const long long i = base + u * kThreads + threadIdx.x;
      v[u] = i < n4 ? reinterpret_cast<const float4*>(p)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < kVpt; ++u) {
      acc = fmaf(v[u].x, v[u].x, acc);
      acc = fmaf(v[u].y, v[u].y, acc);
      acc = fmaf(v[u].z, v[u].z, acc);
      acc = fmaf(v[u].w, v[u].w, acc);
    }
  }
  acc = wave_sum(acc);
  __shared__ float wsum[kThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[b] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// mode 0: reduce + coefficient; 1: reduce only (sumsq out); 2: coefficient only (sumsq in)
__global__ void __launch_bounds__(kThreads) clip_finalize_kernel(const float* __restrict__ partials, int np,
                                                                double* __restrict__ sumsq, float clip_norm, float lr,
                                                                float lr_t, float gs, const float* __restrict__ dyn,
                                                                float* __restrict__ eff, float* __restrict__ stats,
                                                                int mode) {
  __shared__ double red[kThreads];
  double ss = 0.0;
  if (mode != 2) {
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += kThreads) a += static_cast<double>(partials[i]);
    red[threadIdx.x] = a;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    ss = red[0];
  }
  if (threadIdx.x != 0) return;
  if (mode == 1) {
    sumsq[0] = ss;
    return;
  }
  if (mode == 2) ss = sumsq[0];
  if (dyn) {
    lr = dyn[0];
    lr_t = dyn[1];
    gs = dyn[2];
  }
  const float norm = static_cast<float>(static_cast<double>(gs) * sqrt(ss));
  float coef = 1.f;
  if (clip_norm > 0.f) {
    if (!isfinite(norm))
      coef = __builtin_nanf("");
    else if (norm > clip_norm)
      coef = clip_norm / norm;
  }
  eff[0] = lr;
  eff[1] = lr_t;
  eff[2] = coef == 1.f ? gs : gs * coef;
  stats[0] = norm;
  stats[1] = coef;
}

inline void seg_plan(long long n, int* blocks, int* cpb) {
  const long long chunks = ceil_div(n / 4, (long long)kChunk4);
  const long long per = chunks > kGridCap ? ceil_div(chunks, (long long)kGridCap) : 1;
  *cpb = static_cast<int>(per);
  *blocks = static_cast<int>(chunks > 0 ? ceil_div(chunks, per) : 1);
}

}  // namespace

// partials one launch over segments of ns[] elements writes (the caller sizes its buffer with this)
MDTF_EXPORT long long mdtf_grad_sumsq_blocks(const long long* ns, int nseg) {
  if (nseg < 1 || nseg > kMaxSeg) return MDTF_EINVAL;
  long long total = 0;
  for (int i = 0; i < nseg; ++i) {
    if (ns[i] < 0 || ns[i] % 4) return MDTF_EINVAL;
    int blocks, cpb;
    seg_plan(ns[i], &blocks, &cpb);
    total += blocks;
  }
  return total;
}

// sum of squares of nseg <= 8 fp32 buffers (ns[i] elements each, a multiple of 4; 16-B aligned): one fp32 partial
// per block into partials[0 .. mdtf_grad_sumsq_blocks), cap = elements the partials buffer holds
MDTF_EXPORT int mdtf_grad_sumsq(const void* const* ptrs, const long long* ns, int nseg, void* partials, long long cap,
                                hipStream_t st) {
  if (nseg < 1 || nseg > kMaxSeg) return MDTF_EINVAL;
  SumsqSegs s{};
  long long total = 0;
  for (int i = 0; i < nseg; ++i) {
    if (ns[i] < 0 || ns[i] % 4 || (reinterpret_cast<uintptr_t>(ptrs[i]) & 15)) return MDTF_EINVAL;
    if (ns[i] > 0 && !ptrs[i]) return MDTF_EINVAL;
    int blocks;
    seg_plan(ns[i], &blocks, &s.cpb[i]);
    s.p[i] = static_cast<const float*>(ptrs[i]);
    s.n4[i] = ns[i] / 4;
    s.first[i] = static_cast<int>(total);
    total += blocks;
  }
  if (!partials || total > cap || total > 0x7fffffffLL) return MDTF_EINVAL;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(static_cast<unsigned>(total)), dim3(kThreads), 0, st, s, nseg,
                     static_cast<float*>(partials));
  MDTF_LAUNCH_CHECK();
  return 0;
}

// partials[np] -> sumsq (fp64[1]), eff = {lr, lr_t, grad_scale * coef} (fp32[3]), stats = {norm, coef} (fp32[2]);
// dyn (nullable) overrides lr / lr_t / gs like the update kernels' dyn; mode: see clip_finalize_kernel
MDTF_EXPORT int mdtf_clip_finalize(const void* partials, int np, void* sumsq, float clip_norm, float lr, float lr_t,
                                   float gs, const void* dyn, void* eff, void* stats, int mode, hipStream_t st) {
  if (mode < 0 || mode > 2 || np < 0 || (mode != 2 && !partials) || (mode != 0 && !sumsq)) return MDTF_EINVAL;
  if (mode != 1 && (!eff || !stats)) return MDTF_EINVAL;
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kThreads), 0, st, static_cast<const float*>(partials), np,
                     static_cast<double*>(sumsq), clip_norm, lr, lr_t, gs, static_cast<const float*>(dyn),
                     static_cast<float*>(eff), static_cast<float*>(stats), mode);
  MDTF_LAUNCH_CHECK();
  return 0;
}
