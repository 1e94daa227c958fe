// Layer-wise adaptive optimizers (LAMB, LARS) over flat fp32 parameter buffers, with the per-layer trust ratios
// computed on the device (no host read of a norm: the step stays hipGraph-capturable).
//
// The flat update kernels (optim.hip) apply ONE {lr, lr_t, grad_scale} to a whole group; LAMB and LARS scale the
// step of every variable ("layer") by a ratio of L2 norms over that variable.  Each update target gets a host-built
// table of work items {off4, len4, layer, decay} (float4 units; an item lies inside one variable's piece of the
// target and holds at most one 16 KiB chunk), uploaded once.  One block processes one item:
//
//   lamb_moments    reads g, m, v, w; writes m, v; u = m / (sqrt(v) + eps) + wd * w; one fp32 partial pair
//                   (sum w^2, sum u^2) per item.  Every load of the chunk is issued before the math; wave_sum, then a
//                   cross-wave sum through LDS and one plain store per partial (no atomics: bitwise repeatable).
//   lars_norms      reads g, w; partial pair (sum w^2, sum g^2) per item.
//   layer_finalize  one block per LAYER: the layer's partials (contiguous in the table) summed in a fixed order in
//                   fp64 into sums[2 L], then ratio[L] in fp32.  mode 0: reduce + ratio; 1: reduce only; 2: ratio only
//                   (sharded replicas all-reduce ``sums`` between the halves).  LARS applies grad_scale to ||g|| here.
//   lamb_apply      reads m, v, w; recomputes u from the updated moments and the old w (same expression as in
//                   lamb_moments, so the same bits), looks ratio[layer] up per item, writes w and the bf16 shadow.
//                   The gradient buffer is left untouched.
//   lars_apply      the momentum update with the per-item ratio.
//
// Zero-padded elements (alignment gaps, bucket tails, pad rows) are counted with a neighbouring layer: both
// formulas map zeros to zero for any finite ratio, and they add nothing to a norm.
// State streams use nontemporal loads and stores, like the Adam and momentum kernels; the bf16 shadow the next
// forward reads stays cached.  In the BERT-base step they measured 0.09 ms faster than plain ones in three
// alternating rounds and tied for ResNet-50 (profiles/layerwise_optim.md).
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kThreads = 256;
constexpr int kVpt = 4;                          // float4s per thread per item
constexpr int kChunk4 = kThreads * kVpt;         // float4s per item at most (16 KiB)

struct Item {
  int off4;    // first float4 of the item in the target
  int len4;    // float4s (1 .. kChunk4)
  int layer;   // index into ratio[] / sums[]
  int decay;   // 1: weight decay applies to the layer; 0: wd = 0 (and the layer's ratio is 1)
};

struct Layer {
  int first;   // first partial pair of the layer
  int count;   // partial pairs (0: no piece of the layer on this replica)
  int decay;   // 1: the ratio applies; 0: ratio 1
  int pad;
};

__device__ __forceinline__ void load_dyn(const float* dyn, float& lr, float& gs) {
  if (dyn) {
    lr = dyn[0];
    gs = dyn[2];
  }
}

__device__ __forceinline__ void store_shadow4(bf16_t* s, long long i, const float4& w) {
  *reinterpret_cast<uint2*>(s + i) = make_uint2(pack_bf2(w.x, w.y), pack_bf2(w.z, w.w));
}

// the LAMB update direction; ONE expression shared by lamb_moments and lamb_apply (explicit fma: the norm and the
// step see the same bits whatever the compiler contracts elsewhere)
__device__ __forceinline__ float lamb_u(float m, float v, float w, float eps, float wd) {
  return fmaf(wd, w, m / (sqrtf(v) + eps));
}

// (a, b) summed over the block -> out[0], out[1] by thread 0
__device__ __forceinline__ void block_pair_store(float a, float b, float* out) {
  a = wave_sum(a);
  b = wave_sum(b);
  __shared__ float wsum[2][kThreads / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) {
    wsum[0][threadIdx.x / kWave] = a;
    wsum[1][threadIdx.x / kWave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3]);
    out[1] = (wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3]);
  }
}

// state streams (master, gradient, moments: each read and written once per launch): nontemporal 16-B accesses
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p, long long i) {
  return __builtin_bit_cast(float4, __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p) + i));
}
__device__ __forceinline__ void st4(float* p, long long i, const float4& v) {
  __builtin_nontemporal_store(__builtin_bit_cast(f32x4_t, v), reinterpret_cast<f32x4_t*>(p) + i);
}

__global__ void __launch_bounds__(kThreads) lamb_moments_kernel(const Item* __restrict__ items, int pbase,
                                                               const float* __restrict__ w,
                                                               const float* __restrict__ g, float* __restrict__ m,
                                                               float* __restrict__ v, float* __restrict__ partials,
                                                               float b1, float b2, float eps, float gs, float wd,
                                                               const float* __restrict__ dyn) {
  float lr = 0.f;
  load_dyn(dyn, lr, gs);
  const Item it = items[blockIdx.x];
  const long long base = it.off4;
  if (!it.decay) wd = 0.f;
  float4 wv[kVpt], gv[kVpt], mv[kVpt], vv[kVpt];
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j < it.len4) {
      wv[u] = ld4(w, base + j);
      gv[u] = ld4(g, base + j);
      mv[u] = ld4(m, base + j);
      vv[u] = ld4(v, base + j);
    }
  }
  const float c1 = 1.f - b1, c2 = 1.f - b2;
  float sw = 0.f, su = 0.f;
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j >= it.len4) break;
    float* wp = &wv[u].x;
    float* gp = &gv[u].x;
    float* mp = &mv[u].x;
    float* vp = &vv[u].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gh = gp[e] * gs;
      mp[e] = b1 * mp[e] + c1 * gh;
      vp[e] = b2 * vp[e] + c2 * gh * gh;
      const float uu = lamb_u(mp[e], vp[e], wp[e], eps, wd);
      sw = fmaf(wp[e], wp[e], sw);
      su = fmaf(uu, uu, su);
    }
    st4(m, base + j, mv[u]);
    st4(v, base + j, vv[u]);
  }
  block_pair_store(sw, su, partials + 2 * (static_cast<long long>(pbase) + blockIdx.x));
}

__global__ void __launch_bounds__(kThreads) lamb_apply_kernel(const Item* __restrict__ items, float* __restrict__ w,
                                                             const float* __restrict__ m, const float* __restrict__ v,
                                                             bf16_t* __restrict__ shadow,
                                                             const float* __restrict__ ratio, float lr, float eps,
                                                             float wd, const float* __restrict__ dyn) {
  float gs = 1.f;
  load_dyn(dyn, lr, gs);
  const Item it = items[blockIdx.x];
  const long long base = it.off4;
  const float step = lr * ratio[it.layer];
  if (!it.decay) wd = 0.f;
  float4 wv[kVpt], mv[kVpt], vv[kVpt];
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j < it.len4) {
      wv[u] = ld4(w, base + j);
      mv[u] = ld4(m, base + j);
      vv[u] = ld4(v, base + j);
    }
  }
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j >= it.len4) break;
    wv[u].x -= step * lamb_u(mv[u].x, vv[u].x, wv[u].x, eps, wd);
    wv[u].y -= step * lamb_u(mv[u].y, vv[u].y, wv[u].y, eps, wd);
    wv[u].z -= step * lamb_u(mv[u].z, vv[u].z, wv[u].z, eps, wd);
    wv[u].w -= step * lamb_u(mv[u].w, vv[u].w, wv[u].w, eps, wd);
    st4(w, base + j, wv[u]);
    if (shadow) store_shadow4(shadow, (base + j) * 4, wv[u]);
  }
}

__global__ void __launch_bounds__(kThreads) lars_norms_kernel(const Item* __restrict__ items, int pbase,
                                                             const float* __restrict__ w,
                                                             const float* __restrict__ g,
                                                             float* __restrict__ partials) {
  const Item it = items[blockIdx.x];
  const long long base = it.off4;
  float4 wv[kVpt], gv[kVpt];
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    const bool in = j < it.len4;
    wv[u] = in ? ld4(w, base + j) : make_float4(0.f, 0.f, 0.f, 0.f);
    gv[u] = in ? ld4(g, base + j) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sw = 0.f, sg = 0.f;
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    sw = fmaf(wv[u].x, wv[u].x, sw);
    sw = fmaf(wv[u].y, wv[u].y, sw);
    sw = fmaf(wv[u].z, wv[u].z, sw);
    sw = fmaf(wv[u].w, wv[u].w, sw);
    sg = fmaf(gv[u].x, gv[u].x, sg);
    sg = fmaf(gv[u].y, gv[u].y, sg);
    sg = fmaf(gv[u].z, gv[u].z, sg);
    sg = fmaf(gv[u].w, gv[u].w, sg);
  }
  block_pair_store(sw, sg, partials + 2 * (static_cast<long long>(pbase) + blockIdx.x));
}

__global__ void __launch_bounds__(kThreads) lars_apply_kernel(const Item* __restrict__ items, float* __restrict__ w,
                                                             const float* __restrict__ g, float* __restrict__ acc,
                                                             bf16_t* __restrict__ shadow,
                                                             const float* __restrict__ ratio, float lr, float mom,
                                                             float gs, float wd, int nesterov,
                                                             const float* __restrict__ dyn) {
  load_dyn(dyn, lr, gs);
  const Item it = items[blockIdx.x];
  const long long base = it.off4;
  const float step = lr * ratio[it.layer];
  if (!it.decay) wd = 0.f;
  float4 wv[kVpt], gv[kVpt], av[kVpt];
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j < it.len4) {
      wv[u] = ld4(w, base + j);
      gv[u] = ld4(g, base + j);
      av[u] = ld4(acc, base + j);
    }
  }
#pragma unroll
  for (int u = 0; u < kVpt; ++u) {
    const int j = u * kThreads + threadIdx.x;
    if (j >= it.len4) break;
    float* wp = &wv[u].x;
    float* gp = &gv[u].x;
    float* ap = &av[u].x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float s = step * (gp[e] * gs + wd * wp[e]);
      ap[e] = mom * ap[e] + s;
      wp[e] -= nesterov ? s + mom * ap[e] : ap[e];
    }
    st4(acc, base + j, av[u]);
    st4(w, base + j, wv[u]);
    if (shadow) store_shadow4(shadow, (base + j) * 4, wv[u]);
  }
}

// kind 0 LAMB: sums = (sum w^2, sum u^2), ratio = |w| / |u|; kind 1 LARS: sums = (sum w^2, sum g^2),
// ratio = eeta |w| / (gs |g| + wd |w| + eps).  A zero norm gives 1, a non-finite one NaN; layers without decay: 1.
// mode 0: reduce + ratio; 1: reduce only (sums out); 2: ratio only (sums in)
__global__ void __launch_bounds__(kThreads) layer_finalize_kernel(const Layer* __restrict__ layers,
                                                                 const float* __restrict__ partials,
                                                                 double* __restrict__ sums, float* __restrict__ ratio,
                                                                 int kind, float eeta, float wd, float eps, float gs,
                                                                 const float* __restrict__ dyn, int mode) {
  __shared__ double red[2][kThreads];
  const int L = blockIdx.x;
  const Layer ly = layers[L];
  double sa = 0.0, sb = 0.0;
  if (mode != 2) {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < ly.count; i += kThreads) {
      const float2 p = reinterpret_cast<const float2*>(partials)[ly.first + i];
      a += static_cast<double>(p.x);
      b += static_cast<double>(p.y);
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) {
        red[0][threadIdx.x] += red[0][threadIdx.x + o];
        red[1][threadIdx.x] += red[1][threadIdx.x + o];
      }
      __syncthreads();
    }
    sa = red[0][0];
    sb = red[1][0];
  }
  if (threadIdx.x != 0) return;
  if (mode == 1) {
    sums[2 * L] = sa;
    sums[2 * L + 1] = sb;
    return;
  }
  if (mode == 2) {
    sa = sums[2 * L];
    sb = sums[2 * L + 1];
  } else {
    sums[2 * L] = sa;
    sums[2 * L + 1] = sb;
  }
  float r = 1.f;
  if (ly.decay) {
    if (!isfinite(sa) || !isfinite(sb)) {
      r = __builtin_nanf("");
    } else {
      const double wn = sqrt(sa);
      if (kind == 0) {
        const double un = sqrt(sb);
        if (wn > 0.0 && un > 0.0) r = static_cast<float>(wn / un);
      } else {
        if (dyn) gs = dyn[2];
        const double gn = static_cast<double>(gs) * sqrt(sb);
        if (!isfinite(gn))
          r = __builtin_nanf("");
        else if (wn > 0.0 && gn > 0.0)
          r = static_cast<float>(static_cast<double>(eeta) * wn /
                                 (gn + static_cast<double>(wd) * wn + static_cast<double>(eps)));
      }
    }
  }
  ratio[L] = r;
}

inline bool bad_buf(const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

// float4s one work item holds at most (the host builds its tables with this)
MDTF_EXPORT int mdtf_layerwise_chunk4() { return kChunk4; }

// items: nitems x {off4, len4, layer, decay} (int32, device); partials: fp32 pairs, pair (pbase + i) belongs to item i
MDTF_EXPORT int mdtf_lamb_moments(const void* items, int nitems, int pbase, const void* w, const void* g, void* m,
                                  void* v, void* partials, float b1, float b2, float eps, float gs, float wd,
                                  const void* dyn, hipStream_t st) {
  if (nitems < 0 || pbase < 0) return MDTF_EINVAL;
  if (nitems == 0) return 0;
  if (!items || !partials || bad_buf(w) || bad_buf(g) || bad_buf(m) || bad_buf(v)) return MDTF_EINVAL;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3(static_cast<unsigned>(nitems)), dim3(kThreads), 0, st,
                     static_cast<const Item*>(items), pbase, static_cast<const float*>(w),
                     static_cast<const float*>(g), static_cast<float*>(m), static_cast<float*>(v),
                     static_cast<float*>(partials), b1, b2, eps, gs, wd, static_cast<const float*>(dyn));
  MDTF_LAUNCH_CHECK();
  return 0;
}

MDTF_EXPORT int mdtf_lamb_apply(const void* items, int nitems, void* w, const void* m, const void* v, void* shadow,
                                const void* ratio, float lr, float eps, float wd, const void* dyn, hipStream_t st) {
  if (nitems < 0) return MDTF_EINVAL;
  if (nitems == 0) return 0;
  if (!items || !ratio || bad_buf(w) || bad_buf(m) || bad_buf(v)) return MDTF_EINVAL;
  if (shadow && (reinterpret_cast<uintptr_t>(shadow) & 7)) return MDTF_EINVAL;
  hipLaunchKernelGGL(lamb_apply_kernel, dim3(static_cast<unsigned>(nitems)), dim3(kThreads), 0, st,
                     static_cast<const Item*>(items), static_cast<float*>(w), static_cast<const float*>(m),
                     static_cast<const float*>(v), static_cast<bf16_t*>(shadow), static_cast<const float*>(ratio), lr,
                     eps, wd, static_cast<const float*>(dyn));
  MDTF_LAUNCH_CHECK();
  return 0;
}

MDTF_EXPORT int mdtf_lars_norms(const void* items, int nitems, int pbase, const void* w, const void* g, void* partials,
                                hipStream_t st) {
  if (nitems < 0 || pbase < 0) return MDTF_EINVAL;
  if (nitems == 0) return 0;
  if (!items || !partials || bad_buf(w) || bad_buf(g)) return MDTF_EINVAL;
  hipLaunchKernelGGL(lars_norms_kernel, dim3(static_cast<unsigned>(nitems)), dim3(kThreads), 0, st,
                     static_cast<const Item*>(items), pbase, static_cast<const float*>(w),
                     static_cast<const float*>(g), static_cast<float*>(partials));
  MDTF_LAUNCH_CHECK();
  return 0;
}

MDTF_EXPORT int mdtf_lars_apply(const void* items, int nitems, void* w, const void* g, void* acc, void* shadow,
                                const void* ratio, float lr, float mom, float gs, float wd, int nesterov,
                                const void* dyn, hipStream_t st) {
  if (nitems < 0) return MDTF_EINVAL;
  if (nitems == 0) return 0;
  if (!items || !ratio || bad_buf(w) || bad_buf(g) || bad_buf(acc)) return MDTF_EINVAL;
  if (shadow && (reinterpret_cast<uintptr_t>(shadow) & 7)) return MDTF_EINVAL;
  hipLaunchKernelGGL(lars_apply_kernel, dim3(static_cast<unsigned>(nitems)), dim3(kThreads), 0, st,
                     static_cast<const Item*>(items), static_cast<float*>(w), static_cast<const float*>(g),
                     static_cast<float*>(acc), static_cast<bf16_t*>(shadow), static_cast<const float*>(ratio), lr, mom,
                     gs, wd, nesterov, static_cast<const float*>(dyn));
  MDTF_LAUNCH_CHECK();
  return 0;
}

// layers: nlayers x {first, count, decay, 0} (int32, device); sums: fp64[2 nlayers]; ratio: fp32[nlayers]
MDTF_EXPORT int mdtf_layer_finalize(const void* layers, int nlayers, const void* partials, void* sums, void* ratio,
                                    int kind, float eeta, float wd, float eps, float gs, const void* dyn, int mode,
                                    hipStream_t st) {
  if (nlayers < 0 || mode < 0 || mode > 2 || kind < 0 || kind > 1) return MDTF_EINVAL;
  if (nlayers == 0) return 0;
  if (!layers || !sums || (mode != 2 && !partials) || (mode != 1 && !ratio)) return MDTF_EINVAL;
  hipLaunchKernelGGL(layer_finalize_kernel, dim3(static_cast<unsigned>(nlayers)), dim3(kThreads), 0, st,
                     static_cast<const Layer*>(layers), static_cast<const float*>(partials),
                     static_cast<double*>(sums), static_cast<float*>(ratio), kind, eeta, wd, eps, gs,
                     static_cast<const float*>(dyn), mode);
  MDTF_LAUNCH_CHECK();
  return 0;
}
