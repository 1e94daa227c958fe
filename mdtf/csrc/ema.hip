// Exponential moving average of the weights over a flat fp32 buffer (one launch per update target).
//
//   ema -= (1 - decay) * (ema - w)           tf.train.ExponentialMovingAverage / assign_moving_average, fp32
//
// written as ema = fma(-omd, ema - w, ema) with contraction off, so every build variant rounds the same way (as
// optim.hip does).  ``omd`` = 1 - decay is formed on the host (in double, rounded to fp32 once) and never here; it
// is read from ``omd_dev[0]`` when that pointer is non-null, else from the scalar argument: a hipGraph-captured
// step bakes kernel arguments, so the per-step decay (``num_updates``) is refreshed in that buffer instead (the
// convention of ``dyn`` in optim.hip).
// Memory-bound, 12 B per parameter: ema read and written once, w read once.  Each block owns one contiguous chunk
// of kEmaVpt * kThreads float4s per stream and issues every load of the chunk before the math (the pattern of
// adam_kernel and the BN streaming passes).  No atomics, no cross-block communication: bitwise repeatable.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kThreads = 256;
constexpr int kEmaVpt = 4;      // float4s per thread and stream: 8 x 16 B loads in flight per thread

inline bool aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// the ema stream is read and written once per step: nontemporal loads / stores (MDTF_NT_OPT=0: cached forms, as
// for the optimizer state streams).  w was written by the optimizer kernel just before and keeps the cached load
// (measured against the nontemporal one in profiles/ema.md).
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ldf4(const float* p, long long i) {
  if constexpr (NT) return __builtin_bit_cast(float4, __builtin_nontemporal_load(reinterpret_cast<const f32x4_t*>(p) + i));
  return reinterpret_cast<const float4*>(p)[i];
}
template <bool NT>
__device__ __forceinline__ void stf4(float* p, long long i, const float4& v) {
  if constexpr (NT)
    __builtin_nontemporal_store(__builtin_bit_cast(f32x4_t, v), reinterpret_cast<f32x4_t*>(p) + i);
  else
    reinterpret_cast<float4*>(p)[i] = v;
}
inline bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e && e[0] ? e[0] != '0' : dflt;
}

__device__ __forceinline__ void ema1(float& e, float w, float omd) {
#pragma clang fp contract(off)
  e = __builtin_fmaf(-omd, e - w, e);
}

template <bool NT>
__global__ void __launch_bounds__(kThreads) ema_kernel(long long n, float* __restrict__ ema, const float* __restrict__ w,
                                                      const float* __restrict__ omd_dev, float omd) {
  if (omd_dev) omd = omd_dev[0];
  const long long n4 = n >> 2;
  const long long base = (long long)blockIdx.x * (kThreads * kEmaVpt) + threadIdx.x;
  float4 ev[kEmaVpt], wv[kEmaVpt];
#pragma unroll
  for (int u = 0; u < kEmaVpt; ++u) {
    const long long i = base + u * kThreads;
    if (i < n4) {
      ev[u] = ldf4<NT>(ema, i);
      wv[u] = ldf4<false>(w, i);
    }
  }
#pragma unroll
  for (int u = 0; u < kEmaVpt; ++u) {
    const long long i = base + u * kThreads;
    if (i >= n4) break;
    ema1(ev[u].x, wv[u].x, omd);
    ema1(ev[u].y, wv[u].y, omd);
    ema1(ev[u].z, wv[u].z, omd);
    ema1(ev[u].w, wv[u].w, omd);
    stf4<NT>(ema, i, ev[u]);
  }
}

}  // namespace

// n must be a multiple of 4 (flat groups are padded to 64 elements), ema and w 16-byte aligned and distinct;
// one block per chunk of 4 * kThreads * kEmaVpt elements (the grid is not capped: 2^31 blocks cover 2^43 elements)
MDTF_EXPORT int mdtf_ema_update(long long n, float* ema, const float* w, const float* omd_dev, float omd,
                                void* stream) {
  if (n < 0 || n % 4 || !ema || !w || !aligned(ema, 16) || !aligned(w, 16) || !aligned(omd_dev, 4)) return MDTF_EINVAL;
  if (n == 0) return 0;
  static const bool nt = env_flag("MDTF_NT_OPT", true);
  const long long nb = ceil_div(n / 4, (long long)kThreads * kEmaVpt);
  if (nb > 0x7fffffffLL) return MDTF_EUNSUPPORTED;
  auto k = nt ? ema_kernel<true> : ema_kernel<false>;
  hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n, ema, w, omd_dev,
                     omd);
  MDTF_LAUNCH_CHECK();
  return 0;
}
