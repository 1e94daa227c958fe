// Device helpers shared by the per-step recurrent kernels (lstm.hip, gru.hip): the skinny MFMA GEMM of a 16-row batch
// tile with K split over the four waves of a block, its operands loaded straight into VGPRs through a two-slot
// register ring, the reduction of the four partial tiles through LDS in wave order, and the fast gate nonlinearities.
// Everything has internal linkage: each including file gets its own copy.
#pragma once
#include "mdtf_common.h"

using namespace mdtf;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kRows = 16;      // batch rows per block (one MFMA tile)
constexpr int kWaves = 4;      // K is split over the waves of a block
constexpr int kRing = 2;       // register load ring depth, in k-steps of one wave
constexpr int kStep = 32;      // K per MFMA

__device__ __forceinline__ float rcp_fast(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ float sigmoid_fast(float v) { return rcp_fast(1.0f + __expf(-v)); }
// 2 sigmoid(2v) - 1; the exponent saturates to inf / 0 at both ends, which gives -1 / 1
__device__ __forceinline__ float tanh_fast(float v) { return 2.0f * rcp_fast(1.0f + __expf(-2.0f * v)) - 1.0f; }

__device__ __forceinline__ bf16x8_t load_frag(const bf16_t* p, bool ok) {
  uint4 raw = make_uint4(0u, 0u, 0u, 0u);
  if (ok) raw = *reinterpret_cast<const uint4*>(p);
  return __builtin_bit_cast(bf16x8_t, raw);
}

// acc[s] (16 rows x 16 columns, this wave's share of K) for NB column strips: rows `arow`-relative of A [.., lda]
// against the strips Bm + s * 16 * ldb, each 16 rows of a K-contiguous [.., ldb] matrix.  Lane l holds row / column
// l % 16 and the k-octet l / 16 of each 32-wide step; a row at or past `a_ok` is read as zeros.
template <int NB>
__device__ __forceinline__ void skinny_gemm(const bf16_t* __restrict__ a_lane, bool a_ok,
                                            const bf16_t* __restrict__ b_lane, int64_t strip, int nsteps, int wave,
                                            float4v (&acc)[NB]) {
  bf16x8_t ra[kRing], rb[kRing][NB];
#pragma unroll
  for (int d = 0; d < kRing; ++d) {
    const int s = wave + d * kWaves;
    if (s < nsteps) {
      ra[d] = load_frag(a_lane + s * kStep, a_ok);
#pragma unroll
      for (int n = 0; n < NB; ++n) rb[d][n] = load_frag(b_lane + n * strip + s * kStep, true);
    }
  }
  for (int s0 = wave; s0 < nsteps; s0 += kRing * kWaves) {
#pragma unroll
    for (int d = 0; d < kRing; ++d) {
      const int s = s0 + d * kWaves;
      if (s < nsteps) {
        const bf16x8_t fa = ra[d];
        bf16x8_t fb[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n) fb[n] = rb[d][n];
        const int nx = s + kRing * kWaves;           // refill the slot just read
        if (nx < nsteps) {
          ra[d] = load_frag(a_lane + nx * kStep, a_ok);
#pragma unroll
          for (int n = 0; n < NB; ++n) rb[d][n] = load_frag(b_lane + n * strip + nx * kStep, true);
        }
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[n], acc[n], 0, 0, 0);
      }
    }
  }
}

// The four waves' partial tiles -> LDS -> this wave's quarter, summed in wave order.  red: [kWaves][NB][4][64] floats.
// Wave w ends up with out[n] = the sum of accumulator slot j = w of strip n (row (l / 16) * 4 + w, column l % 16).
template <int NB>
__device__ __forceinline__ void reduce_waves(float* red, const float4v (&acc)[NB], int wave, int lane,
                                             float (&out)[NB]) {
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[((wave * NB + n) * 4 + j) * kWave + lane] = acc[n][j];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    float v = red[((0 * NB + n) * 4 + wave) * kWave + lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += red[((w * NB + n) * 4 + wave) * kWave + lane];
    out[n] = v;
  }
}

}  // namespace
