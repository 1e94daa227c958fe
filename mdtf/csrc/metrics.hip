// tf.nn.in_top_k and the tf.metrics reduction on the device.
//
//   in_top_k       per row r: t = x[r, label_r] (loaded once, before the sweep), c = #{j in [0, K): x[r, j] > t};
//                  hits[r] = 1 iff label_r lies in [0, K), t is finite and c < k.  The comparison is strict, so every
//                  class tied with the target counts as inside the top k (TF); NaN elsewhere in the row compares false
//                  and is never counted, +inf is, -inf is not.  A row with weight 0 or a label outside [0, K) is
//                  skipped: its logits are never read and hits[r] = 0 (the rule of losses.hip).  No arithmetic is
//                  done on the logits and bf16 -> fp32 is exact, so the result is exact.
//   metric_reduce  one block, a fixed order, fp64: total = wscale sum_r w_r v_r and count = wscale sum_r w_r over the
//                  rows with w_r != 0 (a NaN value under weight 0 reaches nothing); {total, count} is stored to
//                  `pair` and added to `accum`, which only this single block reads and writes: launches on one
//                  stream accumulate in order without atomics.
//
// Nothing is read back by the host, so both launches can sit inside a captured step.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kRowK = 2048;                      // rows at least this long get a whole block (as losses.hip)

template <typename T>
__device__ __forceinline__ float ldf(const T* p, long long i);
template <>
__device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, long long i) {
  return bf2f(p[i]);
}
template <>
__device__ __forceinline__ float ldf<float>(const float* p, long long i) {
  return p[i];
}

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// whether row takes part at all; its label
__device__ __forceinline__ bool row_live(const long long* labels, const float* weights, int row, int K,
                                         long long* lab) {
  *lab = labels[row];
  if (weights && weights[row] == 0.f) return false;
  return *lab >= 0 && *lab < K;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the two bf16 of one 32-bit word against the target
__device__ __forceinline__ int gt2(uint32_t w, float t) {
  return (__uint_as_float(w << 16) > t ? 1 : 0) + (__uint_as_float(w & 0xffff0000u) > t ? 1 : 0);
}

// one wave per row (four rows per block), any element alignment, bf16 or fp32: four strided loads in flight per lane
template <typename T>
__global__ void __launch_bounds__(kT) in_top_k_wave(const T* __restrict__ logits,
                                                    const long long* __restrict__ labels,
                                                    const float* __restrict__ weights, int N, int K, long long ldr,
                                                    int k, float* __restrict__ hits) {
  const int row = blockIdx.x * (kT / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= N) return;
  long long lab;
  if (!row_live(labels, weights, row, K, &lab)) {
    if (lane == 0) hits[row] = 0.f;
    return;
  }
  const T* p = logits + (long long)row * ldr;
  const float t = ldf(p, lab);
  if (!finite_bits(t)) {
    if (lane == 0) hits[row] = 0.f;
    return;
  }
  int c = 0;
  int j = lane;
  for (; j + 3 * kWave < K; j += 4 * kWave) {
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = ldf(p, j + u * kWave);
#pragma unroll
    for (int u = 0; u < 4; ++u) c += x[u] > t ? 1 : 0;
  }
  for (; j < K; j += kWave) c += ldf(p, j) > t ? 1 : 0;
  c = wave_sum_int(c);
  if (lane == 0) hits[row] = c < k ? 1.f : 0.f;
}

// the block's four wave counts through LDS, then the row's result from thread 0
__device__ __forceinline__ void block_finish(int c, int k, int row, float* hits) {
  c = wave_sum_int(c);
  __shared__ int sc[kT / kWave];
  const int tid = threadIdx.x;
  if ((tid & (kWave - 1)) == 0) sc[tid / kWave] = c;
  __syncthreads();
  if (tid == 0) {
    int total = sc[0];
    for (int i = 1; i < kT / kWave; ++i) total += sc[i];
    hits[row] = total < k ? 1.f : 0.f;
  }
}

// one block per row over 4-byte bf16 pairs (K and the stride even, rows 4-byte aligned), four loads in flight
__global__ void __launch_bounds__(kT) in_top_k_row_pair(const bf16_t* __restrict__ logits,
                                                        const long long* __restrict__ labels,
                                                        const float* __restrict__ weights, int K, long long ldr,
                                                        int k, float* __restrict__ hits) {
  const int row = blockIdx.x, tid = threadIdx.x;
  long long lab;
  if (!row_live(labels, weights, row, K, &lab)) {             // block-uniform: nobody reaches the barrier
    if (tid == 0) hits[row] = 0.f;
    return;
  }
  const bf16_t* p = logits + (long long)row * ldr;
  const float t = bf2f(p[lab]);
  if (!finite_bits(t)) {
    if (tid == 0) hits[row] = 0.f;
    return;
  }
  const uint32_t* p2 = reinterpret_cast<const uint32_t*>(p);
  const int K2 = K >> 1;
  int c = 0;
  int j = tid;
  for (; j + 3 * kT < K2; j += 4 * kT) {
    uint32_t wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wv[u] = p2[j + u * kT];
#pragma unroll
    for (int u = 0; u < 4; ++u) c += gt2(wv[u], t);
  }
  for (; j < K2; j += kT) c += gt2(p2[j], t);
  block_finish(c, k, row, hits);
}

// one block per row, rows 16-B aligned with a stride that is a multiple of 8 (the padded decoder's [rows][30720]
// logits): 16-B loads, four in flight per thread over the vectors that lie inside the row; the last, partial vector
// is one more 16-B load (it ends inside the stride) whose columns are masked against K
__global__ void __launch_bounds__(kT) in_top_k_row_v8(const bf16_t* __restrict__ logits,
                                                      const long long* __restrict__ labels,
                                                      const float* __restrict__ weights, int K, long long ldr, int k,
                                                      float* __restrict__ hits) {
  const int row = blockIdx.x, tid = threadIdx.x;
  long long lab;
  if (!row_live(labels, weights, row, K, &lab)) {
    if (tid == 0) hits[row] = 0.f;
    return;
  }
  const bf16_t* p = logits + (long long)row * ldr;
  const float t = bf2f(p[lab]);
  if (!finite_bits(t)) {
    if (tid == 0) hits[row] = 0.f;
    return;
  }
  const int kf = K >> 3;                          // whole vectors
  int c = 0;
  auto gt8 = [&](const uint4& q) { return gt2(q.x, t) + gt2(q.y, t) + gt2(q.z, t) + gt2(q.w, t); };
  int v = tid;
  for (; v + 3 * kT < kf; v += 4 * kT) {
    uint4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const uint4*>(p + (long long)(v + u * kT) * 8);
#pragma unroll
    for (int u = 0; u < 4; ++u) c += gt8(q[u]);
  }
  for (; v < kf; v += kT) c += gt8(*reinterpret_cast<const uint4*>(p + (long long)v * 8));
  if ((K & 7) != 0 && tid == kT - 1) {            // the thread with the fewest whole vectors
    const uint4 q = *reinterpret_cast<const uint4*>(p + (long long)kf * 8);
    const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
    const int rem = K & 7;
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      c += (2 * h < rem && __uint_as_float(wv[h] << 16) > t) ? 1 : 0;
      c += (2 * h + 1 < rem && __uint_as_float(wv[h] & 0xffff0000u) > t) ? 1 : 0;
    }
  }
  block_finish(c, k, row, hits);
}

__global__ void __launch_bounds__(kT) metric_reduce_kernel(const float* __restrict__ values,
                                                           const float* __restrict__ weights, int N, double wscale,
                                                           double* __restrict__ pair, double* __restrict__ accum) {
  __shared__ double rt[kT], rc[kT];
  double tot = 0.0, cnt = 0.0;
  for (int r = threadIdx.x; r < N; r += kT) {
    const double w = weights ? static_cast<double>(weights[r]) : 1.0;
    if (w != 0.0) {                               // skipped, not multiplied: a NaN value stays out
      tot += w * static_cast<double>(values[r]);
      cnt += w;
    }
  }
  rt[threadIdx.x] = tot;
  rc[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      rt[threadIdx.x] += rt[threadIdx.x + o];
      rc[threadIdx.x] += rc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const bool live = N > 0 && wscale != 0.0;       // a scalar weight of 0 skips every row
  const double total = live ? wscale * rt[0] : 0.0, count = live ? wscale * rc[0] : 0.0;
  if (pair) {
    pair[0] = total;
    pair[1] = count;
  }
  if (accum && live) {
    accum[0] += total;
    accum[1] += count;
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// hits[r] (fp32, 0 or 1) of tf.nn.in_top_k.  logits: bf16 or fp32, rows ld >= K elements apart, unit column stride,
// any element alignment; the columns [K, ld) are never counted.  weights (nullable): fp32 [N], only compared with 0.
MDTF_EXPORT int mdtf_in_top_k(const void* logits, int is_bf16, const long long* labels, const float* weights, int N,
                              int K, long long ld, int k, float* hits, hipStream_t st) {
  if (N < 0 || K < 1 || ld < K || k < 1) return MDTF_EINVAL;
  if (N == 0) return 0;
  if (!logits || !labels || !hits) return MDTF_EINVAL;
  const bf16_t* lb = static_cast<const bf16_t*>(logits);
  const dim3 waves(static_cast<unsigned>(ceil_div(N, kT / kWave)));
  if (is_bf16 && K >= kRowK && aligned(logits, 16) && (ld & 7) == 0)
    hipLaunchKernelGGL(in_top_k_row_v8, dim3(N), dim3(kT), 0, st, lb, labels, weights, K, ld, k, hits);
  else if (is_bf16 && K >= kRowK && aligned(logits, 4) && (K & 1) == 0 && (ld & 1) == 0)
    hipLaunchKernelGGL(in_top_k_row_pair, dim3(N), dim3(kT), 0, st, lb, labels, weights, K, ld, k, hits);
  else if (is_bf16)
    hipLaunchKernelGGL(in_top_k_wave<bf16_t>, waves, dim3(kT), 0, st, lb, labels, weights, N, K, ld, k, hits);
  else
    hipLaunchKernelGGL(in_top_k_wave<float>, waves, dim3(kT), 0, st, static_cast<const float*>(logits), labels,
                       weights, N, K, ld, k, hits);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// pair = {total, count} (fp64 [2], nullable) of values [N] under weights [N] (nullable: all 1) times wscale, also
// added to accum (fp64 [2], nullable).  N == 0 writes zeros to pair and leaves accum as it is.
MDTF_EXPORT int mdtf_metric_reduce(const float* values, const float* weights, int N, double wscale, double* pair,
                                   double* accum, hipStream_t st) {
  if (N < 0 || (!pair && !accum) || (N > 0 && !values)) return MDTF_EINVAL;
  hipLaunchKernelGGL(metric_reduce_kernel, dim3(1), dim3(kT), 0, st, values, weights, N, wscale, pair, accum);
  MDTF_LAUNCH_CHECK();
  return 0;
}
