// tf.losses cross entropy on the device: label smoothing, per-example weights, the four reductions.
//
//   xent_w_fwd   one online pass per row: running max m, rescaled exp-sum s and the plain sum t of the logits.
//                loss_r = lse_r - (1 - eps) x[r, label_r] - (eps / K) t_r in fp32; effw_r = weight of the row, 0 for
//                an ignored row (label outside [0, K) or weight 0), whose logits are never read.
//   loss_reduce  one block: num = sum effw_r loss_r and the denominator of the reduction in fp64, a fixed order, no
//                atomics; out = {scale num / den, scale / den} (0 / 0 = 0, TF's div_no_nan).
//   xent_w_bwd   dlogits[r, k] = c_r (exp(x - lse_r) - (1 - eps) [k == label_r] - eps / K) with
//                c_r = upstream[0] coef[0] effw_r (reduced; coef = out + 1) or upstream[r] effw_r (Reduction.NONE);
//                pad columns [K, ldo) and the rows with effw_r == 0 are stored as zeros.
//
// Nothing is read back by the host: the denominator and the upstream gradient stay in device buffers, so a step that
// holds these launches replays as a hipGraph.  mdtf_xent_fwd / mdtf_xent_bwd (kernels.hip) stay as they are for the
// unsmoothed, unweighted default.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kRowK = 2048;                      // rows at least this long get a whole block
constexpr int kGridCap = 4096;

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

// running (max, exp-sum relative to the max, plain sum) of one thread; the plain sum only when SMOOTH (eps > 0)
template <bool SMOOTH>
struct RowAcc {
  float m = -INFINITY, s = 0.f, t = 0.f;

  // NV logits, all inside the row.  A batch that is all -inf (masked classes) leaves m at -inf and adds nothing
  // to s: exp(-inf - (-inf)) is never formed.
  template <int NV>
  __device__ __forceinline__ void eat(const float (&x)[NV]) {
    float mx = x[0];
#pragma unroll
    for (int j = 1; j < NV; ++j) mx = fmaxf(mx, x[j]);
    if constexpr (SMOOTH) {
#pragma unroll
      for (int j = 0; j < NV; ++j) t += x[j];
    }
    if (mx > m) {
      s = (m == -INFINITY ? 0.f : s * __expf(m - mx));
      m = mx;
    }
    if (m != -INFINITY) {
#pragma unroll
      for (int j = 0; j < NV; ++j) s += __expf(x[j] - m);
    }
  }

  // one logit (the tails of a row)
  __device__ __forceinline__ void eat1(float x) {
    const float one[1] = {x};
    eat(one);
  }

  __device__ __forceinline__ void merge(float m2, float s2, float t2) {
    const float mn = fmaxf(m, m2);
    s = (m == -INFINITY ? 0.f : s * __expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
    t += t2;
  }

  __device__ __forceinline__ void wave_merge() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(t, o, 64));
  }
};

// effective weight of a row: 0 when the row is ignored
__device__ __forceinline__ float row_weight(const long long* labels, const float* weights, float wscale, int row,
                                            int K, long long* lab) {
  *lab = labels[row];
  const float w = (weights ? weights[row] : 1.f) * wscale;
  return (*lab >= 0 && *lab < K) ? w : 0.f;
}

// eps == 0 (!SMOOTH) has no smoothing term at all: 0 * t would turn a masked (-inf) class into NaN
template <bool SMOOTH>
__device__ __forceinline__ void row_store(const RowAcc<SMOOTH>& a, float xl, float eps, int K, float w, int weighted,
                                          int row, float* loss, float* lse, float* effw) {
  const float l = a.m + __logf(a.s);
  float v = l - (1.f - eps) * xl;
  if constexpr (SMOOTH) v -= (eps / (float)K) * a.t;
  lse[row] = l;
  loss[row] = weighted ? v * w : v;
  effw[row] = w;
}

__device__ __forceinline__ void row_ignore(int row, float* loss, float* lse, float* effw) {
  lse[row] = 0.f;
  loss[row] = 0.f;
  effw[row] = 0.f;
}

// one wave per row (four rows per block), any element alignment, bf16 or fp32: four strided loads in flight per lane
template <typename T, bool SMOOTH>
__global__ void __launch_bounds__(kT) xent_w_fwd_wave(const T* __restrict__ logits,
                                                      const long long* __restrict__ labels,
                                                      const float* __restrict__ weights, float wscale, int N, int K,
                                                      long long ldr, float eps, int weighted,
                                                      float* __restrict__ loss, float* __restrict__ lse,
                                                      float* __restrict__ effw) {
  const int row = blockIdx.x * (kT / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= N) return;
  long long lab;
  const float w = row_weight(labels, weights, wscale, row, K, &lab);
  if (w == 0.f) {
    if (lane == 0) row_ignore(row, loss, lse, effw);
    return;
  }
  const T* p = logits + (long long)row * ldr;
  RowAcc<SMOOTH> a;
  int k = lane;
  for (; k + 3 * kWave < K; k += 4 * kWave) {
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = ldf(p, k + u * kWave);
    a.eat(x);
  }
  for (; k < K; k += kWave) a.eat1(ldf(p, k));
  a.wave_merge();
  if (lane == 0) row_store(a, ldf(p, lab), eps, K, w, weighted, row, loss, lse, effw);
}

// the block's four waves through LDS, then the row's results from thread 0
template <bool SMOOTH>
__device__ __forceinline__ void block_finish(RowAcc<SMOOTH>& a, const bf16_t* p, long long lab, float eps, int K, float w,
                                             int weighted, int row, float* loss, float* lse, float* effw) {
  a.wave_merge();
  __shared__ float sm[kT / kWave], ss[kT / kWave], st[kT / kWave];
  const int tid = threadIdx.x;
  if ((tid & (kWave - 1)) == 0) {
    sm[tid / kWave] = a.m;
    ss[tid / kWave] = a.s;
    st[tid / kWave] = a.t;
  }
  __syncthreads();
  if (tid == 0) {
    RowAcc<SMOOTH> r;
    r.m = sm[0], r.s = ss[0], r.t = st[0];
    for (int i = 1; i < kT / kWave; ++i) r.merge(sm[i], ss[i], st[i]);
    row_store(r, bf2f(p[lab]), eps, K, w, weighted, row, loss, lse, effw);
  }
}

// one block per row over 4-byte bf16 pairs (K even, rows 4-byte aligned), four loads in flight per thread
template <bool SMOOTH>
__global__ void __launch_bounds__(kT) xent_w_fwd_row_pair(const bf16_t* __restrict__ logits,
                                                          const long long* __restrict__ labels,
                                                          const float* __restrict__ weights, float wscale, int K,
                                                          long long ldr, float eps, int weighted,
                                                          float* __restrict__ loss, float* __restrict__ lse,
                                                          float* __restrict__ effw) {
  const int row = blockIdx.x, tid = threadIdx.x;
  long long lab;
  const float w = row_weight(labels, weights, wscale, row, K, &lab);
  if (w == 0.f) {
    if (tid == 0) row_ignore(row, loss, lse, effw);
    return;
  }
  const bf16_t* p = logits + (long long)row * ldr;
  const uint32_t* p2 = reinterpret_cast<const uint32_t*>(p);
  const int K2 = K >> 1;
  RowAcc<SMOOTH> a;
  int k = tid;
  for (; k + 3 * kT < K2; k += 4 * kT) {
    uint32_t wv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wv[u] = p2[k + u * kT];
    float x[8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[2 * u] = __uint_as_float(wv[u] << 16);
      x[2 * u + 1] = __uint_as_float(wv[u] & 0xffff0000u);
    }
    a.eat(x);
  }
  for (; k < K2; k += kT) {
    const uint32_t wv = p2[k];
    const float x[2] = {__uint_as_float(wv << 16), __uint_as_float(wv & 0xffff0000u)};
    a.eat(x);
  }
  block_finish(a, p, lab, eps, K, w, weighted, row, loss, lse, effw);
}

// one block per row, rows 16-B aligned with a stride that is a multiple of 8 (the padded decoder's [rows][30720]
// logits): 16-B loads, four in flight per thread over the vectors that lie inside the row; the columns of the last,
// partial vector one by one
template <bool SMOOTH>
__global__ void __launch_bounds__(kT) xent_w_fwd_row_v8(const bf16_t* __restrict__ logits,
                                                        const long long* __restrict__ labels,
                                                        const float* __restrict__ weights, float wscale, int K,
                                                        long long ldr, float eps, int weighted,
                                                        float* __restrict__ loss, float* __restrict__ lse,
                                                        float* __restrict__ effw) {
  const int row = blockIdx.x, tid = threadIdx.x;
  long long lab;
  const float w = row_weight(labels, weights, wscale, row, K, &lab);
  if (w == 0.f) {
    if (tid == 0) row_ignore(row, loss, lse, effw);
    return;
  }
  const bf16_t* p = logits + (long long)row * ldr;
  const int kf = K >> 3;                          // whole vectors
  RowAcc<SMOOTH> a;
  auto eat8 = [&](const uint4& q) {
    const uint32_t wv[4] = {q.x, q.y, q.z, q.w};
    float x[8];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      x[2 * h] = __uint_as_float(wv[h] << 16);
      x[2 * h + 1] = __uint_as_float(wv[h] & 0xffff0000u);
    }
    a.eat(x);
  };
  int v = tid;
  for (; v + 3 * kT < kf; v += 4 * kT) {
    uint4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const uint4*>(p + (long long)(v + u * kT) * 8);
#pragma unroll
    for (int u = 0; u < 4; ++u) eat8(q[u]);
  }
  for (; v < kf; v += kT) eat8(*reinterpret_cast<const uint4*>(p + (long long)v * 8));
  if (tid < (K & 7)) a.eat1(bf2f(p[kf * 8 + tid]));
  block_finish(a, p, lab, eps, K, w, weighted, row, loss, lse, effw);
}

// mode: 0 SUM, 1 SUM_OVER_BATCH_SIZE, 2 MEAN, 3 SUM_BY_NONZERO_WEIGHTS
__global__ void __launch_bounds__(kT) loss_reduce_kernel(const float* __restrict__ loss,
                                                         const float* __restrict__ effw, int N, int mode,
                                                         float den_add, float scale, float* __restrict__ out) {
  __shared__ double rn[kT], rw[kT], rc[kT];
  double num = 0.0, wsum = 0.0, cnt = 0.0;
  for (int r = threadIdx.x; r < N; r += kT) {
    const double w = static_cast<double>(effw[r]);
    num += w * static_cast<double>(loss[r]);
    wsum += w;
    cnt += w != 0.0 ? 1.0 : 0.0;
  }
  rn[threadIdx.x] = num;
  rw[threadIdx.x] = wsum;
  rc[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      rn[threadIdx.x] += rn[threadIdx.x + o];
      rw[threadIdx.x] += rw[threadIdx.x + o];
      rc[threadIdx.x] += rc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double den = mode == 0 ? 1.0 : mode == 1 ? static_cast<double>(N) : mode == 2 ? rw[0] : rc[0];
  den += static_cast<double>(den_add);
  const double sc = static_cast<double>(scale);
  out[0] = den == 0.0 ? 0.f : static_cast<float>(sc * rn[0] / den);
  out[1] = den == 0.0 ? 0.f : static_cast<float>(sc / den);
}

__device__ __forceinline__ float row_coef(const float* effw, const float* coef, const float* upstream, int row) {
  const float w = effw[row];
  if (w == 0.f) return 0.f;                      // also keeps a NaN upstream out of an ignored row
  return coef ? upstream[0] * coef[0] * w : upstream[row] * w;
}

// c (p - hot - eps / K) of one logit; hot = 1 - eps; without SMOOTH (eps == 0) the last term is not formed
template <bool SMOOTH>
__device__ __forceinline__ float grad_of(float x, float l, bool is_label, float c, float hot, float epsk) {
  const float g = __expf(x - l) - (is_label ? hot : 0.f);
  if constexpr (SMOOTH) return c * (g - epsk);
  return c * g;
}

// any layout: a grid-stride loop over the N x ldo elements of the output, pad columns included
template <typename T>
__global__ void __launch_bounds__(kT) xent_w_bwd_generic(const T* __restrict__ logits,
                                                         const long long* __restrict__ labels,
                                                         const float* __restrict__ lse,
                                                         const float* __restrict__ effw,
                                                         const float* __restrict__ coef,
                                                         const float* __restrict__ upstream, T* __restrict__ dlogits,
                                                         int N, int K, long long ldi, long long ldo, float eps) {
  const long long total = (long long)N * ldo;
  const float epsk = eps / (float)K;
  for (long long i = blockIdx.x * (long long)kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    const int row = static_cast<int>(i / ldo);
    const int k = static_cast<int>(i - row * ldo);
    float g = 0.f;
    if (k < K && effw[row] != 0.f)
      g = grad_of<true>(ldf(logits, row * ldi + k), lse[row], labels[row] == k, row_coef(effw, coef, upstream, row),
                        1.f - eps, epsk);
    if constexpr (sizeof(T) == 2)
      dlogits[i] = f2bf(g);
    else
      dlogits[i] = g;
  }
}

// bf16 rows, both strides multiples of 8 and both bases 16-B aligned: one block per row, 16-B vectors, two loads in
// flight per thread over the vectors inside the row, the partial vector masked, the vectors past K stored as zeros
template <bool SMOOTH>
__global__ void __launch_bounds__(kT) xent_w_bwd_row_v8(const bf16_t* __restrict__ logits,
                                                        const long long* __restrict__ labels,
                                                        const float* __restrict__ lse,
                                                        const float* __restrict__ effw,
                                                        const float* __restrict__ coef,
                                                        const float* __restrict__ upstream,
                                                        bf16_t* __restrict__ dlogits, int K, long long ldi,
                                                        long long ldo, float eps) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const bf16_t* p = logits + row * ldi;
  bf16_t* q = dlogits + row * ldo;
  const int nv = static_cast<int>(ldo >> 3);
  const uint4 zero = {0u, 0u, 0u, 0u};
  if (effw[row] == 0.f) {
    for (int v = tid; v < nv; v += kT) *reinterpret_cast<uint4*>(q + (long long)v * 8) = zero;
    return;
  }
  const int kf = K >> 3, kv = (K + 7) >> 3;
  const float l = lse[row], c = row_coef(effw, coef, upstream, row), hot = 1.f - eps, epsk = eps / (float)K;
  const long long lab = labels[row];
  auto grad8 = [&](const uint4& w, int v, bool masked) {
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
    uint32_t ov[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int k0 = v * 8 + 2 * h;
      float g0 = grad_of<SMOOTH>(__uint_as_float(wv[h] << 16), l, lab == k0, c, hot, epsk);
      float g1 = grad_of<SMOOTH>(__uint_as_float(wv[h] & 0xffff0000u), l, lab == k0 + 1, c, hot, epsk);
      if (masked) {
        g0 = k0 < K ? g0 : 0.f;
        g1 = k0 + 1 < K ? g1 : 0.f;
      }
      ov[h] = pack_bf2(g0, g1);
    }
    *reinterpret_cast<uint4*>(q + (long long)v * 8) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
  };
  int v = tid;
  for (; v + kT < kf; v += 2 * kT) {
    const uint4 w0 = *reinterpret_cast<const uint4*>(p + (long long)v * 8);
    const uint4 w1 = *reinterpret_cast<const uint4*>(p + (long long)(v + kT) * 8);
    grad8(w0, v, false);
    grad8(w1, v + kT, false);
  }
  for (; v < kf; v += kT) grad8(*reinterpret_cast<const uint4*>(p + (long long)v * 8), v, false);
  if (kv > kf && tid == 0) grad8(*reinterpret_cast<const uint4*>(p + (long long)kf * 8), kf, true);
  for (v = kv + tid; v < nv; v += kT) *reinterpret_cast<uint4*>(q + (long long)v * 8) = zero;
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// Rows of weighted, smoothed sparse softmax cross entropy.  logits: bf16 or fp32, rows ld >= K elements apart, unit
// column stride, any element alignment.  weights (nullable): fp32 [N]; effw_r = weights[r] * wscale, 0 for an ignored
// row.  loss[r] holds loss_r, or effw_r * loss_r when weighted_out is set (Reduction.NONE).
MDTF_EXPORT int mdtf_xent_w_fwd(const void* logits, int is_bf16, const long long* labels, const float* weights,
                                float wscale, int N, int K, long long ld, float eps, int weighted_out, float* loss,
                                float* lse, float* effw, hipStream_t st) {
  if (N < 0 || K < 2 || ld < K || !(eps >= 0.f && eps <= 1.f)) return MDTF_EINVAL;
  if (N == 0) return 0;
  if (!logits || !labels || !loss || !lse || !effw) return MDTF_EINVAL;
  const bf16_t* lb = static_cast<const bf16_t*>(logits);
  const dim3 waves(static_cast<unsigned>(ceil_div(N, kT / kWave)));
  const bool sm = eps > 0.f;
  if (is_bf16 && K >= kRowK && aligned(logits, 16) && (ld & 7) == 0)
    hipLaunchKernelGGL(sm ? xent_w_fwd_row_v8<true> : xent_w_fwd_row_v8<false>, dim3(N), dim3(kT), 0, st, lb, labels,
                       weights, wscale, K, ld, eps, weighted_out, loss, lse, effw);
  else if (is_bf16 && K >= kRowK && aligned(logits, 4) && (K & 1) == 0 && (ld & 1) == 0)
    hipLaunchKernelGGL(sm ? xent_w_fwd_row_pair<true> : xent_w_fwd_row_pair<false>, dim3(N), dim3(kT), 0, st, lb,
                       labels, weights, wscale, K, ld, eps, weighted_out, loss, lse, effw);
  else if (is_bf16)
    hipLaunchKernelGGL((sm ? xent_w_fwd_wave<bf16_t, true> : xent_w_fwd_wave<bf16_t, false>), waves, dim3(kT), 0, st,
                       lb, labels, weights, wscale, N, K, ld, eps, weighted_out, loss, lse, effw);
  else
    hipLaunchKernelGGL((sm ? xent_w_fwd_wave<float, true> : xent_w_fwd_wave<float, false>), waves, dim3(kT), 0, st,
                       static_cast<const float*>(logits), labels, weights, wscale, N, K, ld, eps, weighted_out, loss,
                       lse, effw);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// out[0] = scale * sum_r effw_r loss_r / den, out[1] = scale / den; den by mode (0 SUM: 1, 1 SUM_OVER_BATCH_SIZE: N,
// 2 MEAN: sum effw, 3 SUM_BY_NONZERO_WEIGHTS: rows with effw != 0) plus den_add; both 0 when den == 0
MDTF_EXPORT int mdtf_loss_reduce(const float* loss, const float* effw, int N, int mode, float den_add, float scale,
                                 float* out, hipStream_t st) {
  if (N < 0 || mode < 0 || mode > 3 || !out || (N > 0 && (!loss || !effw))) return MDTF_EINVAL;
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(kT), 0, st, loss, effw, N, mode, den_add, scale, out);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// dlogits (the logits' dtype, rows ldo >= K apart) of mdtf_xent_w_fwd; coef (nullable): out + 1 of mdtf_loss_reduce
// with upstream a device scalar, null: upstream holds one value per row.  Every element of the N x ldo output is
// stored, the columns [K, ldo) as zeros.
MDTF_EXPORT int mdtf_xent_w_bwd(const void* logits, int is_bf16, const long long* labels, const float* lse,
                                const float* effw, const float* coef, const float* upstream, void* dlogits, int N,
                                int K, long long ldi, long long ldo, float eps, hipStream_t st) {
  if (N < 0 || K < 2 || ldi < K || ldo < K || !(eps >= 0.f && eps <= 1.f)) return MDTF_EINVAL;
  if (N == 0) return 0;
  if (!logits || !labels || !lse || !effw || !upstream || !dlogits) return MDTF_EINVAL;
  const long long blocks = ceil_div((long long)N * ldo, (long long)kT);
  const dim3 grid(static_cast<unsigned>(blocks < kGridCap ? blocks : kGridCap));
  if (is_bf16 && (ldi & 7) == 0 && (ldo & 7) == 0 && aligned(logits, 16) && aligned(dlogits, 16))
    hipLaunchKernelGGL(eps > 0.f ? xent_w_bwd_row_v8<true> : xent_w_bwd_row_v8<false>, dim3(N), dim3(kT), 0, st,
                       static_cast<const bf16_t*>(logits), labels, lse, effw, coef, upstream,
                       static_cast<bf16_t*>(dlogits), K, ldi, ldo, eps);
  else if (is_bf16)
    hipLaunchKernelGGL(xent_w_bwd_generic<bf16_t>, grid, dim3(kT), 0, st, static_cast<const bf16_t*>(logits), labels,
                       lse, effw, coef, upstream, static_cast<bf16_t*>(dlogits), N, K, ldi, ldo, eps);
  else
    hipLaunchKernelGGL(xent_w_bwd_generic<float>, grid, dim3(kT), 0, st, static_cast<const float*>(logits), labels,
                       lse, effw, coef, upstream, static_cast<float*>(dlogits), N, K, ldi, ldo, eps);
  MDTF_LAUNCH_CHECK();
  return 0;
}
