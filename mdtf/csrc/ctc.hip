// tf.nn.ctc_loss on the device: connectionist temporal classification in the log domain, blank = class K - 1.
//
//   ctc_rows        one pass over the logits x [T, B, K].  Per live row (t < T_b): lse in fp32 (one online pass: running
//                   max and rescaled exp-sum) and the L_b + 1 log-probabilities the recurrence reads, gathered into the
//                   compact fp32 lpc[t, b, 0 .. L_b] = x[label_j] - lse (j < L_b), x[K - 1] - lse (j = L_b).  Rows
//                   shorter than 2048 classes get one wave (four rows per block), longer ones a whole block with 16-byte
//                   loads behind a head peeled to the next 16-byte boundary (K need not be a multiple of the vector).
//                   The first B blocks of the same launch build, per item, the occurrence chain of its labels (for
//                   position j: the next position with the same symbol, and whether j is the first) and the
//                   feasibility flag: every label inside [0, K - 1) and L_b + #{j: l_j == l_{j-1}} <= T_b.
//   ctc_alpha_beta  grid (B, 2): block (b, 0) runs alpha with t ascending, block (b, 1) beta with t descending.  Beta is
//                   alpha of the mirrored problem (state S_b - 1 - s, time T_b - 1 - t), so one recurrence serves both:
//                     a_0(0) = lp[0, 0], a_0(1) = lp[0, 1], a_t(s) = lp[t, s] + logadd(a(s), a(s - 1), a(s - 2) if skip)
//                   Wave variant (2 Lmax + 1 <= 64): lane = state, neighbours by __shfl_up, no LDS and no barrier in the
//                   time loop.  Block variant (Lmax <= 511): 256 threads, up to four states each (strided by 256), the
//                   previous row in a double-buffered LDS array behind a two-element -inf apron, one barrier per step.
//                   Both load the next step's lpc values ahead of the current step's math and keep the skip predicate
//                   in a register.  alpha and beta go out as fp32 [T, B, 2 Lmax + 1]; the alpha block writes loss[b].
//                   An infeasible item gets +inf (0 with ignore_longer) and an empty one (T_b = 0, L_b = 0) 0, before
//                   any load of lpc.
//   ctc_grad        one pass over the logits: dx[t, b, k] = g_b (softmax_k - sum_{s: l'_s = k} exp(alpha_t(s) +
//                   beta_t(s) - lp[t, s] + loss_b)).  A row's threads store g_b softmax; after a block barrier the
//                   threads that own a first-occurrence label position, and one for the blank, walk their chain in
//                   position order, sum in fp32 and store their one element again, now with the sum taken off.  Distinct
//                   addresses: no atomics.  Dead rows (t >= T_b) and infeasible items are stored as zeros and nothing
//                   of theirs is read.
//
// No float atomics, no host read, no allocation: two launches make the loss and one the gradient whatever T is, all
// bitwise repeatable and replayable in a hipGraph while the int32 lengths change in place.  Frame lengths are clamped
// to [0, T], label lengths to [0, Lmax].  There is no matrix product in this op, so no MFMA.
#include "mdtf_common.h"

#include <limits.h>

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kRowK = 2048;                      // rows at least this long get a whole block
constexpr int kMaxL = 511;                       // 2 * 511 + 1 = 1023 states: four per thread
constexpr int kSPT = 4;                          // states per thread of the block variant
constexpr int kFirst = 1 << 30;                  // chain[j]: bit 30 = first occurrence, low bits = next position + 1
constexpr int kNextMask = kFirst - 1;
constexpr float kNegInf = -INFINITY;

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
__device__ __forceinline__ void stf(bf16_t* p, long long i, float v) { p[i] = f2bf(v); }
__device__ __forceinline__ void stf(float* p, long long i, float v) { p[i] = v; }

// one 16-byte vector <-> 16 / sizeof(T) floats
template <typename T>
struct Vec;
template <>
struct Vec<bf16_t> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4& q, float (&f)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __uint_as_float(w[i] << 16);
      f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  static __device__ __forceinline__ uint4 pack(const float (&f)[8]) {
    return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
  }
};
template <>
struct Vec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4& q, float (&f)[4]) {
    f[0] = __uint_as_float(q.x), f[1] = __uint_as_float(q.y), f[2] = __uint_as_float(q.z), f[3] = __uint_as_float(q.w);
  }
  static __device__ __forceinline__ uint4 pack(const float (&f)[4]) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  }
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// elements in front of the first 16-byte boundary of a row (the whole row when vectors are off)
template <typename T>
__device__ __forceinline__ int row_head(const T* p, int K, bool vec) {
  if (!vec) return K;
  const int h = static_cast<int>(((16u - (reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
  return h < K ? h : K;
}

// running max and exp-sum relative to it.  A batch that is all -inf leaves m at -inf and adds nothing: exp(-inf + inf)
// is never formed.
struct RowAcc {
  float m = kNegInf, s = 0.f;

  template <int NV>
  __device__ __forceinline__ void eat(const float (&x)[NV]) {
    float mx = x[0];
#pragma unroll
    for (int j = 1; j < NV; ++j) mx = fmaxf(mx, x[j]);
    if (mx > m) {
      s = (m == kNegInf ? 0.f : s * __expf(m - mx));
      m = mx;
    }
    if (m != kNegInf) {
#pragma unroll
      for (int j = 0; j < NV; ++j) s += __expf(x[j] - m);
    }
  }
  __device__ __forceinline__ void eat1(float x) {
    const float one[1] = {x};
    eat(one);
  }
  __device__ __forceinline__ void merge(float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = (m == kNegInf ? 0.f : s * __expf(m - mn)) + (m2 == kNegInf ? 0.f : s2 * __expf(m2 - mn));
    m = mn;
  }
  __device__ __forceinline__ void wave_merge() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) merge(__shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  }
};

// the (max, exp-sum) of one row over the NT threads that share it: scalar loads in front of the first 16-byte boundary
// and behind the last whole vector, 16-byte loads (two in flight) between
template <typename T, int NT>
__device__ __forceinline__ void row_scan(const T* p, int K, int lane, bool vec, RowAcc& a) {
  constexpr int V = Vec<T>::N;
  const int head = row_head(p, K, vec);
  int k = lane;
  for (; k + 3 * NT < head; k += 4 * NT) {
    float x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = ldf(p, k + u * NT);
    a.eat(x);
  }
  for (; k < head; k += NT) a.eat1(ldf(p, k));
  const int nv = (K - head) / V;
  const T* q = p + head;
  float f0[V], f1[V];
  int v = lane;
  for (; v + NT < nv; v += 2 * NT) {
    const uint4 w0 = *reinterpret_cast<const uint4*>(q + (long long)v * V);
    const uint4 w1 = *reinterpret_cast<const uint4*>(q + (long long)(v + NT) * V);
    Vec<T>::unpack(w0, f0);
    Vec<T>::unpack(w1, f1);
    a.eat(f0);
    a.eat(f1);
  }
  for (; v < nv; v += NT) {
    Vec<T>::unpack(*reinterpret_cast<const uint4*>(q + (long long)v * V), f0);
    a.eat(f0);
  }
  for (k = head + nv * V + lane; k < K; k += NT) a.eat1(ldf(p, k));
}

// every element of a row through f(k, x) -> the stored value (READ) or f(k) alone (zero fill), same split as row_scan
template <typename T, int NT, bool READ, typename F>
__device__ __forceinline__ void row_map(const T* p, T* q, int K, int lane, bool vec, F f) {
  constexpr int V = Vec<T>::N;
  const int head = row_head(q, K, vec);
  for (int k = lane; k < head; k += NT) stf(q, k, f(READ ? ldf(p, k) : 0.f));
  const int nv = (K - head) / V;
  for (int v = lane; v < nv; v += NT) {
    float x[V];
    if constexpr (READ) {
      Vec<T>::unpack(*reinterpret_cast<const uint4*>(p + head + (long long)v * V), x);
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) x[i] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < V; ++i) x[i] = f(x[i]);
    *reinterpret_cast<uint4*>(q + head + (long long)v * V) = Vec<T>::pack(x);
  }
  for (int k = head + nv * V + lane; k < K; k += NT) stf(q, k, f(READ ? ldf(p, k) : 0.f));
}

// ------------------------------------------------------------------------------------------------------ ctc_rows
// block b < B: the occurrence chain and the feasibility flag of item b; one thread per label position, O(L) scans
__device__ __forceinline__ void chain_block(const int* __restrict__ labels, const int* __restrict__ seq_len,
                                            const int* __restrict__ lab_len, int b, int T, int K, int Lmax,
                                            int* __restrict__ chain, int* __restrict__ flag) {
  __shared__ int s_bad, s_rep;
  if (threadIdx.x == 0) s_bad = 0, s_rep = 0;
  __syncthreads();
  const int L = clampi(lab_len[b], 0, Lmax), Tb = clampi(seq_len[b], 0, T);
  const int* lab = labels + (long long)b * Lmax;
  int bad = 0, rep = 0;
  for (int j = threadIdx.x; j < Lmax; j += kT) {
    int code = 0;
    if (j < L) {
      const int c = lab[j];
      bad |= (c < 0 || c >= K - 1);
      rep += (j > 0 && lab[j - 1] == c);
      int first = 1, next = -1;
      for (int i = 0; i < j; ++i) first &= (lab[i] != c);
      for (int i = L - 1; i > j; --i) next = (lab[i] == c) ? i : next;
      code = (next + 1) | (first ? kFirst : 0);
    }
    chain[(long long)b * Lmax + j] = code;
  }
  if (bad) atomicOr(&s_bad, 1);                  // integer LDS atomics: order-free
  if (rep) atomicAdd(&s_rep, rep);
  __syncthreads();
  if (threadIdx.x == 0) flag[b] = (!s_bad && L + s_rep <= Tb) ? 1 : 0;
}

template <typename T, int NT>
__global__ void __launch_bounds__(kT) ctc_rows_kernel(const T* __restrict__ x, const int* __restrict__ labels,
                                                      const int* __restrict__ seq_len, const int* __restrict__ lab_len,
                                                      int Tn, int B, int K, int Lmax, int vec, float* __restrict__ lse,
                                                      float* __restrict__ lpc, int* __restrict__ chain,
                                                      int* __restrict__ flag) {
  if (static_cast<int>(blockIdx.x) < B) {
    chain_block(labels, seq_len, lab_len, blockIdx.x, Tn, K, Lmax, chain, flag);
    return;
  }
  constexpr int RPB = kT / NT;
  const long long r = (long long)(blockIdx.x - B) * RPB + threadIdx.x / NT;
  const int lane = threadIdx.x % NT;
  if (r >= (long long)Tn * B) return;            // (uniform over the threads that share a row)
  const int t = static_cast<int>(r / B), b = static_cast<int>(r % B);
  if (t >= clampi(seq_len[b], 0, Tn)) return;    // a dead row is not read
  const T* p = x + r * K;
  RowAcc a;
  row_scan<T, NT>(p, K, lane, vec != 0, a);
  a.wave_merge();
  if constexpr (NT > kWave) {
    __shared__ float sm[NT / kWave], ss[NT / kWave];
    if ((lane & (kWave - 1)) == 0) sm[lane / kWave] = a.m, ss[lane / kWave] = a.s;
    __syncthreads();
    a.m = sm[0], a.s = ss[0];
    for (int i = 1; i < NT / kWave; ++i) a.merge(sm[i], ss[i]);
  }
  const float l = a.m + __logf(a.s);
  if (lane == 0) lse[r] = l;
  const int L = clampi(lab_len[b], 0, Lmax);
  const int* lab = labels + (long long)b * Lmax;
  float* out = lpc + r * (Lmax + 1);
  for (int j = lane; j <= L; j += NT) {
    const int k = j < L ? lab[j] : K - 1;
    out[j] = (k >= 0 && k < K) ? ldf(p, k) - l : kNegInf;      // (a label out of range: the item is infeasible)
  }
}

// ------------------------------------------------------------------------------------------------ ctc_alpha_beta
// log(e^a + e^b + e^c); an all -inf triple stays -inf
__device__ __forceinline__ float logadd3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == kNegInf) return kNegInf;
  return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// what block (b, dir) needs of its item; sp is a state of the mirrored problem, state(sp) the real one
struct Item {
  int L, Tb, Sb, dir;
  long long row0, rstep;                          // first row t * B + b and the step between rows, in time order of dir
  __device__ __forceinline__ int state(int sp) const { return dir ? Sb - 1 - sp : sp; }
  // index into the lpc row of state s: its label position, the blank behind the labels
  __device__ __forceinline__ int lp_index(int s) const { return (s & 1) ? (s >> 1) : L; }
  // whether sp may be entered from sp - 2: a label state whose symbol differs from the one two states back
  __device__ __forceinline__ bool skip(const int* lab, int sp) const {
    if (!(sp & 1) || sp < 2) return false;
    const int s = state(sp), s2 = dir ? s + 2 : s - 2;
    return lab[s >> 1] != lab[s2 >> 1];
  }
};

__device__ __forceinline__ bool item_setup(const int* seq_len, const int* lab_len, const int* flag, int b, int dir,
                                           int Tn, int B, int Lmax, int ignore_longer, float* loss, Item& it) {
  it.L = clampi(lab_len[b], 0, Lmax);
  it.Tb = clampi(seq_len[b], 0, Tn);
  it.Sb = 2 * it.L + 1;
  it.dir = dir;
  const int ok = flag[b];
  if (!ok || it.Tb == 0) {
    if (dir == 0 && threadIdx.x == 0) loss[b] = (ok || ignore_longer) ? 0.f : INFINITY;
    return false;
  }
  it.row0 = dir ? (long long)(it.Tb - 1) * B + b : b;
  it.rstep = dir ? -(long long)B : (long long)B;
  return true;
}

__device__ __forceinline__ float final_loss(float a_last, float a_prev) {
  return -logadd3(a_last, a_prev, kNegInf);
}

__global__ void __launch_bounds__(kWave) ctc_ab_wave_kernel(const float* __restrict__ lpc, const int* __restrict__ labels,
                                                            const int* __restrict__ seq_len,
                                                            const int* __restrict__ lab_len, const int* __restrict__ flag,
                                                            int Tn, int B, int Lmax, int ignore_longer,
                                                            float* __restrict__ alpha, float* __restrict__ beta,
                                                            float* __restrict__ loss) {
  const int b = blockIdx.x, sp = threadIdx.x;
  Item it;
  if (!item_setup(seq_len, lab_len, flag, b, blockIdx.y, Tn, B, Lmax, ignore_longer, loss, it)) return;
  const int S = 2 * Lmax + 1, W = Lmax + 1;
  const bool valid = sp < it.Sb;
  const int s = valid ? it.state(sp) : 0;
  const int li = it.lp_index(s);
  const bool skip = valid && it.skip(labels + (long long)b * Lmax, sp);
  float* out = (it.dir ? beta : alpha) + s;
  long long row = it.row0;
  float lp_next = valid ? lpc[row * W + li] : kNegInf;
  float a = kNegInf;
  for (int tp = 0; tp < it.Tb; ++tp) {
    const float lp = lp_next;
    if (tp + 1 < it.Tb && valid) lp_next = lpc[(row + it.rstep) * W + li];
    float v;
    if (tp == 0) {
      v = sp < 2 ? lp : kNegInf;
    } else {
      float a1 = __shfl_up(a, 1, kWave), a2 = __shfl_up(a, 2, kWave);
      a1 = sp >= 1 ? a1 : kNegInf;
      a2 = skip ? a2 : kNegInf;
      v = lp + logadd3(a, a1, a2);
    }
    a = valid ? v : kNegInf;
    if (valid) out[row * S] = a;
    row += it.rstep;
  }
  const float a_last = __shfl(a, it.Sb - 1, kWave), a_prev = __shfl(a, it.Sb >= 2 ? it.Sb - 2 : 0, kWave);
  if (it.dir == 0 && sp == 0) loss[b] = final_loss(a_last, it.Sb >= 2 ? a_prev : kNegInf);
}

__global__ void __launch_bounds__(kT) ctc_ab_block_kernel(const float* __restrict__ lpc, const int* __restrict__ labels,
                                                          const int* __restrict__ seq_len,
                                                          const int* __restrict__ lab_len, const int* __restrict__ flag,
                                                          int Tn, int B, int Lmax, int ignore_longer,
                                                          float* __restrict__ alpha, float* __restrict__ beta,
                                                          float* __restrict__ loss) {
  // prev[buf][sp + 2] = a(sp) of the step before; [0] and [1] are the -inf apron under states 0 and 1
  __shared__ float prev[2][kSPT * kT + 2];
  const int b = blockIdx.x, tid = threadIdx.x;
  Item it;
  if (!item_setup(seq_len, lab_len, flag, b, blockIdx.y, Tn, B, Lmax, ignore_longer, loss, it)) return;
  const int S = 2 * Lmax + 1, W = Lmax + 1;
  if (tid < 2) prev[0][tid] = kNegInf, prev[1][tid] = kNegInf;
  bool valid[kSPT], skip[kSPT];
  int li[kSPT], so[kSPT];
  float lp_next[kSPT];
  long long row = it.row0;
#pragma unroll
  for (int i = 0; i < kSPT; ++i) {
    const int sp = tid + i * kT;
    valid[i] = sp < it.Sb;
    so[i] = valid[i] ? it.state(sp) : 0;
    li[i] = it.lp_index(so[i]);
    skip[i] = valid[i] && it.skip(labels + (long long)b * Lmax, sp);
    lp_next[i] = valid[i] ? lpc[row * W + li[i]] : kNegInf;
  }
  float* out = it.dir ? beta : alpha;
  for (int tp = 0; tp < it.Tb; ++tp) {
    const int cur = tp & 1;                       // read prev[cur ^ 1], write prev[cur]
    float lp[kSPT];
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
      lp[i] = lp_next[i];
      if (tp + 1 < it.Tb && valid[i]) lp_next[i] = lpc[(row + it.rstep) * W + li[i]];
    }
#pragma unroll
    for (int i = 0; i < kSPT; ++i) {
      if (!valid[i]) continue;
      const int sp = tid + i * kT;
      float v;
      if (tp == 0) {
        v = sp < 2 ? lp[i] : kNegInf;
      } else {
        const float* pr = prev[cur ^ 1] + sp;
        v = lp[i] + logadd3(pr[2], pr[1], skip[i] ? pr[0] : kNegInf);
      }
      prev[cur][sp + 2] = v;
      out[row * S + so[i]] = v;
    }
    row += it.rstep;
    __syncthreads();                              // prev[cur] complete; every read of prev[cur ^ 1] done
  }
  if (it.dir == 0 && tid == 0) {
    const float* pr = prev[(it.Tb - 1) & 1];
    loss[b] = final_loss(pr[it.Sb + 1], pr[it.Sb]);             // states Sb - 1 and Sb - 2 (the apron when Sb == 1)
  }
}

// ------------------------------------------------------------------------------------------------------ ctc_grad
template <typename T, int NT>
__global__ void __launch_bounds__(kT) ctc_grad_kernel(const T* __restrict__ x, const int* __restrict__ labels,
                                                      const int* __restrict__ seq_len, const int* __restrict__ lab_len,
                                                      const int* __restrict__ flag, const int* __restrict__ chain,
                                                      const float* __restrict__ lse, const float* __restrict__ lpc,
                                                      const float* __restrict__ alpha, const float* __restrict__ beta,
                                                      const float* __restrict__ loss, const float* __restrict__ g,
                                                      T* __restrict__ dx, int Tn, int B, int K, int Lmax, int vec) {
  constexpr int RPB = kT / NT;
  const long long r = (long long)blockIdx.x * RPB + threadIdx.x / NT;
  const int lane = threadIdx.x % NT;
  const bool in_range = r < (long long)Tn * B;
  const int t = in_range ? static_cast<int>(r / B) : 0, b = in_range ? static_cast<int>(r % B) : 0;
  const bool live = in_range && flag[b] != 0 && t < clampi(seq_len[b], 0, Tn);
  const T* p = x + r * K;
  T* q = dx + r * K;
  float gb = 0.f, l = 0.f;
  if (live) {
    gb = g[b];
    l = lse[r];
    row_map<T, NT, true>(p, q, K, lane, vec != 0, [&](float v) { return gb * __expf(v - l); });
  } else if (in_range) {
    row_map<T, NT, false>(p, q, K, lane, vec != 0, [](float) { return 0.f; });
  }
  __threadfence_block();
  __syncthreads();                                // the row's softmax is stored before its owners store again
  if (!live) return;
  const int L = clampi(lab_len[b], 0, Lmax), S = 2 * Lmax + 1;
  const int* lab = labels + (long long)b * Lmax;
  const int* ch = chain + (long long)b * Lmax;
  const float* al = alpha + r * S;
  const float* be = beta + r * S;
  const float* lp = lpc + r * (Lmax + 1);
  const float ls = loss[b];
  auto term = [&](int s, float lpj) {
    const float a = al[s], bt = be[s];
    return (a == kNegInf || bt == kNegInf) ? 0.f : __expf(((a + bt) - lpj) + ls);
  };
  for (int j = lane; j <= L; j += NT) {
    int k;
    float sum = 0.f;
    if (j < L) {
      if (!(ch[j] & kFirst)) continue;
      k = lab[j];
      const float lpj = lp[j];
      for (int pos = j; pos >= 0; pos = (ch[pos] & kNextMask) - 1) sum += term(2 * pos + 1, lpj);
    } else {
      k = K - 1;
      const float lpj = lp[L];
      for (int pos = 0; pos <= L; ++pos) sum += term(2 * pos, lpj);
    }
    if (k < 0 || k >= K) continue;                // (labels changed since the forward: never store outside the row)
    stf(q, k, gb * (__expf(ldf(p, k) - l) - sum));
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int check_shape(int T, int B, int K, int Lmax, int dtype) {
  if (T < 0 || B < 0 || Lmax < 0) return MDTF_EINVAL;
  if (Lmax > kMaxL || K < 2 || (dtype != 0 && dtype != 1)) return MDTF_EUNSUPPORTED;
  if ((long long)T * B + B > INT_MAX) return MDTF_EUNSUPPORTED;
  return 0;
}

}  // namespace

// dtype codes of the entry points: 0 bf16, 1 fp32 (the dtype of x and dx).  labels int32 [B, Lmax], seq_len and lab_len
// int32 [B], all read on the device at every launch.
//
// lse fp32 [T, B], lpc fp32 [T, B, Lmax + 1], chain int32 [B, Lmax], flag int32 [B]; rows at t >= T_b are left as they
// are (nothing reads them).
MDTF_EXPORT int mdtf_ctc_rows(const void* x, const int* labels, const int* seq_len, const int* lab_len, float* lse,
                              float* lpc, int* chain, int* flag, int T, int B, int K, int Lmax, int dtype,
                              hipStream_t st) {
  if (const int rc = check_shape(T, B, K, Lmax, dtype)) return rc;
  if (T == 0 || B == 0) return 0;
  if (!x || !seq_len || !lab_len || !lse || !lpc || !flag || (Lmax > 0 && (!labels || !chain))) return MDTF_EINVAL;
  const long long rows = (long long)T * B;
  const int vec = aligned16(x);
  if (K >= kRowK) {
    const dim3 grid(static_cast<unsigned>(B + rows));
    if (dtype == 0)
      hipLaunchKernelGGL((ctc_rows_kernel<bf16_t, kT>), grid, dim3(kT), 0, st, static_cast<const bf16_t*>(x), labels,
                         seq_len, lab_len, T, B, K, Lmax, vec, lse, lpc, chain, flag);
    else
      hipLaunchKernelGGL((ctc_rows_kernel<float, kT>), grid, dim3(kT), 0, st, static_cast<const float*>(x), labels,
                         seq_len, lab_len, T, B, K, Lmax, vec, lse, lpc, chain, flag);
  } else {
    const dim3 grid(static_cast<unsigned>(B + ceil_div(rows, kT / kWave)));
    if (dtype == 0)
      hipLaunchKernelGGL((ctc_rows_kernel<bf16_t, kWave>), grid, dim3(kT), 0, st, static_cast<const bf16_t*>(x), labels,
                         seq_len, lab_len, T, B, K, Lmax, 0, lse, lpc, chain, flag);
    else
      hipLaunchKernelGGL((ctc_rows_kernel<float, kWave>), grid, dim3(kT), 0, st, static_cast<const float*>(x), labels,
                         seq_len, lab_len, T, B, K, Lmax, 0, lse, lpc, chain, flag);
  }
  MDTF_LAUNCH_CHECK();
  return 0;
}

// alpha, beta fp32 [T, B, 2 Lmax + 1] (states of live rows only) and loss fp32 [B] from the buffers of mdtf_ctc_rows
MDTF_EXPORT int mdtf_ctc_alpha_beta(const float* lpc, const int* labels, const int* seq_len, const int* lab_len,
                                    const int* flag, float* alpha, float* beta, float* loss, int ignore_longer, int T,
                                    int B, int K, int Lmax, int dtype, hipStream_t st) {
  if (const int rc = check_shape(T, B, K, Lmax, dtype)) return rc;
  if (B == 0) return 0;
  if (!seq_len || !lab_len || !flag || !loss || (T > 0 && (!lpc || !alpha || !beta)) || (Lmax > 0 && !labels))
    return MDTF_EINVAL;
  if (2 * Lmax + 1 <= kWave)
    hipLaunchKernelGGL(ctc_ab_wave_kernel, dim3(B, 2), dim3(kWave), 0, st, lpc, labels, seq_len, lab_len, flag, T, B,
                       Lmax, ignore_longer, alpha, beta, loss);
  else
    hipLaunchKernelGGL(ctc_ab_block_kernel, dim3(B, 2), dim3(kT), 0, st, lpc, labels, seq_len, lab_len, flag, T, B,
                       Lmax, ignore_longer, alpha, beta, loss);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// dx [T, B, K] in the dtype of x: every element is stored; g fp32 [B] is the upstream gradient, read on the device
MDTF_EXPORT int mdtf_ctc_grad(const void* x, const int* labels, const int* seq_len, const int* lab_len, const int* flag,
                              const int* chain, const float* lse, const float* lpc, const float* alpha,
                              const float* beta, const float* loss, const float* g, void* dx, int T, int B, int K,
                              int Lmax, int dtype, hipStream_t st) {
  if (const int rc = check_shape(T, B, K, Lmax, dtype)) return rc;
  if (T == 0 || B == 0) return 0;
  if (!x || !seq_len || !lab_len || !flag || !lse || !lpc || !alpha || !beta || !loss || !g || !dx ||
      (Lmax > 0 && (!labels || !chain)))
    return MDTF_EINVAL;
  const long long rows = (long long)T * B;
  const int vec = aligned16(x) && aligned16(dx);
#define MDTF_CTC_GRAD(TYPE, NT, GRID, VEC)                                                                            \
  hipLaunchKernelGGL((ctc_grad_kernel<TYPE, NT>), dim3(static_cast<unsigned>(GRID)), dim3(kT), 0, st,                 \
                     static_cast<const TYPE*>(x), labels, seq_len, lab_len, flag, chain, lse, lpc, alpha, beta, loss, \
                     g, static_cast<TYPE*>(dx), T, B, K, Lmax, VEC)
  if (K >= kRowK) {
    if (dtype == 0)
      MDTF_CTC_GRAD(bf16_t, kT, rows, vec);
    else
      MDTF_CTC_GRAD(float, kT, rows, vec);
  } else {
    const long long grid = ceil_div(rows, kT / kWave);
    if (dtype == 0)
      MDTF_CTC_GRAD(bf16_t, kWave, grid, 0);
    else
      MDTF_CTC_GRAD(float, kWave, grid, 0);
  }
#undef MDTF_CTC_GRAD
  MDTF_LAUNCH_CHECK();
  return 0;
}
