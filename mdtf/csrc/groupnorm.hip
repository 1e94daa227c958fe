// tf.contrib.layers.group_norm on bf16 NHWC: x [N, H, W, C], fp32 gamma / beta [C], G groups of Cg = C / G adjacent
// channels, fp32 statistics mean / rstd [N, G] over the m = H * W * Cg elements of an (image, group).
//
//   xhat = (x - mean) * rstd      pre = xhat * gamma[c] + beta[c]      y = act(pre), act in {none, relu}
//   dz = dy * [pre > 0] (relu) or dy      A = sum dz * gamma      Q = sum dz * gamma * xhat     (per image and group)
//   dx = rstd * (dz * gamma - A / m - xhat * Q / m)      dgamma[c] = sum dz * xhat      dbeta[c] = sum dz
//
// A lane owns one 16-byte vector of 8 adjacent channels of some pixels and keeps eight per-channel fp32 sums.  The
// block adds them over its pixel lanes through LDS in a fixed order (fold_rows), and only then are channels folded
// into groups (serially per group, in channel order), so a group may start and end anywhere inside a vector:
// Cg = 1, 2, 3, ... need no special case.  Variances are always sums of squares about a mean that is already known;
// E[x^2] - mean^2 is never formed.  The ReLU mask of the backward is recomputed through gn_xhat / gn_pre, the inline
// functions the forward uses, so both passes take the same decision for every element; no mask is stored.
//
// Two designs, chosen per call (path: 0 auto, 1 resident, 2 streaming):
//
// resident   A block owns one image's strip of S adjacent groups (S * Cg a multiple of 8, so a strip is whole
//            vectors, widened to at most 128 bytes per pixel while it fits) and stages it in LDS with 16-byte loads,
//            up to 8 per lane in flight before any of them is used.  Sum -> group mean -> squares about that mean
//            from LDS -> normalise from LDS: x is read from memory once and y written once.  The backward stages the
//            x and dy strips (half the pixels fit), folds sum dz and sum dz * xhat per channel, stores them as
//            [N, C, 2] partials for the parameter gradients, folds them with gamma into A, Q and writes dx from LDS.
//            Strips of one image are adjacent block indices.
// streaming  gn_stats: a block owns a chunk of 8 * (256 / (C / 8)) pixels of one image, all channels, held in
//            registers (8 vectors per lane): per-channel sums -> per-group chunk mean -> M2 about it from the
//            registers -> (count, sum, M2) per (image, chunk, group).  gn_finalize: one thread per (image, group)
//            merges the triples in chunk order in fp64 (Chan).  gn_apply: the same chunks, nontemporal stores.
//            Backward: gn_bwd_stats (per-channel partials of a few adjacent chunks per block, so that the rows stay
//            near 2048), gn_bwd_finalize (A / m, Q / m), gn_bwd_dx.
//
// gn_param_finalize (both paths): a block per 8 channels adds the partial rows in fp64 in a fixed order (32 row lanes,
// each in row order, then the lanes in order) and stores to, or adds into, the fp32 gradient slots.
//
// No float atomics, no host reads, no allocation: every element of every output and workspace has one writer per
// launch, the launches replay inside a captured step and the results are bitwise repeatable.  C % 8 == 0,
// C <= 2048 and C % G == 0, or MDTF_EINVAL.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kVec = 8;                          // vectors a lane has in flight (resident) or owns (streaming)
constexpr int kMaxC = 2048;                      // C / 8 <= kT: one lane per channel vector of a pixel
constexpr int kLds = 65536;                      // resident: strip(s) + reduction scratch of a block
constexpr int kWideCh = 64;                      // resident: widen a strip up to 128 bytes per pixel

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(const uint4 raw, float (&f)[8]) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}

__device__ __forceinline__ void store_nt(bf16_t* p, const uint4 v) {
  const u32x4_t w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, reinterpret_cast<u32x4_t*>(p));
}

// The normalised value and the pre-activation: the only place either is formed, forward and backward.
__device__ __forceinline__ float gn_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float gn_pre(float xhat, float g, float b) { return __builtin_fmaf(xhat, g, b); }

// What a lane needs for its 8 channels: the statistics of each channel's group and the affine parameters.
struct Lane8 {
  float mu[8], rs[8], g[8], b[8];
};

template <bool RELU>
__device__ __forceinline__ uint4 gn_y8(const uint4 xv, const Lane8& L) {
  float f[8];
  unpack8(xv, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float pre = gn_pre(gn_xhat(f[k], L.mu[k], L.rs[k]), L.g[k], L.b[k]);
    f[k] = RELU ? (pre > 0.f ? pre : 0.f) : pre;
  }
  return pack8(f);
}

// dz and xhat of 8 elements
template <bool RELU>
__device__ __forceinline__ void gn_dz8(const uint4 xv, const uint4 dv, const Lane8& L, float (&dz)[8],
                                       float (&xh)[8]) {
  float f[8];
  unpack8(xv, f);
  unpack8(dv, dz);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    xh[k] = gn_xhat(f[k], L.mu[k], L.rs[k]);
    if (RELU && !(gn_pre(xh[k], L.g[k], L.b[k]) > 0.f)) dz[k] = 0.f;
  }
}

// a[k] = A / m, q[k] = Q / m of the channel's group
__device__ __forceinline__ uint4 gn_dx8(const float (&dz)[8], const float (&xh)[8], const Lane8& L,
                                        const float (&a)[8], const float (&q)[8]) {
  float o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = L.rs[k] * (dz[k] * L.g[k] - a[k] - xh[k] * q[k]);
  return pack8(o);
}

__device__ __forceinline__ void put_row(float* red, int lane, int CH, int v, const float (&a)[8]) {
  float* o = red + lane * CH + v * 8;             // a multiple of 8 floats from a 16-byte aligned base
  reinterpret_cast<float4*>(o)[0] = make_float4(a[0], a[1], a[2], a[3]);
  reinterpret_cast<float4*>(o)[1] = make_float4(a[4], a[5], a[6], a[7]);
}

// out[c] = sum over the PL rows of red[row][c], c < CH, in a fixed order: J = min(PL, kT / CH) runs of adjacent rows,
// each in row order, then the runs in order (CH >= kT: one run).  part: kT floats.  Every thread calls it; it
// begins and ends with a barrier, so red and part may be reused at once.
__device__ void fold_rows(const float* red, float* part, float* out, int PL, int CH) {
  const int tid = threadIdx.x;
  const int J = CH >= kT ? 1 : (PL < kT / CH ? PL : kT / CH);
  __syncthreads();
  if (J == 1) {
    for (int c = tid; c < CH; c += kT) {
      float s = 0.f;
      for (int r = 0; r < PL; ++r) s += red[r * CH + c];
      out[c] = s;
    }
  } else {
    const int Lr = (PL + J - 1) / J;
    if (tid < J * CH) {
      const int j = tid / CH, c = tid - j * CH;
      const int hi = (j + 1) * Lr < PL ? (j + 1) * Lr : PL;
      float s = 0.f;
      for (int r = j * Lr; r < hi; ++r) s += red[r * CH + c];
      part[tid] = s;
    }
    __syncthreads();
    if (tid < CH) {
      float s = 0.f;
      for (int j = 0; j < J; ++j) s += part[j * CH + tid];
      out[tid] = s;
    }
  }
  __syncthreads();
}

// sum of the Cg channel values of group j, in channel order, optionally weighted (gamma)
__device__ __forceinline__ float group_sum(const float* ch, const float* wt, int j, int Cg) {
  float s = 0.f;
  for (int c = j * Cg; c < (j + 1) * Cg; ++c) s += wt ? ch[c] * wt[c] : ch[c];
  return s;
}

// ------------------------------------------------------------------------------------------------- resident
struct ResPlan {
  int S, SV, PL, CH, strips, lds;                // groups, vectors, pixel lanes, channels of a strip; 0 lds: no fit
};

template <bool RELU>
__global__ void __launch_bounds__(kT) gn_res_fwd_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                        float* __restrict__ mean, float* __restrict__ rstd, int HW,
                                                        int C, int G, int Cg, ResPlan pl, float eps) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint4* sx = reinterpret_cast<uint4*>(lds);
  float* red = reinterpret_cast<float*>(lds + (size_t)HW * pl.SV * 16);
  float* part = red + pl.PL * pl.CH;
  float* ch = part + kT;
  float* gmu = ch + pl.CH;
  float* grs = gmu + pl.S;
  const int strip = blockIdx.x % pl.strips, n = blockIdx.x / pl.strips;
  const int cbase = strip * pl.CH;
  const int tid = threadIdx.x, sv = tid % pl.SV, lane = tid / pl.SV;
  const bool active = lane < pl.PL;
  const long long off = (long long)n * HW * C + cbase + sv * 8;
  const float m = static_cast<float>(HW) * static_cast<float>(Cg);

  // stage the strip, up to kVec loads in flight, and sum per channel
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    for (int p0 = lane; p0 < HW; p0 += kVec * pl.PL) {
      uint4 r[kVec];
#pragma unroll
      for (int i = 0; i < kVec; ++i) {
        const int p = p0 + i * pl.PL;
        r[i] = make_uint4(0u, 0u, 0u, 0u);
        if (p < HW) r[i] = *reinterpret_cast<const uint4*>(x + off + (long long)p * C);
      }
#pragma unroll
      for (int i = 0; i < kVec; ++i) {
        const int p = p0 + i * pl.PL;
        if (p < HW) {
          sx[p * pl.SV + sv] = r[i];
          float f[8];
          unpack8(r[i], f);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[k] += f[k];
        }
      }
    }
    put_row(red, lane, pl.CH, sv, acc);
  }
  fold_rows(red, part, ch, pl.PL, pl.CH);
  if (tid < pl.S) gmu[tid] = group_sum(ch, nullptr, tid, Cg) / m;
  __syncthreads();

  // squares about the group mean, from LDS (a lane reads back what it stored)
  Lane8 L;
  int gi[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gi[k] = (sv * 8 + k) / Cg;
    L.mu[k] = gmu[gi[k]];
    acc[k] = 0.f;
  }
  if (active) {
    for (int p = lane; p < HW; p += pl.PL) {
      float f[8];
      unpack8(sx[p * pl.SV + sv], f);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = f[k] - L.mu[k];
        acc[k] += d * d;
      }
    }
    put_row(red, lane, pl.CH, sv, acc);
  }
  fold_rows(red, part, ch, pl.PL, pl.CH);
  if (tid < pl.S) {
    const float r = rsqrtf(group_sum(ch, nullptr, tid, Cg) / m + eps);
    grs[tid] = r;
    mean[(long long)n * G + strip * pl.S + tid] = gmu[tid];
    rstd[(long long)n * G + strip * pl.S + tid] = r;
  }
  __syncthreads();

  if (active) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      L.rs[k] = grs[gi[k]];
      L.g[k] = gamma[cbase + sv * 8 + k];
      L.b[k] = beta[cbase + sv * 8 + k];
    }
    for (int p = lane; p < HW; p += pl.PL)
      *reinterpret_cast<uint4*>(y + off + (long long)p * C) = gn_y8<RELU>(sx[p * pl.SV + sv], L);
  }
}

template <bool RELU>
__global__ void __launch_bounds__(kT) gn_res_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                        float* __restrict__ wsp, int HW, int C, int G, int Cg,
                                                        ResPlan pl) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  uint4* sx = reinterpret_cast<uint4*>(lds);
  uint4* sd = sx + (size_t)HW * pl.SV;
  float* red = reinterpret_cast<float*>(sd + (size_t)HW * pl.SV);
  float* part = red + pl.PL * pl.CH;
  float* ch1 = part + kT;
  float* ch2 = ch1 + pl.CH;
  float* ga = ch2 + pl.CH;
  float* gq = ga + pl.S;
  const int strip = blockIdx.x % pl.strips, n = blockIdx.x / pl.strips;
  const int cbase = strip * pl.CH;
  const int tid = threadIdx.x, sv = tid % pl.SV, lane = tid / pl.SV;
  const bool active = lane < pl.PL;
  const long long off = (long long)n * HW * C + cbase + sv * 8;
  const float m = static_cast<float>(HW) * static_cast<float>(Cg);

  Lane8 L;
  int gi[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gi[k] = (sv * 8 + k) / Cg;
    L.mu[k] = mean[(long long)n * G + strip * pl.S + gi[k]];
    L.rs[k] = rstd[(long long)n * G + strip * pl.S + gi[k]];
    L.g[k] = gamma[cbase + sv * 8 + k];
    L.b[k] = beta[cbase + sv * 8 + k];
  }
  float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (active) {
    for (int p0 = lane; p0 < HW; p0 += (kVec / 2) * pl.PL) {
      uint4 rx[kVec / 2], rd[kVec / 2];
#pragma unroll
      for (int i = 0; i < kVec / 2; ++i) {
        const int p = p0 + i * pl.PL;
        rx[i] = rd[i] = make_uint4(0u, 0u, 0u, 0u);
        if (p < HW) {
          rx[i] = *reinterpret_cast<const uint4*>(x + off + (long long)p * C);
          rd[i] = *reinterpret_cast<const uint4*>(dy + off + (long long)p * C);
        }
      }
#pragma unroll
      for (int i = 0; i < kVec / 2; ++i) {
        const int p = p0 + i * pl.PL;
        if (p < HW) {
          sx[p * pl.SV + sv] = rx[i];
          sd[p * pl.SV + sv] = rd[i];
          float dz[8], xh[8];
          gn_dz8<RELU>(rx[i], rd[i], L, dz, xh);
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            s1[k] += dz[k];
            s2[k] += dz[k] * xh[k];
          }
        }
      }
    }
    put_row(red, lane, pl.CH, sv, s1);
  }
  fold_rows(red, part, ch1, pl.PL, pl.CH);
  if (active) put_row(red, lane, pl.CH, sv, s2);
  fold_rows(red, part, ch2, pl.PL, pl.CH);
  for (int c = tid; c < pl.CH; c += kT)
    *reinterpret_cast<float2*>(wsp + ((long long)n * C + cbase + c) * 2) = make_float2(ch1[c], ch2[c]);
  if (tid < pl.S) {
    ga[tid] = group_sum(ch1, gamma + cbase, tid, Cg) / m;
    gq[tid] = group_sum(ch2, gamma + cbase, tid, Cg) / m;
  }
  __syncthreads();
  if (active) {
    float a[8], q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      a[k] = ga[gi[k]];
      q[k] = gq[gi[k]];
    }
    for (int p = lane; p < HW; p += pl.PL) {
      float dz[8], xh[8];
      gn_dz8<RELU>(sx[p * pl.SV + sv], sd[p * pl.SV + sv], L, dz, xh);
      *reinterpret_cast<uint4*>(dx + off + (long long)p * C) = gn_dx8(dz, xh, L, a, q);
    }
  }
}

// ------------------------------------------------------------------------------------------------ streaming
// A block: chunk k of image n, pixels [k * chunk, min(HW, (k + 1) * chunk)), chunk = kVec * PL, PL = kT / (C / 8).
struct Chunk {
  int n, p0, np, cv, lane;                       // image, first pixel, pixels, the lane's channel vector and pixel lane
  bool active;
  long long off;                                 // element offset of the lane's first vector
};

__device__ __forceinline__ Chunk chunk_at(int n, int k, int HW, int C) {
  Chunk ck;
  const int CV = C >> 3, PL = kT / CV;
  ck.n = n;
  ck.p0 = k * kVec * PL;
  ck.np = HW - ck.p0 < kVec * PL ? HW - ck.p0 : kVec * PL;
  ck.cv = threadIdx.x % CV;
  ck.lane = threadIdx.x / CV;
  ck.active = ck.lane < PL;
  ck.off = ((long long)ck.n * HW + ck.p0 + ck.lane) * C + ck.cv * 8;
  return ck;
}

__device__ __forceinline__ Chunk chunk_of(int HW, int C, int K) {
  return chunk_at(blockIdx.x / K, blockIdx.x % K, HW, C);
}

// the lane's vectors of its chunk (pixel lane + i * PL of the chunk), zeros past the chunk's end: all loads first
__device__ __forceinline__ void load_chunk(const bf16_t* __restrict__ src, const Chunk& ck, int C, uint4 (&r)[kVec]) {
  const int PL = kT / (C >> 3);
#pragma unroll
  for (int i = 0; i < kVec; ++i) {
    r[i] = make_uint4(0u, 0u, 0u, 0u);
    if (ck.active && ck.lane + i * PL < ck.np)
      r[i] = *reinterpret_cast<const uint4*>(src + ck.off + (long long)i * PL * C);
  }
}

__device__ __forceinline__ void lane_stats(const float* __restrict__ mean, const float* __restrict__ rstd,
                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                           const Chunk& ck, int G, int Cg, Lane8& L, int (&gi)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    gi[k] = (ck.cv * 8 + k) / Cg;
    L.mu[k] = mean[(long long)ck.n * G + gi[k]];
    L.rs[k] = rstd[(long long)ck.n * G + gi[k]];
    L.g[k] = gamma[ck.cv * 8 + k];
    L.b[k] = beta[ck.cv * 8 + k];
  }
}

__global__ void __launch_bounds__(kT) gn_stats_kernel(const bf16_t* __restrict__ x, float* __restrict__ ws, int HW,
                                                      int C, int G, int Cg, int K) {
  __shared__ __attribute__((aligned(16))) float red[kT * 8];
  __shared__ float part[kT], ch[kMaxC], gm[kMaxC];
  const Chunk ck = chunk_of(HW, C, K);
  const int PL = kT / (C >> 3), tid = threadIdx.x;
  uint4 r[kVec];
  load_chunk(x, ck, C, r);
  float f[kVec][8], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < kVec; ++i) {
    unpack8(r[i], f[i]);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += f[i][k];
  }
  if (ck.active) put_row(red, ck.lane, C, ck.cv, acc);
  fold_rows(red, part, ch, PL, C);
  const float cnt = static_cast<float>(ck.np) * static_cast<float>(Cg);
  float* out = ws + (long long)blockIdx.x * G * 3;
  for (int g = tid; g < G; g += kT) {
    const float s = group_sum(ch, nullptr, g, Cg);
    gm[g] = s / cnt;
    out[g * 3] = cnt;
    out[g * 3 + 1] = s;
  }
  __syncthreads();
  float mu[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    mu[k] = gm[(ck.cv * 8 + k) / Cg];
    acc[k] = 0.f;
  }
#pragma unroll
  for (int i = 0; i < kVec; ++i)
    if (ck.lane + i * PL < ck.np) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = f[i][k] - mu[k];
        acc[k] += d * d;
      }
    }
  if (ck.active) put_row(red, ck.lane, C, ck.cv, acc);
  fold_rows(red, part, ch, PL, C);
  for (int g = tid; g < G; g += kT) out[g * 3 + 2] = group_sum(ch, nullptr, g, Cg);
}

// one thread per (image, group): Chan's merge of the chunk triples in chunk order, in fp64
__global__ void __launch_bounds__(kT) gn_finalize_kernel(const float* __restrict__ ws, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int NG, int G, int K, float m,
                                                         float eps) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= NG) return;
  const int n = e / G, g = e - n * G;
  double na = 0.0, mu = 0.0, m2 = 0.0;
  for (int k = 0; k < K; ++k) {
    const float* t = ws + (((long long)n * K + k) * G + g) * 3;
    const double nb = t[0], mb = static_cast<double>(t[1]) / nb, d = mb - mu, nn = na + nb;
    mu += d * nb / nn;
    m2 += static_cast<double>(t[2]) + d * d * na * nb / nn;
    na = nn;
  }
  mean[e] = static_cast<float>(mu);
  rstd[e] = rsqrtf(static_cast<float>(m2 / static_cast<double>(m)) + eps);
}

template <bool RELU>
__global__ void __launch_bounds__(kT) gn_apply_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const float* __restrict__ mean,
                                                      const float* __restrict__ rstd, bf16_t* __restrict__ y, int HW,
                                                      int C, int G, int Cg, int K) {
  const Chunk ck = chunk_of(HW, C, K);
  const int PL = kT / (C >> 3);
  if (!ck.active) return;
  uint4 r[kVec];
  load_chunk(x, ck, C, r);
  Lane8 L;
  int gi[8];
  lane_stats(mean, rstd, gamma, beta, ck, G, Cg, L, gi);
#pragma unroll
  for (int i = 0; i < kVec; ++i)
    if (ck.lane + i * PL < ck.np) store_nt(y + ck.off + (long long)i * PL * C, gn_y8<RELU>(r[i], L));
}

template <bool RELU>
__global__ void __launch_bounds__(kT) gn_bwd_stats_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, float* __restrict__ wsp,
                                                          int HW, int C, int G, int Cg, int K, int span) {
  __shared__ __attribute__((aligned(16))) float red[kT * 8];
  __shared__ float part[kT], ch1[kMaxC], ch2[kMaxC];
  const int K2 = (K + span - 1) / span;          // a block: `span` adjacent chunks of one image, one partial row
  const int n = blockIdx.x / K2, k0 = (blockIdx.x - n * K2) * span;
  Chunk ck = chunk_at(n, k0, HW, C);
  const int PL = kT / (C >> 3), tid = threadIdx.x;
  Lane8 L;
  int gi[8];
  lane_stats(mean, rstd, gamma, beta, ck, G, Cg, L, gi);
  float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int kc = k0; kc < k0 + span && kc < K; ++kc) {
    ck = chunk_at(n, kc, HW, C);
    uint4 rx[kVec], rd[kVec];
    load_chunk(x, ck, C, rx);
    load_chunk(dy, ck, C, rd);
#pragma unroll
    for (int i = 0; i < kVec; ++i) {             // past the chunk's end dy is 0: dz = 0 whatever pre is
      float dz[8], xh[8];
      gn_dz8<RELU>(rx[i], rd[i], L, dz, xh);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        s1[k] += dz[k];
        s2[k] += dz[k] * xh[k];
      }
    }
  }
  if (ck.active) put_row(red, ck.lane, C, ck.cv, s1);
  fold_rows(red, part, ch1, PL, C);
  if (ck.active) put_row(red, ck.lane, C, ck.cv, s2);
  fold_rows(red, part, ch2, PL, C);
  for (int c = tid; c < C; c += kT)
    *reinterpret_cast<float2*>(wsp + ((long long)blockIdx.x * C + c) * 2) = make_float2(ch1[c], ch2[c]);
}

// one thread per (image, group): A / m and Q / m from the chunk partials, chunk then channel order, in fp64
__global__ void __launch_bounds__(kT) gn_bwd_finalize_kernel(const float* __restrict__ wsp,
                                                             const float* __restrict__ gamma, float* __restrict__ aq,
                                                             int NG, int G, int Cg, int C, int K, float m) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= NG) return;
  const int n = e / G, g = e - n * G;
  double a = 0.0, q = 0.0;
  for (int k = 0; k < K; ++k)
    for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
      const float2 p = *reinterpret_cast<const float2*>(wsp + (((long long)n * K + k) * C + c) * 2);
      a += static_cast<double>(p.x) * gamma[c];
      q += static_cast<double>(p.y) * gamma[c];
    }
  aq[2 * (long long)e] = static_cast<float>(a / static_cast<double>(m));
  aq[2 * (long long)e + 1] = static_cast<float>(q / static_cast<double>(m));
}

template <bool RELU>
__global__ void __launch_bounds__(kT) gn_bwd_dx_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ aq, bf16_t* __restrict__ dx, int HW,
                                                       int C, int G, int Cg, int K) {
  const Chunk ck = chunk_of(HW, C, K);
  const int PL = kT / (C >> 3);
  if (!ck.active) return;
  uint4 rx[kVec], rd[kVec];
  load_chunk(x, ck, C, rx);
  load_chunk(dy, ck, C, rd);
  Lane8 L;
  int gi[8];
  lane_stats(mean, rstd, gamma, beta, ck, G, Cg, L, gi);
  float a[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float2 p = *reinterpret_cast<const float2*>(aq + 2 * ((long long)ck.n * G + gi[k]));
    a[k] = p.x;
    q[k] = p.y;
  }
#pragma unroll
  for (int i = 0; i < kVec; ++i)
    if (ck.lane + i * PL < ck.np) {
      float dz[8], xh[8];
      gn_dz8<RELU>(rx[i], rd[i], L, dz, xh);
      store_nt(dx + ck.off + (long long)i * PL * C, gn_dx8(dz, xh, L, a, q));
    }
}

// The partial rows [R, C, 2] in fp64 in a fixed order: a block owns 8 channels, each of its 32 row lanes adds rows
// lane, lane + 32, ... in row order, then one thread per channel adds the 32 lane sums in lane order.
__global__ void __launch_bounds__(kT) gn_param_finalize_kernel(const float* __restrict__ wsp,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               long long R, int C, int accumulate) {
  __shared__ double lb[32][8], lg[32][8];
  const int cl = threadIdx.x & 7, lane = threadIdx.x >> 3;
  const int c = blockIdx.x * 8 + cl;              // C % 8 == 0: c < C
  double sb = 0.0, sg = 0.0;
  for (long long r = lane; r < R; r += 32) {
    const float2 p = *reinterpret_cast<const float2*>(wsp + (r * C + c) * 2);
    sb += static_cast<double>(p.x);
    sg += static_cast<double>(p.y);
  }
  lb[lane][cl] = sb;
  lg[lane][cl] = sg;
  __syncthreads();
  if (lane) return;
  sb = sg = 0.0;
  for (int l = 0; l < 32; ++l) {
    sb += lb[l][cl];
    sg += lg[l][cl];
  }
  if (accumulate) {
    sb += static_cast<double>(dbeta[c]);
    sg += static_cast<double>(dgamma[c]);
  }
  dbeta[c] = static_cast<float>(sb);
  dgamma[c] = static_cast<float>(sg);
}

// ------------------------------------------------------------------------------------------------------ host
inline bool aligned(const void* p, uintptr_t a) { return p && (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline bool sizes_ok(int N, int H, int W, int C, int G) {
  if (N < 0 || H < 1 || W < 1 || C < 8 || C > kMaxC || (C & 7) || G < 1 || C % G) return false;
  const long long HW = (long long)H * W;
  return HW * C < (1ll << 31) && (long long)N * HW < (1ll << 31);
}

inline int chunk_pixels(int C) { return kVec * (kT / (C >> 3)); }
inline int chunks_of(int HW, int C) { return static_cast<int>(ceil_div(HW, chunk_pixels(C))); }
// backward statistics: adjacent chunks of an image per block (one partial row each), about 2048 blocks in all
inline int bwd_span(int N, int K) {
  const long long s = (long long)N * K / 2048;
  return s < 1 ? 1 : (s > K ? K : static_cast<int>(s));
}

// The strip of a resident block: the fewest groups that make whole vectors, doubled, tripled, ... while the strip
// stays within kWideCh channels, divides G and fits; lds == 0 when even the narrowest does not fit.
ResPlan res_plan(int HW, int C, int G, bool bwd) {
  ResPlan best = {0, 0, 0, 0, 0, 0};
  const int Cg = C / G;
  int s0 = 8;
  while (s0 > 1 && (s0 / 2 * Cg) % 8 == 0) s0 /= 2;
  for (int k = 1; s0 * k <= G; ++k) {
    if ((G / s0) % k) continue;
    ResPlan p;
    p.S = s0 * k;
    p.CH = p.S * Cg;
    if (k > 1 && p.CH > kWideCh) break;
    p.SV = p.CH / 8;
    p.PL = kT / p.SV;
    p.strips = G / p.S;
    const long long bytes = (long long)HW * p.CH * 2 * (bwd ? 2 : 1) +
                            4ll * (p.PL * p.CH + kT + (bwd ? 2 : 1) * p.CH + 2 * p.S);
    if (bytes > kLds) break;
    p.lds = static_cast<int>(bytes);
    best = p;
  }
  return best;
}

// 1 resident, 2 streaming, 0: path 1 was asked for and the strip does not fit.  The auto rule is read off
// profiles/group_norm.md: the resident kernels win where a strip is whole 128-byte lines per pixel (forward: and has
// at least 128 pixels, 14x14x1024 but not 7x7x2048) and, whatever the strip, where the tensor is at most 32 MiB and
// the single launch counts (batch 32 of 28x28x512 and smaller); streaming wins elsewhere, by up to 2.9x at the
// 16-byte strips of 56x56x256.
inline int resolve(int path, const ResPlan& pl, int N, int HW, int C, bool bwd) {
  if (path == 2) return 2;
  if (path == 1) return pl.lds ? 1 : 0;
  if (!pl.lds) return 2;
  if ((long long)N * HW * C * 2 <= (32ll << 20)) return 1;
  return pl.CH * 2 >= 128 && (bwd || HW >= 128) ? 1 : 2;
}

}  // namespace

// whether the resident design takes these sizes (backward: both strips staged)
MDTF_EXPORT int mdtf_gn_resident_fits(int H, int W, int C, int G, int backward) {
  if (!sizes_ok(1, H, W, C, G)) return 0;
  return res_plan(H * W, C, G, backward != 0).lds != 0;
}

// vectors (of 8 channels) per streaming chunk: a whole number of pixels
MDTF_EXPORT long long mdtf_gn_chunk(int C) {
  if (C < 8 || C > kMaxC || (C & 7)) return 0;
  return (long long)chunk_pixels(C) * (C >> 3);
}

// floats of workspace of mdtf_gn_fwd: streaming [N, chunks, G, 3]; resident none
MDTF_EXPORT long long mdtf_gn_fwd_ws(int N, int H, int W, int C, int G, int path) {
  if (!sizes_ok(N, H, W, C, G) || path < 0 || path > 2) return 0;
  if (resolve(path, res_plan(H * W, C, G, false), N, H * W, C, false) != 2) return 0;
  return (long long)N * chunks_of(H * W, C) * G * 3;
}

// floats of workspace of mdtf_gn_bwd: the parameter partials [N (* chunks), C, 2], streaming also A, Q [N, G, 2]
MDTF_EXPORT long long mdtf_gn_bwd_ws(int N, int H, int W, int C, int G, int path) {
  if (!sizes_ok(N, H, W, C, G) || path < 0 || path > 2) return 0;
  const int r = resolve(path, res_plan(H * W, C, G, true), N, H * W, C, true);
  if (r == 0) return 0;
  if (r == 1) return (long long)N * C * 2;
  const int K = chunks_of(H * W, C);
  return (long long)N * ceil_div(K, bwd_span(N, K)) * C * 2 + (long long)N * G * 2;
}

// y = act(group_norm(x)); mean, rstd [N, G] are stored for the backward.  x, y bf16 [N, H, W, C], 16-byte aligned.
MDTF_EXPORT int mdtf_gn_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                            float* ws, int N, int H, int W, int C, int G, float eps, int relu, int path,
                            hipStream_t st) {
  if (!sizes_ok(N, H, W, C, G) || path < 0 || path > 2 || !(eps >= 0.f)) return MDTF_EINVAL;
  if (!aligned(x, 16) || !aligned(y, 16) || !aligned(gamma, 4) || !aligned(beta, 4) || !aligned(mean, 4) ||
      !aligned(rstd, 4))
    return MDTF_EINVAL;
  const int HW = H * W, Cg = C / G;
  const ResPlan pl = res_plan(HW, C, G, false);
  const int r = resolve(path, pl, N, HW, C, false);
  if (r == 0 || (r == 2 && !aligned(ws, 4))) return MDTF_EINVAL;
  if (N == 0) return 0;
  const bf16_t* xp = static_cast<const bf16_t*>(x);
  bf16_t* yp = static_cast<bf16_t*>(y);
  if (r == 1) {
    const dim3 grid(static_cast<unsigned>((long long)N * pl.strips));
    if (relu)
      hipLaunchKernelGGL(gn_res_fwd_kernel<true>, grid, dim3(kT), pl.lds, st, xp, gamma, beta, yp, mean, rstd, HW, C,
                         G, Cg, pl, eps);
    else
      hipLaunchKernelGGL(gn_res_fwd_kernel<false>, grid, dim3(kT), pl.lds, st, xp, gamma, beta, yp, mean, rstd, HW, C,
                         G, Cg, pl, eps);
    MDTF_LAUNCH_CHECK();
    return 0;
  }
  const int K = chunks_of(HW, C);
  const dim3 grid(static_cast<unsigned>((long long)N * K));
  const float m = static_cast<float>(HW) * static_cast<float>(Cg);
  hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(kT), 0, st, xp, ws, HW, C, G, Cg, K);
  MDTF_LAUNCH_CHECK();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(static_cast<unsigned>(ceil_div((long long)N * G, kT))), dim3(kT), 0, st,
                     ws, mean, rstd, N * G, G, K, m, eps);
  MDTF_LAUNCH_CHECK();
  if (relu)
    hipLaunchKernelGGL(gn_apply_kernel<true>, grid, dim3(kT), 0, st, xp, gamma, beta, mean, rstd, yp, HW, C, G, Cg, K);
  else
    hipLaunchKernelGGL(gn_apply_kernel<false>, grid, dim3(kT), 0, st, xp, gamma, beta, mean, rstd, yp, HW, C, G, Cg,
                       K);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// dx, and dgamma / dbeta (fp32 [C]) = or += (accumulate) the parameter gradients, for the dy of mdtf_gn_fwd's y.
// mean, rstd: what the forward stored.  ws: mdtf_gn_bwd_ws floats, 8-byte aligned.
MDTF_EXPORT int mdtf_gn_bwd(const void* x, const void* dy, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, void* dx, float* dgamma, float* dbeta, float* ws, int N, int H, int W,
                            int C, int G, int relu, int accumulate, int path, hipStream_t st) {
  if (!sizes_ok(N, H, W, C, G) || path < 0 || path > 2) return MDTF_EINVAL;
  if (!aligned(x, 16) || !aligned(dy, 16) || !aligned(dx, 16) || !aligned(gamma, 4) || !aligned(beta, 4) ||
      !aligned(mean, 4) || !aligned(rstd, 4) || !aligned(dgamma, 4) || !aligned(dbeta, 4) || !aligned(ws, 8))
    return MDTF_EINVAL;
  const int HW = H * W, Cg = C / G;
  const ResPlan pl = res_plan(HW, C, G, true);
  const int r = resolve(path, pl, N, HW, C, true);
  if (r == 0) return MDTF_EINVAL;
  const bf16_t* xp = static_cast<const bf16_t*>(x);
  const bf16_t* dyp = static_cast<const bf16_t*>(dy);
  bf16_t* dxp = static_cast<bf16_t*>(dx);
  long long rows = N;
  if (N > 0 && r == 1) {
    const dim3 grid(static_cast<unsigned>((long long)N * pl.strips));
    if (relu)
      hipLaunchKernelGGL(gn_res_bwd_kernel<true>, grid, dim3(kT), pl.lds, st, xp, dyp, gamma, beta, mean, rstd, dxp,
                         ws, HW, C, G, Cg, pl);
    else
      hipLaunchKernelGGL(gn_res_bwd_kernel<false>, grid, dim3(kT), pl.lds, st, xp, dyp, gamma, beta, mean, rstd, dxp,
                         ws, HW, C, G, Cg, pl);
    MDTF_LAUNCH_CHECK();
  } else if (N > 0) {
    const int K = chunks_of(HW, C), span = bwd_span(N, K), K2 = static_cast<int>(ceil_div(K, span));
    rows = (long long)N * K2;
    float* aq = ws + rows * C * 2;
    const dim3 grid(static_cast<unsigned>((long long)N * K)), sgrid(static_cast<unsigned>(rows));
    const float m = static_cast<float>(HW) * static_cast<float>(Cg);
    if (relu)
      hipLaunchKernelGGL(gn_bwd_stats_kernel<true>, sgrid, dim3(kT), 0, st, xp, dyp, gamma, beta, mean, rstd, ws, HW,
                         C, G, Cg, K, span);
    else
      hipLaunchKernelGGL(gn_bwd_stats_kernel<false>, sgrid, dim3(kT), 0, st, xp, dyp, gamma, beta, mean, rstd, ws, HW,
                         C, G, Cg, K, span);
    MDTF_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(static_cast<unsigned>(ceil_div((long long)N * G, kT))), dim3(kT),
                       0, st, ws, gamma, aq, N * G, G, Cg, C, K2, m);
    MDTF_LAUNCH_CHECK();
    if (relu)
      hipLaunchKernelGGL(gn_bwd_dx_kernel<true>, grid, dim3(kT), 0, st, xp, dyp, gamma, beta, mean, rstd, aq, dxp, HW,
                         C, G, Cg, K);
    else
      hipLaunchKernelGGL(gn_bwd_dx_kernel<false>, grid, dim3(kT), 0, st, xp, dyp, gamma, beta, mean, rstd, aq, dxp, HW,
                         C, G, Cg, K);
    MDTF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gn_param_finalize_kernel, dim3(static_cast<unsigned>(C / 8)), dim3(kT), 0, st, ws, dgamma,
                     dbeta, rows, C, accumulate != 0);
  MDTF_LAUNCH_CHECK();
  return 0;
}
