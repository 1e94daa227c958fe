// Encoder-decoder (cross) multi-head attention with per-item source lengths: queries q [B*Sq, H] of one sequence
// attend to the keys / values kv [B*Sk, 2H] (k | v, heads contiguous inside each half) of another; batch item b sees
// keys k < kv_len[b] only.  Sq and Sk independent, each % 64 == 0; head dim 64 / 128 (gfx950, bf16 MFMA).
//
// The tiling is that of attention_flash.hip / attention_causal.hip (64-key K/V tiles by LDS-DMA, double-buffered; Q
// fragments in registers; S^T = K Q^T; P^T fed from registers as a B operand; V^T through ds_read_b64_tr_b16; helpers
// in attn_tile.h).  The source length is read once per block from the device buffer (one scalar load, b is
// block-uniform) and shapes all three main loops instead of being one more additive mask:
//   forward (workgroup = 64 or 128 queries at q0, wave = 16 or 32 queries): the key-tile loop runs to ceil(len / 64);
//     tiles wholly below len run the unmasked code, only the tile that len crosses pays the per-element k < len
//     compare (hidden elements: probability exactly 0, no exp, no hash); len == 0: no load, out = 0, lse = 0;
//   dK/dV (workgroup = 64 keys at k0, wave = 16 keys): a block with k0 >= len stores zeros with 16-B stores and
//     returns before any load; the block that len crosses compares per key column (a wave whose 16 keys are all
//     hidden skips the MFMAs, not the barriers) and stores zeros for its hidden rows; the others loop over all
//     32-query tiles;
//   dQ (workgroup = 64 queries at q0, wave = 16 queries): the key-tile loop runs to ceil(len / 64), the compare on
//     the crossing tile only; len == 0 stores dq = 0.
// The forward block is 64 queries (QT = 1: one 16-query tile per wave) at head dim 64 and at Sq == 64 (the decoder's
// usual case, where a 128-query block leaves two of its four waves without work), and 128 queries (QT = 2: each K
// fragment read from LDS feeds two MFMAs) at head dim 128 with Sq > 64: the measured winner of each
// (profiles/attention_cross.md, "Query block").  mdtf_attn_fwd_cross_qb takes the block size as an argument for
// that A/B.
// Dropout: the counter hash of attn_tile.h on element index (bh * Sq + q) * Sk + k (Sq == Sk: the keep bits of the
// self-attention kernels), the device step counter mixed in through step_seed.  lse is per query over the visible
// keys.  dq and dkv are fully written.  No atomics, no host read of the lengths, no allocation.
#include <type_traits>

#include "attn_tile.h"

namespace {

using Cross = std::true_type;    // tile crossed by the source length: per-element k < len compare
using Below = std::false_type;   // tile wholly below the source length: every element visible

__device__ __forceinline__ uint32_t drop_threshold(float p_drop) {
  return p_drop > 0.f ? (uint32_t)fminf(p_drop * 4294967296.f, 4294967295.f) : 0u;
}

// ================================================================================ forward
template <int D, int QT>
__global__ void __launch_bounds__(NT, 2) attn_fwd_cross(const bf16_t* __restrict__ qin, const bf16_t* __restrict__ kv,
                                                         const float* __restrict__ mask,
                                                         const int* __restrict__ kv_len, bf16_t* __restrict__ out,
                                                         float* __restrict__ lse_out, int B, int Sq, int Sk, int nh,
                                                         float scale, float p_drop, uint32_t seed,
                                                         const long long* __restrict__ seed_off) {
  constexpr int DH = D / 64;                     // 64-column halves of a head
  constexpr int TILE = 64 * 128 * DH;            // one K or V tile image (64 keys)
  seed = step_seed(seed, seed_off);
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * TILE];   // [buf][K | V]
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh;
  const int q0 = blockIdx.y * (64 * QT);
  const int H = nh * D, ld = 2 * H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const long long rowb = (long long)b * Sk * ld, qrow = (long long)b * Sq * H;
  const int tbytes = (int)((long long)B * Sk * ld * 2);
  const int len = kv_length(kv_len, b, Sk);
  const int nfull = len >> 6, nkt = (len + 63) >> 6;   // tiles wholly visible / tiles that hold a visible key
  const int qw0 = q0 + 16 * QT * wave;           // this wave's queries: qw0 .. qw0 + 16 QT - 1
  // the last 128-query block of an Sq % 128 == 64 sequence has 64 queries: the waves past Sq compute and store nothing
  const bool live = qw0 < Sq;

  if (nkt == 0) {                                // empty item: no load; out = 0, lse finite (the backward never reads it)
    if (!live) return;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int q = qw0 + 16 * qt + li;
      if (g == 0) lse_out[(long long)bh * Sq + q] = 0.f;
      bf16_t* o = out + qrow + (long long)q * H + h * D;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) *reinterpret_cast<uint2*>(o + dt * 16 + 4 * g) = make_uint2(0u, 0u);
    }
    return;
  }

  auto load_kv = [&](int kb, int buf) {
    char* Ki = smem + buf * 2 * TILE;
    char* Vi = Ki + TILE;
#pragma unroll
    for (int hh = 0; hh < DH; ++hh) {
      load_tile<SwzA, 64>(kv, tbytes, rowb + (long long)kb * 64 * ld, ld, h * D + 64 * hh, Ki + hh * 8192, wave, lane);
      load_tile<SwzV, 64>(kv, tbytes, rowb + (long long)kb * 64 * ld, ld, H + h * D + 64 * hh, Vi + hh * 8192, wave,
                          lane);
    }
  };
  load_kv(0, 0);
  bf16x8_t qf[QT][D / 32];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds) {
      const int q = min(qw0 + 16 * qt + li, Sq - 1);
      qf[qt][ds] = gfrag(qin + qrow + (long long)q * H + h * D + 32 * ds + 8 * g);
    }
  const uint32_t thr = drop_threshold(p_drop);
  const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  float m[QT], l[QT];
  float4v oacc[D / 16][QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m[qt] = -3.0e38f;
    l[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) oacc[dt][qt] = float4v{0.f, 0.f, 0.f, 0.f};
  }

  // one 64-key tile against this wave's 16 QT queries
  auto tile = [&](int kb, auto cross) {
    constexpr bool CROSS = decltype(cross)::value;
    const char* Ki = smem + (kb & 1) * 2 * TILE;
    const char* Vi = Ki + TILE;
    float4v sacc[4][QT];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) sacc[kt][qt] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bf16x8_t kf = row_frag<SwzA>(Ki + (ds >> 1) * 8192, kt * 16, 4 * (ds & 1), lane);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) sacc[kt][qt] = mfma(kf, qf[qt][ds], sacc[kt][qt]);
      }
    float mk[4][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float4 m4 = mask4(mask, (long long)b * Sk + kb * 64 + kt * 16 + 4 * g);
      mk[kt][0] = m4.x;
      mk[kt][1] = m4.y;
      mk[kt][2] = m4.z;
      mk[kt][3] = m4.w;
    }
    bf16x8_t pf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int q = qw0 + 16 * qt + li;
      // A hidden element (k >= len) never enters the running max and contributes exactly 0 to the row sum and to P
      // (set, not left to exp underflow).  The crossing tile holds key 64 * nfull < len, visible to every row, so mx
      // is finite there too; were it not, mn = m, corr = 1, sum = 0 would leave m and l unchanged.
      float mx = -3.0e38f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = sacc[kt][qt][i] * scale + mk[kt][i];
          sacc[kt][qt][i] = s;
          if (!CROSS || kb * 64 + kt * 16 + 4 * g + i < len) mx = fmaxf(mx, s);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[qt], mx);
      const float corr = __expf(m[qt] - mn);
      m[qt] = mn;
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = kb * 64 + kt * 16 + 4 * g + i;
          if (CROSS && k >= len) {
            sacc[kt][qt][i] = 0.f;                 // hidden: exactly 0 in the row sum and in P; no exp, no hash
          } else {
            const float e = __expf(sacc[kt][qt][i] - mn);
            sum += e;
            sacc[kt][qt][i] = (thr && !keep_elem_x(seed, bh, Sq, Sk, q, k, thr)) ? 0.f : e * inv_keep;
          }
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l[qt] = l[qt] * corr + sum;
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) oacc[dt][qt] *= corr;
      pf[qt][0] = pack_acc(sacc[0][qt], sacc[1][qt]);
      pf[qt][1] = pack_acc(sacc[2][qt], sacc[3][qt]);
    }
    // O^T[d][q] += V^T P^T
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const bf16x8_t vf = trp_frag(Vi + (dt >> 2) * 8192, 32 * ks, (dt & 3) * 16, lane);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) oacc[dt][qt] = mfma(vf, pf[qt][ks], oacc[dt][qt]);
      }
  };

  auto next = [&](int kb) {
    wait_vmcnt<0>();
    __syncthreads();                                   // tile kb landed; tile kb-1's buffer is free
    if (kb + 1 < nkt) load_kv(kb + 1, (kb + 1) & 1);
  };
  // One loop body per variant, not a branch inside one loop (attention_causal.hip: the invariants hoisted for both
  // variants together do not fit the register file at head dim 128).
  for (int kb = 0; kb < nfull; ++kb) {                 // wholly visible: the unmasked code
    next(kb);
    if (live) tile(kb, Below{});
  }
  if (nfull < nkt) {                                   // the tile that len crosses
    next(nfull);
    if (live) tile(nfull, Cross{});
  }
  if (!live) return;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = qw0 + 16 * qt + li;
    const float inv = 1.f / l[qt];
    if (g == 0) lse_out[(long long)bh * Sq + q] = m[qt] + __logf(l[qt]);
    bf16_t* o = out + qrow + (long long)q * H + h * D;
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const float4v v = oacc[dt][qt];
      *reinterpret_cast<uint2*>(o + dt * 16 + 4 * g) =
          make_uint2(pack_bf2(v[0] * inv, v[1] * inv), pack_bf2(v[2] * inv, v[3] * inv));
    }
  }
}

// ================================================================================ backward
// dK, dV for 64 keys of one (b, h); wave = 16 keys; loop over all 32-query tiles unless the keys are hidden
template <int D>
__global__ void __launch_bounds__(NT, 2) attn_bwd_dkv_cross(const bf16_t* __restrict__ qin,
                                                             const bf16_t* __restrict__ kv,
                                                             const float* __restrict__ mask,
                                                             const int* __restrict__ kv_len,
                                                             const bf16_t* __restrict__ dout,
                                                             const float* __restrict__ lse,
                                                             const float* __restrict__ dqv, bf16_t* __restrict__ dkv,
                                                             int B, int Sq, int Sk, int nh, float scale, float p_drop,
                                                             uint32_t seed, const long long* __restrict__ seed_off) {
  constexpr int DH = D / 64;
  constexpr int IMG = 32 * 128;                  // [32 queries][64 d]
  constexpr int BUF = 4 * DH * IMG;              // Q_A, dO_A, Q_V, dO_V (each DH halves)
  seed = step_seed(seed, seed_off);
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh;
  const int k0 = blockIdx.y * 64;
  const int H = nh * D, ld = 2 * H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const long long rowb = (long long)b * Sk * ld, qrow = (long long)b * Sq * H;
  const int qbytes = (int)((long long)B * Sq * H * 2);
  const int nqt = Sq / 32;
  const int len = kv_length(kv_len, b, Sk);

  if (k0 >= len) {                               // every key hidden: dK = dV = 0, nothing loaded
    bf16_t* p = dkv + rowb + (long long)k0 * ld + h * D;
    zero_rows<D>(p, 64, ld, threadIdx.x);
    zero_rows<D>(p + H, 64, ld, threadIdx.x);
    return;
  }
  const bool crossing = len < k0 + 64;           // block-uniform: some of the 64 keys are hidden
  const bool wave_hidden = k0 + 16 * wave >= len;   // wave-uniform: all 16 keys of this wave are hidden

  auto load_q = [&](int qb, int buf) {
    char* base = smem + buf * BUF;
#pragma unroll
    for (int hh = 0; hh < DH; ++hh) {
      const long long r = qrow + (long long)qb * 32 * H;
      load_tile<SwzA, 32>(qin, qbytes, r, H, h * D + 64 * hh, base + (0 * DH + hh) * IMG, wave, lane);
      load_tile<SwzA, 32>(dout, qbytes, r, H, h * D + 64 * hh, base + (1 * DH + hh) * IMG, wave, lane);
      load_tile<SwzV, 32>(qin, qbytes, r, H, h * D + 64 * hh, base + (2 * DH + hh) * IMG, wave, lane);
      load_tile<SwzV, 32>(dout, qbytes, r, H, h * D + 64 * hh, base + (3 * DH + hh) * IMG, wave, lane);
    }
  };
  load_q(0, 0);
  const int key = k0 + 16 * wave + li;           // this lane's key column (< Sk)
  bf16x8_t kf[D / 32], vf[D / 32];
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    kf[ds] = gfrag(kv + rowb + (long long)key * ld + h * D + 32 * ds + 8 * g);
    vf[ds] = gfrag(kv + rowb + (long long)key * ld + H + h * D + 32 * ds + 8 * g);
  }
  const float mkey = mask ? mask[(long long)b * Sk + key] : 0.f;
  const uint32_t thr = drop_threshold(p_drop);
  const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  float4v vacc[D / 16], kacc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) vacc[dt] = kacc[dt] = float4v{0.f, 0.f, 0.f, 0.f};

  // one 32-query tile against this wave's 16 keys
  auto tile = [&](int qb, auto cross) {
    constexpr bool CROSS = decltype(cross)::value;
    const char* base = smem + (qb & 1) * BUF;
    const char* QA = base;
    const char* OA = base + DH * IMG;
    const char* QV = base + 2 * DH * IMG;
    const char* OV = base + 3 * DH * IMG;
    // S[q][k], dP[q][k] for 32 queries x this wave's 16 keys
    float4v sacc[2], pacc[2];
    sacc[0] = sacc[1] = pacc[0] = pacc[1] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const bf16x8_t qa = row_frag<SwzA>(QA + (ds >> 1) * IMG, 16 * qt, 4 * (ds & 1), lane);
        const bf16x8_t oa = row_frag<SwzA>(OA + (ds >> 1) * IMG, 16 * qt, 4 * (ds & 1), lane);
        sacc[qt] = mfma(qa, kf[ds], sacc[qt]);
        pacc[qt] = mfma(oa, vf[ds], pacc[qt]);
      }
    // lane holds queries 16qt + 4g + i of key `key`
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int q = qb * 32 + 16 * qt + 4 * g + i;
        if (CROSS && key >= len) {
          sacc[qt][i] = 0.f;                                  // hidden: P = dS = 0, no exp, no hash
          pacc[qt][i] = 0.f;
          continue;
        }
        const float p = __expf(sacc[qt][i] * scale + mkey - lse[(long long)bh * Sq + q]);
        float dp = pacc[qt][i], pk = p;
        if (thr) {
          const bool keep = keep_elem_x(seed, bh, Sq, Sk, q, key, thr);
          pk = keep ? p * inv_keep : 0.f;
          dp = keep ? dp * inv_keep : 0.f;
        }
        sacc[qt][i] = pk;                                     // P_drop
        pacc[qt][i] = p * (dp - dqv[(long long)bh * Sq + q]); // dS
      }
    const bf16x8_t pb = pack_acc(sacc[0], sacc[1]);
    const bf16x8_t sb = pack_acc(pacc[0], pacc[1]);
    // dV^T[d][k] += dO^T P_drop, dK^T[d][k] += Q^T dS  (k-dim = the 32 queries, permuted order)
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
      const bf16x8_t of = trp_frag(OV + (dt >> 2) * IMG, 0, (dt & 3) * 16, lane);
      const bf16x8_t qf = trp_frag(QV + (dt >> 2) * IMG, 0, (dt & 3) * 16, lane);
      vacc[dt] = mfma(of, pb, vacc[dt]);
      kacc[dt] = mfma(qf, sb, kacc[dt]);
    }
  };

  auto next = [&](int qb) {
    wait_vmcnt<0>();
    __syncthreads();
    if (qb + 1 < nqt) load_q(qb + 1, (qb + 1) & 1);
  };
  if (crossing) {                                      // the compare in the block that len crosses only
    for (int qb = 0; qb < nqt; ++qb) {
      next(qb);
      if (!wave_hidden) tile(qb, Cross{});
    }
  } else {
    for (int qb = 0; qb < nqt; ++qb) {
      next(qb);
      tile(qb, Below{});
    }
  }
  // lane holds rows d = 16dt + 4g .. +3 of key column `key`; a hidden key's rows are stored as zeros
  const bool hidden = key >= len;
  bf16_t* rowp = dkv + rowb + (long long)key * ld + h * D;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const float4v kk = kacc[dt], vv = vacc[dt];
    const uint2 dk2 = make_uint2(pack_bf2(kk[0] * scale, kk[1] * scale), pack_bf2(kk[2] * scale, kk[3] * scale));
    const uint2 dv2 = make_uint2(pack_bf2(vv[0], vv[1]), pack_bf2(vv[2], vv[3]));
    *reinterpret_cast<uint2*>(rowp + dt * 16 + 4 * g) = hidden ? make_uint2(0u, 0u) : dk2;
    *reinterpret_cast<uint2*>(rowp + H + dt * 16 + 4 * g) = hidden ? make_uint2(0u, 0u) : dv2;
  }
}

// dQ for 64 queries of one (b, h); wave = 16 queries; loop over the 64-key tiles that hold a visible key
template <int D>
__global__ void __launch_bounds__(NT, 2) attn_bwd_dq_cross(const bf16_t* __restrict__ qin,
                                                            const bf16_t* __restrict__ kv,
                                                            const float* __restrict__ mask,
                                                            const int* __restrict__ kv_len,
                                                            const bf16_t* __restrict__ dout,
                                                            const float* __restrict__ lse,
                                                            const float* __restrict__ dqv, bf16_t* __restrict__ dq,
                                                            int B, int Sq, int Sk, int nh, float scale, float p_drop,
                                                            uint32_t seed, const long long* __restrict__ seed_off) {
  constexpr int DH = D / 64;
  constexpr int IMG = 64 * 128;                  // [64 keys][64 d]
  constexpr int BUF = 3 * DH * IMG;              // K_A, V_A, K_V
  seed = step_seed(seed, seed_off);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int bh = blockIdx.x, b = bh / nh, h = bh - b * nh;
  const int q0 = blockIdx.y * 64;
  const int H = nh * D, ld = 2 * H;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const long long rowb = (long long)b * Sk * ld, qrow = (long long)b * Sq * H;
  const int tbytes = (int)((long long)B * Sk * ld * 2);
  const int len = kv_length(kv_len, b, Sk);
  const int nfull = len >> 6, nkt = (len + 63) >> 6;

  if (nkt == 0) {                                // empty item: dq = 0, nothing loaded
    zero_rows<D>(dq + qrow + (long long)q0 * H + h * D, 64, H, threadIdx.x);
    return;
  }

  auto load_k = [&](int kb, int buf) {
    char* base = smem + buf * BUF;
    const long long krow = rowb + (long long)kb * 64 * ld;
#pragma unroll
    for (int hh = 0; hh < DH; ++hh) {
      load_tile<SwzA, 64>(kv, tbytes, krow, ld, h * D + 64 * hh, base + (0 * DH + hh) * IMG, wave, lane);
      load_tile<SwzA, 64>(kv, tbytes, krow, ld, H + h * D + 64 * hh, base + (1 * DH + hh) * IMG, wave, lane);
      load_tile<SwzV, 64>(kv, tbytes, krow, ld, h * D + 64 * hh, base + (2 * DH + hh) * IMG, wave, lane);
    }
  };
  load_k(0, 0);
  const int q = q0 + 16 * wave + li;             // this lane's query column
  bf16x8_t qf[D / 32], of[D / 32];
#pragma unroll
  for (int ds = 0; ds < D / 32; ++ds) {
    qf[ds] = gfrag(qin + qrow + (long long)q * H + h * D + 32 * ds + 8 * g);
    of[ds] = gfrag(dout + qrow + (long long)q * H + h * D + 32 * ds + 8 * g);
  }
  const float lq = lse[(long long)bh * Sq + q], Dq = dqv[(long long)bh * Sq + q];
  const uint32_t thr = drop_threshold(p_drop);
  const float inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  float4v qacc[D / 16];
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) qacc[dt] = float4v{0.f, 0.f, 0.f, 0.f};

  // one 64-key tile against this wave's 16 queries
  auto tile = [&](int kb, auto cross) {
    constexpr bool CROSS = decltype(cross)::value;
    const char* base = smem + (kb & 1) * BUF;
    const char* KA = base;
    const char* VA = base + DH * IMG;
    const char* KV = base + 2 * DH * IMG;
    // S^T[k][q], dP^T[k][q] for 64 keys x this wave's 16 queries
    float4v sacc[4], pacc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) sacc[kt] = pacc[kt] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ds = 0; ds < D / 32; ++ds)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bf16x8_t ka = row_frag<SwzA>(KA + (ds >> 1) * IMG, 16 * kt, 4 * (ds & 1), lane);
        const bf16x8_t va = row_frag<SwzA>(VA + (ds >> 1) * IMG, 16 * kt, 4 * (ds & 1), lane);
        sacc[kt] = mfma(ka, qf[ds], sacc[kt]);
        pacc[kt] = mfma(va, of[ds], pacc[kt]);
      }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float4 m4 = mask4(mask, (long long)b * Sk + kb * 64 + kt * 16 + 4 * g);
      const float mk[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = kb * 64 + kt * 16 + 4 * g + i;
        if (CROSS && k >= len) {
          sacc[kt][i] = 0.f;                                     // hidden: dS = 0, no exp, no hash
          continue;
        }
        const float p = __expf(sacc[kt][i] * scale + mk[i] - lq);
        float dp = pacc[kt][i];
        if (thr) dp = keep_elem_x(seed, bh, Sq, Sk, q, k, thr) ? dp * inv_keep : 0.f;
        sacc[kt][i] = p * (dp - Dq);                           // dS^T
      }
    }
    // dQ^T[d][q] += K^T dS^T  (k-dim = keys, 2 steps of 32, permuted order)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8_t sb = pack_acc(sacc[2 * ks], sacc[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < D / 16; ++dt) {
        const bf16x8_t kt_ = trp_frag(KV + (dt >> 2) * IMG, 32 * ks, (dt & 3) * 16, lane);
        qacc[dt] = mfma(kt_, sb, qacc[dt]);
      }
    }
  };

  auto next = [&](int kb) {
    wait_vmcnt<0>();
    __syncthreads();
    if (kb + 1 < nkt) load_k(kb + 1, (kb + 1) & 1);
  };
  for (int kb = 0; kb < nfull; ++kb) {                 // wholly visible: the unmasked code
    next(kb);
    tile(kb, Below{});
  }
  if (nfull < nkt) {                                   // the compare on the crossing tile only
    next(nfull);
    tile(nfull, Cross{});
  }
  bf16_t* rowp = dq + qrow + (long long)q * H + h * D;
#pragma unroll
  for (int dt = 0; dt < D / 16; ++dt) {
    const float4v v = qacc[dt];
    *reinterpret_cast<uint2*>(rowp + dt * 16 + 4 * g) =
        make_uint2(pack_bf2(v[0] * scale, v[1] * scale), pack_bf2(v[2] * scale, v[3] * scale));
  }
}

// Sq, Sk % 64 == 0, head dim 64 / 128; 32-bit byte offsets into q and kv (the LDS-DMA descriptors) and a 32-bit
// dropout element index
bool shape_ok(int B, int Sq, int Sk, int nh, int dh) {
  if (B <= 0 || nh <= 0 || Sq % 64 || Sq < 64 || Sk % 64 || Sk < 64 || (dh != 64 && dh != 128)) return false;
  const long long H = (long long)nh * dh, Bl = B;
  return Bl * Sq * H * 2 <= 0x7fffffffLL && Bl * Sk * 2 * H * 2 <= 0x7fffffffLL && Bl * nh * Sq * Sk <= 0xffffffffLL;
}

template <int D, int QT>
void fwd_kernel(const dim3& grid, hipStream_t st, const void* q, const void* kv, const float* mask, const int* kv_len,
                void* out, float* lse, int B, int Sq, int Sk, int nh, float scale, float p_drop, unsigned seed,
                const long long* seed_off) {
  hipLaunchKernelGGL((attn_fwd_cross<D, QT>), grid, dim3(NT), 0, st, (const bf16_t*)q, (const bf16_t*)kv, mask, kv_len,
                     (bf16_t*)out, lse, B, Sq, Sk, nh, scale, p_drop, (uint32_t)seed, seed_off);
}

// qb: queries per forward block, 64 or 128; 0 = the rule (128 at head dim 128 with Sq > 64, else 64)
int launch_fwd(const void* q, const void* kv, const float* mask, const int* kv_len, void* out, float* lse, int B,
               int Sq, int Sk, int nh, int dh, float scale, float p_drop, unsigned seed, const long long* seed_off,
               int qb, hipStream_t st) {
  if (!shape_ok(B, Sq, Sk, nh, dh) || (qb != 0 && qb != 64 && qb != 128)) return MDTF_EUNSUPPORTED;
  if (qb == 0) qb = (dh == 128 && Sq > 64) ? 128 : 64;
  const dim3 grid(B * nh, (Sq + qb - 1) / qb);
  if (dh == 64 && qb == 64)
    fwd_kernel<64, 1>(grid, st, q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  else if (dh == 64)
    fwd_kernel<64, 2>(grid, st, q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  else if (qb == 64)
    fwd_kernel<128, 1>(grid, st, q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  else
    fwd_kernel<128, 2>(grid, st, q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  MDTF_LAUNCH_CHECK();
  return 0;
}

template <int D>
void bwd_kernels(hipStream_t st, const void* q, const void* kv, const float* mask, const int* kv_len, const void* dout,
                 const float* lse, const float* ws, void* dq, void* dkv, int B, int Sq, int Sk, int nh, float scale,
                 float p_drop, unsigned seed, const long long* seed_off) {
  hipLaunchKernelGGL(attn_bwd_dkv_cross<D>, dim3(B * nh, Sk / 64), dim3(NT), 0, st, (const bf16_t*)q,
                     (const bf16_t*)kv, mask, kv_len, (const bf16_t*)dout, lse, ws, (bf16_t*)dkv, B, Sq, Sk, nh, scale,
                     p_drop, (uint32_t)seed, seed_off);
  hipLaunchKernelGGL(attn_bwd_dq_cross<D>, dim3(B * nh, Sq / 64), dim3(NT), 2 * 3 * (D / 64) * 64 * 128, st,
                     (const bf16_t*)q, (const bf16_t*)kv, mask, kv_len, (const bf16_t*)dout, lse, ws, (bf16_t*)dq, B,
                     Sq, Sk, nh, scale, p_drop, (uint32_t)seed, seed_off);
}

}  // namespace

// out[B*Sq, H] = attention(q[B*Sq, H], kv[B*Sk, 2H]) over the keys k < kv_len[b] (kv_len: device int32 [B] or null =
// every key) for Sq, Sk % 64 == 0, head dim 64 / 128; lse [B*nh, Sq] (fp32) over the visible keys; mask: additive
// [B, Sk] key mask or null
MDTF_EXPORT int mdtf_attn_fwd_cross(const void* q, const void* kv, const float* mask, const int* kv_len, void* out,
                                    float* lse, int B, int Sq, int Sk, int nh, int dh, float scale, float p_drop,
                                    unsigned seed, const long long* seed_off, hipStream_t st) {
  return launch_fwd(q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, dh, scale, p_drop, seed, seed_off, 0, st);
}

// dq[B*Sq, H] and dkv[B*Sk, 2H] (every element written) from dout[B*Sq, H]; ws: fp32 [B*nh*Sq] (Dq = rowsum(dO*O))
MDTF_EXPORT int mdtf_attn_bwd_cross(const void* q, const void* kv, const float* mask, const int* kv_len,
                                    const void* out, const void* dout, const float* lse, void* dq, void* dkv,
                                    float* ws, int B, int Sq, int Sk, int nh, int dh, float scale, float p_drop,
                                    unsigned seed, const long long* seed_off, hipStream_t st) {
  if (!shape_ok(B, Sq, Sk, nh, dh)) return MDTF_EUNSUPPORTED;
  const long long rows = (long long)B * Sq * nh;
  hipLaunchKernelGGL(attn_bwd_pre, dim3((unsigned)ceil_div(rows, 32LL)), dim3(256), 0, st, (const bf16_t*)out,
                     (const bf16_t*)dout, ws, B, Sq, nh, dh);
  if (dh == 64)
    bwd_kernels<64>(st, q, kv, mask, kv_len, dout, lse, ws, dq, dkv, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  else
    bwd_kernels<128>(st, q, kv, mask, kv_len, dout, lse, ws, dq, dkv, B, Sq, Sk, nh, scale, p_drop, seed, seed_off);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// The forward with the queries per block (64 / 128) as an argument, for the A/B of bench/attn_cross_probe.py only:
// no state, nothing the Python package registers.
MDTF_EXPORT int mdtf_attn_fwd_cross_qb(const void* q, const void* kv, const float* mask, const int* kv_len, void* out,
                                       float* lse, int B, int Sq, int Sk, int nh, int dh, float scale, float p_drop,
                                       unsigned seed, const long long* seed_off, int qb, hipStream_t st) {
  return launch_fwd(q, kv, mask, kv_len, out, lse, B, Sq, Sk, nh, dh, scale, p_drop, seed, seed_off, qb ? qb : -1, st);
}
