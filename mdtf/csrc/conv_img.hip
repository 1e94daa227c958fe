// Image-resident 3x3 convolution for C -> C channels at stride 1, pad 1 (the conv2 of ResNet stages 2 and 3:
// 28 x 28 x 128 and 14 x 14 x 256; forward and data gradient).
//
// Why: the implicit GEMM (conv_fd_v2) treats each of the 9 taps as new K, so every input pixel travels L2 -> LDS
// 9 times.  At batch 256 that is, per call,
//   14 x 14 x 256: 196 tiles x 36 K-steps x 64 KiB = 462 MB (2.36 MB per active CU, 196 of 256 CUs busy),
//   28 x 28 x 128: 1568 tiles x 18 K-steps x 32 KiB = 925 MB,
// against 52 MB / 103 MB of activations and at most 1.2 MB of filter that the conv has to touch.  conv_rows.hip
// removed the same redundancy for stage 1 by keeping the whole filter in LDS; at 128 / 256 channels the filter is
// 288 KiB / 1.15 MiB and does not fit.  Here the roles are swapped: the input is resident, the filter streams.
//   * A 512-thread block owns 14 output rows of one image: the whole 14 x 14 image, or one of the two bands of a
//     28 x 28 image (with the halo row it shares with the other band).  Grid = N or 2N blocks of equal work, no
//     cross-block synchronisation.
//   * Its input is staged in LDS once by LDS-DMA (zero fill outside the image through the buffer descriptor): per
//     64-channel plane, rows of W + 2 pixels (zero halo columns) of 128 B, 16-B chunk c of pixel px at slot
//     c ^ (px & 6) as in conv3_rows.  14 x 14 x 256 keeps no halo rows (112 KiB; the two tap rows that fall outside
//     the image are skipped, wave-uniform); a 28 x 28 x 128 band keeps 16 rows (120 KiB).
//   * The filter streams through a ring of 16-KiB LDS-DMA stages (3 at 112 KiB, 2 at 120 KiB) in MFMA fragment
//     order, one counted vmcnt wait and one barrier per stage; all 9 taps x C / 64 planes read the staged input.
//   * Wave (pg, cg) computes 7 pixel fragments (16 pixels of one row) x 64 output channels: 28 accumulator tiles.
// Traffic per block: 98 KiB + 1.15 MiB filter (328 MB per call at batch 256, 1.28 MB per CU) at 14 x 14 x 256;
// 120 KiB + 288 KiB (210 MB per call) at 28 x 28 x 128.
// Epilogues: plain store, forward BN statistics (sum y, sum y^2 of the fp32 accumulators), or the BN-backward
// statistics of the gradient it completes (sum g*mask, sum g*mask*x), as conv3_rows.  Selected inside
// mdtf_conv_fwd_v2 / mdtf_conv_dgrad_v2 (conv_igemm.hip); MDTF_CONV_IMG chooses the (shape, pass) set.
// Replaces the cuDNN conv2d the reference reaches through tf.nn.conv2d (distribute_tools.py:76,88) and its
// autodiff backward (distribute_tower.py:27) for these shapes; SURVEY §2.5 K1.
#include <stdlib.h>

#include <atomic>

#include "conv_ws_kernel.inc"

using namespace mdtf;
using namespace mdtf::ws;

namespace {
constexpr int kBand = 14;               // output rows per block
constexpr int kStageBytes = 16 * 1024;  // one filter ring stage: 16 MFMA fragments of 1 KiB
constexpr int kLdsBytes = 160 * 1024;

// Σ over lanes of a 16-lane DPP row with the lane-bit-0 parity kept: lanes 14 / 15 end with the sums of the
// row's even / odd lanes (three row_shr adds, zero fill past the row start)
__device__ __forceinline__ float row_sum8_pairs(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
  return v;
}
__device__ __forceinline__ float row_sum16_all(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
  return row_sum8_pairs(v);
}

template <int WI, int C>
struct ImgGeom {
  static constexpr bool FULL = WI == kBand;             // the band is the whole image: no halo rows staged
  static constexpr int WP = WI + 2;                     // staged pixels per row (zero halo both sides)
  static constexpr int SR = FULL ? kBand : kBand + 2;   // staged rows
  static constexpr int R0 = FULL ? 0 : -1;              // first staged row, relative to the band's first output row
  static constexpr int pitch = WP * 128;                // bytes per staged row of one 64-channel plane
  static constexpr int plane = SR * pitch;
  static constexpr int NP = C / 64;                     // planes = 64-channel groups of the output too
  static constexpr int act = NP * plane;
  static constexpr int S = (kLdsBytes - act) / kStageBytes;    // ring stages
  static constexpr int KSI = C / 32;                    // k-steps per tap
  static constexpr int KPS = kStageBytes / (C * 64);    // k-steps per ring stage (x C output channels x 64 B)
  static constexpr int SPK = 3 * KSI / KPS;             // stages per filter row
  static constexpr int NST = 3 * SPK;
  static constexpr int TPW = (WI + 15) / 16;            // pixel fragments per output row
  static constexpr int PG = 8 / NP;                     // waves that share a channel group
  static constexpr int FPW = kBand * TPW / PG;          // pixel fragments per wave
  static constexpr int QT = NP * SR * WP * 8;           // staged 16-B chunks
  static_assert(C % 64 == 0 && 8 % NP == 0 && KPS >= 1 && KPS * NP * 4 == 16, "a stage is 16 fragments");
  static_assert(S >= 2 && SPK % S == 0, "ring slots are compile-time inside a filter row");
  static_assert(kBand * TPW % PG == 0 && QT % 512 == 0, "even split over the waves");
  static_assert(QT / 512 + 2 * (S - 1) < 64, "vmcnt range");
};

// EPI: 0 plain, 1 forward statistics, 3 BN-backward statistics (Epi<> of conv_ws_kernel.inc; no accumulate).
// WI: image width; C: channels in = out.  H = rows of the image, a multiple of 14 (14 when WI == 14).
// wmode 0: wgt = Wt[co][(kh, kw, ci)]; wmode 1: wgt = W HWIO used flipped (the stride-1 data gradient, src = DY).
template <int EPI, int WI, int C>
__global__ void __launch_bounds__(512, 1) conv3_img(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wgt,
                                                     bf16_t* __restrict__ out, int H, int wmode, int nbytes,
                                                     float* __restrict__ ps0, float* __restrict__ ps1, int slots,
                                                     const bf16_t* __restrict__ bx, const uint8_t* __restrict__ bmask) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  using E = Epi<EPI>;
  using G = ImgGeom<WI, C>;
  constexpr int S = G::S, KPS = G::KPS, FPW = G::FPW, NP = G::NP;
  char* ring = lds + G::act;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int cg = wave % NP, pg = wave / NP;
  const int bpi = H / kBand;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int n = bid / bpi, oh0 = (bid - n * bpi) * kBand;

  // ---- the band's input -> LDS: chunk q = (plane, staged row r, pixel px, slot pos) holds channel chunk
  // pos ^ (px & 6) of input pixel (oh0 + R0 + r, px - 1), zero outside the image
  const i32x4_t ra = buffer_rsrc(src, nbytes);
#pragma unroll
  for (int t = 0; t < G::QT / 512; ++t) {
    const int q = (t * 8 + wave) * 64 + lane;
    const int pos = q & 7, pq = q >> 3, px = pq % G::WP, rq = pq / G::WP, r = rq % G::SR, pl = rq / G::SR;
    const int ih = oh0 + G::R0 + r, iw = px - 1;
    const bool ok = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)WI;
    const unsigned vo = ok ? (unsigned)((((n * H + ih) * WI + iw) * C + pl * 64 + 8 * (pos ^ (px & 6))) * 2) : kOOB;
    dma16_asm(ra, lds + (t * 8 + wave) * 1024, vo);
  }

  // ---- filter stream: stage s = k-steps s KPS .. + KPS - 1 (k-step ks: tap ks / KSI, channels 32 (ks % KSI) ..)
  // of every output channel; fragment fi = (q NP + cg) 4 + i of a stage, lane l: output channel 64 cg +
  // chan_of(i, l & 15), k = 32 ks + 8 (l >> 4).  Wave w fetches fragments w and w + 8.
  const i32x4_t rw = buffer_rsrc(wgt, 9 * C * C * 2);
  unsigned wl[2];
#pragma unroll
  for (int f2 = 0; f2 < 2; ++f2) {
    const int fi = wave + 8 * f2;
    const int co = ((fi >> 2) % NP) * 64 + chan_of(fi & 3, li);
    wl[f2] = (unsigned)((wmode == 0 ? co * 9 * C : co * C) + 8 * g) * 2u;
  }
  // byte offset of k-step ks = (tap, c32): wmode 0: 64 ks; wmode 1: ((8 - tap) C C + 32 c32) 2 = 64 ks + w1a - tap w1b
  const int w1a = wmode == 0 ? 0 : 16 * C * C, w1b = wmode == 0 ? 0 : 2 * C * C + 64 * G::KSI;
  auto stage = [&](int s, int slot) {
#pragma unroll
    for (int f2 = 0; f2 < 2; ++f2) {
      const int fi = wave + 8 * f2;
      const int ks = s * KPS + fi / (NP * 4), tap = ks / G::KSI;
      const unsigned uni = (unsigned)(ks * 64 + w1a - tap * w1b);
      // stages past the last one keep the vmcnt arithmetic uniform: they read zeros into a slot nobody reads
      dma16_asm(rw, ring + slot * kStageBytes + fi * 1024, s < G::NST ? wl[f2] + uni : kOOB);
    }
  };
#pragma unroll
  for (int s = 0; s < S - 1; ++s) stage(s, s);

  // ---- this wave's pixel fragments: fragment u = output row frow(u), pixels 16 fj(u) .. + 15.  B-fragment byte
  // offsets within a plane (without the filter row): staged pixel 16 j + li + kw (clamped for pixels past the
  // row: their results are never stored nor counted), channel chunk g of the first half; the second half is ^ 64
  auto frow = [&](int u) { return (pg * FPW + u) / G::TPW; };
  auto fj = [&](int u) { return (pg * FPW + u) % G::TPW; };
  // (per lane only the column part: fragments u and u + TPW share it; the row part is wave-uniform)
  int boff[G::TPW][3];
#pragma unroll
  for (int x = 0; x < G::TPW; ++x)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      int px = 16 * fj(x) + li + kw;
      px = px < G::WP - 1 ? px : G::WP - 1;
      boff[x][kw] = px * 128 + ((16 * g) ^ ((px & 6) << 4));
    }

  float4v acc[4][FPW];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int u = 0; u < FPW; ++u) acc[i][u] = float4v{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int kh = 0; kh < 3; ++kh) {
    // whole image resident: the wave's first / last fragment row has no input row above / below the image
    const bool skip_lo = G::FULL && kh == 0 && pg == 0, skip_hi = G::FULL && kh == 2 && pg == G::PG - 1;
    const char* rows = lds + (kh - 1 - G::R0) * G::pitch;      // fragment row f, tap row kh: staged row f + kh - 1 - R0
#pragma unroll
    for (int t = 0; t < G::SPK; ++t) {
      // stages up to kh SPK + t + S - 2 are issued; vmcnt retires in order: at most S - 2 stages may still fly
      wait_vmcnt<(S - 2) * 2>();
      // every wave's DMA of this stage is in, and every wave's reads of the previous stage are complete
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      stage(kh * G::SPK + t + S - 1, (t + S - 1) % S);
      const char* fr = ring + (t % S) * kStageBytes + lane * 16;
#pragma unroll
      for (int q = 0; q < KPS; ++q) {
        const int kk = t * KPS + q, kw = kk / G::KSI, c32 = kk % G::KSI;
        const char* pb = rows + (c32 >> 1) * G::plane;
        bf16x8_t af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          af[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(fr + ((q * NP + cg) * 4 + i) * 1024));
        bf16x8_t b[FPW];
#pragma unroll
        for (int u = 0; u < FPW; ++u) {
          // a skipped fragment reads the row below / above instead (in range, unused)
          const int fr_u = frow(u) + (u == 0 && skip_lo ? 1 : u == FPW - 1 && skip_hi ? -1 : 0);
          b[u] = __builtin_bit_cast(
              bf16x8_t, *reinterpret_cast<const uint4*>(pb + fr_u * G::pitch + (boff[u % G::TPW][kw] ^ ((c32 & 1) * 64))));
        }
#pragma unroll
        for (int u = 0; u < FPW; ++u) {
          if (u == 0 && skip_lo) continue;
          if (u == FPW - 1 && skip_hi) continue;
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i][u] = mfma(af[i], b[u], acc[i][u]);
        }
      }
    }
  }

  // ---- epilogue.  The ring is free once the trailing (zero) stages have landed: it holds the block's statistics
  float* stat_s = reinterpret_cast<float*>(ring);        // [2][C] block partials
  wait_vmcnt<0>();
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (E::stats || E::bstat) {
    if (threadIdx.x < 2 * C) stat_s[threadIdx.x] = 0.f;
    __syncthreads();
  }

  // fragment layout (chunk g, pixel li) -> row layout (pixel rp, chunk rc), 2 x 16-B stores per pixel (as
  // conv_ws_kernel's: conflict-free ds_bpermute sources); statistics per lane, row-reduced with DPP
  const int rp = (lane & 31) >> 1, rc = (lane & 1) | ((lane >> 5) << 1);
  const int xsrc = (16 * rc + rp) * 4;
  auto xpose = [&](const uint4& v) {
    return make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(xsrc, (int)v.x),
                      (uint32_t)__builtin_amdgcn_ds_bpermute(xsrc, (int)v.y),
                      (uint32_t)__builtin_amdgcn_ds_bpermute(xsrc, (int)v.z),
                      (uint32_t)__builtin_amdgcn_ds_bpermute(xsrc, (int)v.w));
  };
  float s0[16], s1[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) s0[e] = s1[e] = 0.f;
#pragma unroll
  for (int u = 0; u < FPW; ++u) {
    float v0[8], v1[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v0[r] = acc[0][u][r];
      v0[4 + r] = acc[1][u][r];
      v1[r] = acc[2][u][r];
      v1[4 + r] = acc[3][u][r];
    }
    if (E::stats && 16 * fj(u) + li < WI) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s0[e] += v0[e];
        s1[e] += v0[e] * v0[e];
        s0[8 + e] += v1[e];
        s1[8 + e] += v1[e] * v1[e];
      }
    }
    const uint4 w0 = xpose(pack8(v0)), w1 = xpose(pack8(v1));
    const int ow = 16 * fj(u) + rp;
    if (ow < WI) {
      const long long off = (((long long)n * H + oh0 + frow(u)) * WI + ow) * C + cg * 64 + 8 * rc;
      if (E::bstat) {
        // statistics of the gradient as stored (bf16), like a separate reduction would see it
        const uint4 x0v = *reinterpret_cast<const uint4*>(bx + off), x1v = *reinterpret_cast<const uint4*>(bx + off + 32);
        const uint32_t mk0 = bmask ? bmask[off >> 3] : 0xffu, mk1 = bmask ? bmask[(off + 32) >> 3] : 0xffu;
        float q0[8], q1[8], xa[8], xb[8];
        unpack8(w0, q0);
        unpack8(w1, q1);
        unpack8(x0v, xa);
        unpack8(x1v, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ga = ((mk0 >> e) & 1u) ? q0[e] : 0.f;
          const float gb = ((mk1 >> e) & 1u) ? q1[e] : 0.f;
          s0[e] += ga;
          s1[e] += ga * xa[e];
          s0[8 + e] += gb;
          s1[8 + e] += gb * xb[e];
        }
      }
      bf16_t* o = out + off;
      *reinterpret_cast<uint4*>(o) = w0;
      *reinterpret_cast<uint4*>(o + 32) = w1;
    }
  }
  if (E::stats) {              // fragment layout: channel chunk g, reduce over li
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s0[e] = row_sum16_all(s0[e]);
      s1[e] = row_sum16_all(s1[e]);
    }
    if (li == 15) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = cg * 64 + (e < 8 ? 8 * g + e : 32 + 8 * g + (e - 8));
        atomicAdd(stat_s + c, s0[e]);
        atomicAdd(stat_s + C + c, s1[e]);
      }
    }
  }
  if (E::bstat) {              // row layout: chunk rc = (lane & 1) | (lane >> 5) << 1, reduce over lane bits 1-4
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      s0[e] = row_sum8_pairs(s0[e]);
      s1[e] = row_sum8_pairs(s1[e]);
    }
    if (li >= 14) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int c = cg * 64 + (e < 8 ? 8 * rc + e : 32 + 8 * rc + (e - 8));
        atomicAdd(stat_s + c, s0[e]);
        atomicAdd(stat_s + C + c, s1[e]);
      }
    }
  }
  if (E::stats || E::bstat) {
    __syncthreads();
    if (threadIdx.x < 2 * C) {
      float* dst = (threadIdx.x < C ? ps0 : ps1) + (long long)(blockIdx.x % slots) * C + (threadIdx.x % C);
      atomicAdd(dst, stat_s[threadIdx.x]);
    }
  }
}

template <int EPI, int WI, int C>
void launch_img(const void* src, const void* wgt, void* out, int N, int H, int wmode, float* s0, float* s1, int slots,
                const void* bx, const void* bmask, hipStream_t st) {
  using G = ImgGeom<WI, C>;
  const size_t lds = (size_t)G::act + (size_t)G::S * kStageBytes;
  static_assert(G::act + G::S * kStageBytes <= kLdsBytes && 2 * C * sizeof(float) <= kStageBytes, "LDS budget");
  hipLaunchKernelGGL((conv3_img<EPI, WI, C>), dim3((unsigned)(N * (H / kBand))), dim3(512), lds, st, (const bf16_t*)src,
                     (const bf16_t*)wgt, (bf16_t*)out, H, wmode, (int)((long long)N * H * WI * C * 2), s0, s1,
                     slots > 0 ? slots : 1, (const bf16_t*)bx, (const uint8_t*)bmask);
}

template <int WI, int C>
void launch_img_epi(const void* src, const void* wgt, void* out, int N, int H, int wmode, float* s0, float* s1,
                    int slots, const void* bx, const void* bmask, hipStream_t st) {
  if (!s0)
    launch_img<0, WI, C>(src, wgt, out, N, H, wmode, s0, s1, slots, bx, bmask, st);
  else if (wmode == 0)
    launch_img<1, WI, C>(src, wgt, out, N, H, wmode, s0, s1, slots, bx, bmask, st);
  else
    launch_img<3, WI, C>(src, wgt, out, N, H, wmode, s0, s1, slots, bx, bmask, st);
}
}  // namespace

// MDTF_CONV_IMG: the (shape, pass) set that mdtf_conv_fwd_v2 / mdtf_conv_dgrad_v2 route here, as a bit mask:
// 1 = 28x28x128 forward, 2 = 28x28x128 data gradient, 4 = 14x14x256 forward, 8 = 14x14x256 data gradient.
// 0 restores conv_fd_v2 everywhere; unset = the pairs that won the in-step A/B (profiles/conv_img.md).
MDTF_EXPORT int mdtf_get_deterministic();   // kernels.hip

namespace {
constexpr int kImgDefaultMask = 15;     // every pair won, per call and in the step (profiles/conv_img.md)
std::atomic<int> g_img_mask{-1};      // >= 0: a test or probe overrides the environment for this process
}  // namespace

MDTF_EXPORT int mdtf_conv_img_mask() {
  static const int env = [] {
    const char* e = getenv("MDTF_CONV_IMG");
    return e && e[0] ? atoi(e) & 15 : kImgDefaultMask;
  }();
  const int over = g_img_mask.load(std::memory_order_relaxed);
  return over >= 0 ? over : env;
}

// override the mask for this process (tests, probes); negative: back to the environment's
MDTF_EXPORT void mdtf_set_conv_img_mask(int mask) {
  g_img_mask.store(mask < 0 ? -1 : (mask & 15), std::memory_order_relaxed);
}

// 1 if (H, W, C, pass) is routed to conv3_img by the mask above (wmode 0 forward, 1 data gradient)
MDTF_EXPORT int mdtf_conv_img_routed(int H, int W, int C, int wmode) {
  const int shape = (H == 28 && W == 28 && C == 128) ? 0 : (H == 14 && W == 14 && C == 256) ? 1 : -1;
  // deterministic mode sizes the statistics rows by conv_fd_v2's tiles (one writer per row): stay there
  if (shape < 0 || (wmode != 0 && wmode != 1) || mdtf_get_deterministic()) return 0;
  return (mdtf_conv_img_mask() >> (2 * shape + wmode)) & 1;
}

// out[N][H][W][C] = conv3x3(src[N][H][W][C], filter), stride 1, pad 1; (H, W, C) = (28, 28, 128) or (14, 14, 256).
// wmode 0: wgt = Wt[C][9*C] (transpose_filter); s0/s1 non-null: forward BN statistics ([slots][C] partials).
// wmode 1: wgt = HWIO [3][3][C][C] used flipped, src = DY, out = DX; s0/s1 non-null: BN-backward statistics
// of DX against bx (the BN input) and the optional ReLU bitmask bmask.
MDTF_EXPORT int mdtf_conv3_img(const void* src, const void* wgt, void* out, int N, int H, int W, int C, int wmode,
                               float* s0, float* s1, int slots, const void* bx, const void* bmask, hipStream_t st) {
  if (N < 1 || (wmode != 0 && wmode != 1) || (!s0) != (!s1)) return MDTF_EINVAL;
  if (wmode == 1 && s0 && !bx) return MDTF_EINVAL;
  if ((long long)N * H * W * C * 2 >= 0x80000000LL) return MDTF_EUNSUPPORTED;   // 32-bit buffer offsets
  if (H == 28 && W == 28 && C == 128)
    launch_img_epi<28, 128>(src, wgt, out, N, H, wmode, s0, s1, slots, bx, bmask, st);
  else if (H == 14 && W == 14 && C == 256)
    launch_img_epi<14, 256>(src, wgt, out, N, H, wmode, s0, s1, slots, bx, bmask, st);
  else
    return MDTF_EUNSUPPORTED;
  MDTF_LAUNCH_CHECK();
  return 0;
}
