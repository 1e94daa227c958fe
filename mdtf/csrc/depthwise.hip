// tf.nn.depthwise_conv2d (channel multiplier 1) on bf16 NHWC: forward, data gradient and weight gradient as direct,
// memory-bound kernels.  kh * kw multiply-adds per element loaded: no MFMA, the streaming form of the pooling kernels.
//
//   fwd     y[n, oh, ow, c]  = sum_{i, j} x[n, oh * sh + i * dh - pt, ow * sw + j * dw - pl, c] * w[i, j, c]
//   dgrad   dx[n, h, w, c]   = sum_{i, j} dy[n, (h + pt - i * dh) / sh, (w + pl - j * dw) / sw, c] * w[i, j, c]
//                              over the taps whose quotient is exact and inside the OH x OW plane (gather form)
//   wgrad   dw[i, j, c]      = sum_{n, oh, ow} x[n, oh * sh + i * dh - pt, ow * sw + j * dw - pl, c] * dy[n, oh, ow, c]
//
// fwd / dgrad are one kernel template.  A lane owns 8 consecutive channels of one destination pixel: a 16-byte load
// per tap, a 16-byte store.  A tap outside the source plane is tested before its address is formed and is never
// loaded.  The taps are summed in fp32 in (i, j) order with written-out fused multiply-adds (contraction off, as in
// optim.hip), then rounded once to bf16, so the result does not depend on the mapping.  A block covers a patch of
// tw x (th * rows) adjacent destination pixels of one image for up to 8 channel groups; the halo re-reads of a patch
// hit the cache, and the filter slice of the block's channels is staged in LDS once per block.  3x3 and 5x5 at
// stride 1 / 2 with dilation 1 are template instances whose tap loops unroll; everything else (kh * kw <= 49, any
// stride / dilation / pads) takes the generic instance.
//
// wgrad has no float atomics.  Phase 1: a block takes one contiguous chunk of the N * OH * OW output pixels, up to 8
// channel groups and up to 9 taps; a thread walks the chunk's pixels with a stride of the block's pixel lanes and
// keeps (taps x 8) fp32 sums in registers; the block adds them over its pixel lanes through LDS in lane order and
// stores one partial [chunk][kh * kw][C].  Phase 2 (finalize): one thread per (tap, channel) adds the partials in
// chunk order in fp64 and stores to, or adds into, the fp32 [kh, kw, C, 1] destination.  Every element of the
// workspace and of the destination is stored, and the result is bitwise repeatable.
//
// Nothing is read back by the host and nothing is allocated: every launch replays inside a captured step.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kMaxTaps = 49;
constexpr int kMaxCgb = 8;                       // channel groups (of 8 channels) per block
constexpr int kTG = 9;                           // wgrad: taps per block (72 fp32 sums per thread)
constexpr int kRedTaps = 3;                      // wgrad: taps per LDS reduction round (24 KiB)
constexpr int kMinIters = 16;                    // wgrad: least pixels per pixel lane in a full chunk
constexpr int kTargetBlocks = 768;               // wgrad: about 3 blocks per CU before chunks grow

struct DwGeo {
  int N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PL;
};

struct DwTile {
  int cgb, cgblocks, tw, th, rows, tiles_w, tiles_h;
};

__device__ __forceinline__ void unpack8(const uint4 raw, float (&f)[8]) {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ void fma8(const uint4 a, const uint4 b, float (&acc)[8]) {
#pragma clang fp contract(off)
  float fa[8], fb[8];
  unpack8(a, fa);
  unpack8(b, fb);
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(fa[k], fb[k], acc[k]);
}

// The source coordinate of tap t along one axis for destination coordinate d, and whether it exists.
//   forward: s = d * stride + t * dil - pad inside [0, n_src)
//   dgrad:   q = d + pad - t * dil >= 0, divisible by stride, s = q / stride < n_src
template <int S, bool DGRAD>
__device__ __forceinline__ bool tap_src(int d, int t, int stride, int dil, int pad, int n_src, int& s) {
  const int st = S > 0 ? S : stride;
  if constexpr (!DGRAD) {
    s = d * st + t * dil - pad;
    return s >= 0 && s < n_src;
  } else {
    const int q = d + pad - t * dil;
    if (q < 0) return false;
    if constexpr (S == 1) {
      s = q;
    } else if constexpr (S == 2) {
      if (q & 1) return false;
      s = q >> 1;
    } else {
      s = q / st;
      if (s * st != q) return false;
    }
    return s < n_src;
  }
}

// KH = KW = S = 0: the generic instance (runtime filter size, strides and dilations)
template <int KH, int KW, int S, bool DGRAD>
__global__ void __launch_bounds__(kT) dw_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wt,
                                                bf16_t* __restrict__ dst, DwGeo g, DwTile tl) {
  __shared__ uint4 wl[kMaxTaps * kMaxCgb];
  const int kh = KH > 0 ? KH : g.KH, kw = KW > 0 ? KW : g.KW;
  const int dh = KH > 0 ? 1 : g.DH, dw = KH > 0 ? 1 : g.DW;
  const int CG = g.C >> 3;
  // destination / source planes
  const int DH_ = DGRAD ? g.H : g.OH, DW_ = DGRAD ? g.W : g.OW;
  const int SH_ = DGRAD ? g.OH : g.H, SW_ = DGRAD ? g.OW : g.W;

  int b = blockIdx.x;
  const int cgblk = b % tl.cgblocks;
  b /= tl.cgblocks;
  const int tx = b % tl.tiles_w;
  b /= tl.tiles_w;
  const int ty = b % tl.tiles_h;
  const int n = b / tl.tiles_h;

  const int tid = threadIdx.x;
  const int taps = kh * kw;
  for (int e = tid; e < taps * tl.cgb; e += kT) {
    const int t = e / tl.cgb, cl = e - t * tl.cgb;
    const int cg = cgblk * tl.cgb + cl;
    if (cg < CG) wl[e] = reinterpret_cast<const uint4*>(wt)[(long long)t * CG + cg];
  }
  __syncthreads();

  const int cl = tid % tl.cgb, p = tid / tl.cgb;
  const int px = p % tl.tw, py = p / tl.tw;
  const int cg = cgblk * tl.cgb + cl;
  const int x = tx * tl.tw + px;
  if (cg >= CG || x >= DW_ || py >= tl.th || n >= g.N) return;
  const bf16_t* sp = src + (long long)n * SH_ * SW_ * g.C + cg * 8;
  bf16_t* dp = dst + (long long)n * DH_ * DW_ * g.C + cg * 8;

  for (int r = 0; r < tl.rows; ++r) {
    const int y = (ty * tl.rows + r) * tl.th + py;
    if (y >= DH_) break;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (KH > 0) {
#pragma unroll
      for (int i = 0; i < KH; ++i) {
        int sy = 0;
        const bool oky = tap_src<S, DGRAD>(y, i, g.SH, 1, g.PT, SH_, sy);
        uint4 raw[KW];
        bool ok[KW];
#pragma unroll
        for (int j = 0; j < KW; ++j) {
          int sx = 0;
          ok[j] = tap_src<S, DGRAD>(x, j, g.SW, 1, g.PL, SW_, sx) && oky;
          raw[j] = make_uint4(0u, 0u, 0u, 0u);
          if (ok[j]) raw[j] = *reinterpret_cast<const uint4*>(sp + ((long long)sy * SW_ + sx) * g.C);
        }
#pragma unroll
        for (int j = 0; j < KW; ++j)
          if (ok[j]) fma8(raw[j], wl[(i * KW + j) * tl.cgb + cl], acc);
      }
    } else {
      for (int i = 0; i < kh; ++i) {
        int sy = 0;
        if (!tap_src<0, DGRAD>(y, i, g.SH, dh, g.PT, SH_, sy)) continue;
        for (int j = 0; j < kw; ++j) {
          int sx = 0;
          if (!tap_src<0, DGRAD>(x, j, g.SW, dw, g.PL, SW_, sx)) continue;
          const uint4 raw = *reinterpret_cast<const uint4*>(sp + ((long long)sy * SW_ + sx) * g.C);
          fma8(raw, wl[(i * kw + j) * tl.cgb + cl], acc);
        }
      }
    }
    store_bf8(dp + ((long long)y * DW_ + x) * g.C, acc);
  }
}

struct WgPlan {
  int cgb, cgblocks, tgroups, chunk, nchunks;
};

__global__ void __launch_bounds__(kT) dw_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                      float* __restrict__ ws, DwGeo g, WgPlan pl, int P) {
  __shared__ __attribute__((aligned(16))) float red[kT * kRedTaps * 8];
  const int CG = g.C >> 3, T = g.KH * g.KW;
  int b = blockIdx.x;
  const int tgp = b % pl.tgroups;
  b /= pl.tgroups;
  const int cgblk = b % pl.cgblocks;
  const int ck = b / pl.cgblocks;
  const int tid = threadIdx.x;
  const int cgb = pl.cgb, PB = kT / cgb;          // cgb is a power of two: PB * cgb == kT
  const int cl = tid % cgb, lane = tid / cgb;
  const int cg = cgblk * cgb + cl;
  const int t0 = tgp * kTG;

  int ti[kTG], tj[kTG];
  bool tv[kTG];
#pragma unroll
  for (int t = 0; t < kTG; ++t) {
    tv[t] = t0 + t < T;
    ti[t] = tv[t] ? (t0 + t) / g.KW : 0;
    tj[t] = tv[t] ? (t0 + t) - ti[t] * g.KW : 0;
  }
  float acc[kTG][8];
#pragma unroll
  for (int t = 0; t < kTG; ++t)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;

  const int p0 = ck * pl.chunk;                   // ck < nchunks: p0 < P
  const int p1 = P - p0 < pl.chunk ? P : p0 + pl.chunk;
  const int plane = g.OH * g.OW;
  if (cg < CG) {
    for (int p = p0 + lane; p < p1; p += PB) {
      const int n = p / plane, r = p - n * plane;
      const int oh = r / g.OW, ow = r - oh * g.OW;
      const uint4 dv = *reinterpret_cast<const uint4*>(dy + (long long)p * g.C + cg * 8);
      const bf16_t* xp = x + (long long)n * g.H * g.W * g.C + cg * 8;
#pragma unroll
      for (int t = 0; t < kTG; ++t) {
        const int ih = oh * g.SH + ti[t] * g.DH - g.PT, iw = ow * g.SW + tj[t] * g.DW - g.PL;
        if (tv[t] && ih >= 0 && ih < g.H && iw >= 0 && iw < g.W) {
          const uint4 xv = *reinterpret_cast<const uint4*>(xp + ((long long)ih * g.W + iw) * g.C);
          fma8(xv, dv, acc[t]);
        }
      }
    }
  }

  // the block's sums over its pixel lanes, kRedTaps taps per round, in lane order
  const int E = kRedTaps * cgb * 8;               // <= 192 outputs per round
#pragma unroll
  for (int r = 0; r < kTG / kRedTaps; ++r) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kRedTaps; ++q) {
      float* o = red + ((q * PB + lane) * cgb + cl) * 8;
      const float(&a)[8] = acc[r * kRedTaps + q];
      reinterpret_cast<float4*>(o)[0] = make_float4(a[0], a[1], a[2], a[3]);
      reinterpret_cast<float4*>(o)[1] = make_float4(a[4], a[5], a[6], a[7]);
    }
    __syncthreads();
    if (tid < E) {
      const int q = tid / (cgb * 8), c8 = tid - q * (cgb * 8);
      float s = 0.f;
      for (int l = 0; l < PB; ++l) s += red[(q * PB + l) * cgb * 8 + c8];
      const int t = t0 + r * kRedTaps + q, c = cgblk * cgb * 8 + c8;
      if (t < T && c < g.C) ws[((long long)ck * T + t) * g.C + c] = s;
    }
  }
}

__global__ void __launch_bounds__(kT) dw_wgrad_finalize_kernel(const float* __restrict__ ws, float* __restrict__ dst,
                                                               int nchunks, int TC, int accumulate) {
  const int e = blockIdx.x * kT + threadIdx.x;
  if (e >= TC) return;
  double s = 0.0;
  for (int ck = 0; ck < nchunks; ++ck) s += static_cast<double>(ws[(long long)ck * TC + e]);
  if (accumulate) s += static_cast<double>(dst[e]);
  dst[e] = static_cast<float>(s);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int pow2_cgb(int CG) {
  int c = 1;
  while (c < CG && c < kMaxCgb) c <<= 1;
  return c;
}

// The sizes, and OH / OW as they follow from H, W, the filter, strides, dilations and the four pads.
bool geometry_ok(int N, int H, int W, int C, int OH, int OW, int KH, int KW, int SH, int SW, int DH, int DW, int PT,
                 int PB, int PL, int PR) {
  if (N < 0 || H < 1 || W < 1 || C < 8 || (C & 7) || OH < 1 || OW < 1) return false;
  if (KH < 1 || KW < 1 || (long long)KH * KW > kMaxTaps || SH < 1 || SW < 1 || DH < 1 || DW < 1) return false;
  if (PT < 0 || PB < 0 || PL < 0 || PR < 0) return false;
  const long long eh = (long long)(KH - 1) * DH + 1, ew = (long long)(KW - 1) * DW + 1;
  const long long fh = (long long)H + PT + PB - eh, fw = (long long)W + PL + PR - ew;
  if (fh < 0 || fw < 0 || fh / SH + 1 != OH || fw / SW + 1 != OW) return false;
  // pixel counts fit an int, padded coordinates too
  if ((long long)N * H * W >= (1ll << 31) || (long long)N * OH * OW >= (1ll << 31)) return false;
  if ((long long)H + PT + PB + eh >= (1ll << 30) || (long long)W + PL + PR + ew >= (1ll << 30)) return false;
  return true;
}

// the patch of destination pixels a block covers: DHp x DWp is the destination plane
bool make_tile(int N, int DHp, int DWp, int C, DwTile* tl) {
  const int CG = C >> 3;
  tl->cgb = pow2_cgb(CG);
  tl->cgblocks = static_cast<int>(ceil_div(CG, tl->cgb));
  const int pb = kT / tl->cgb;                                  // 32, 64, 128 or 256 pixels
  tl->tw = pb >= 128 ? 16 : 8;
  tl->th = pb / tl->tw;
  tl->tiles_w = static_cast<int>(ceil_div(DWp, tl->tw));
  const long long per_row = (long long)N * tl->tiles_w * tl->cgblocks;
  tl->rows = 1;
  for (int r = 4; r > 1; r >>= 1)
    if (per_row * ceil_div(DHp, tl->th * r) >= 1024) {
      tl->rows = r;
      break;
    }
  tl->tiles_h = static_cast<int>(ceil_div(DHp, tl->th * tl->rows));
  return per_row * tl->tiles_h < (1ll << 31);
}

template <bool DGRAD>
int launch_dw(const void* src, const void* w, void* dst, const DwGeo& g, hipStream_t st) {
  DwTile tl;
  if (!make_tile(g.N, DGRAD ? g.H : g.OH, DGRAD ? g.W : g.OW, g.C, &tl)) return MDTF_EINVAL;
  const dim3 grid(static_cast<unsigned>((long long)g.N * tl.tiles_w * tl.tiles_h * tl.cgblocks));
  const bf16_t* s = static_cast<const bf16_t*>(src);
  const bf16_t* wt = static_cast<const bf16_t*>(w);
  bf16_t* d = static_cast<bf16_t*>(dst);
  const bool unit = g.DH == 1 && g.DW == 1 && g.SH == g.SW;
#define MDTF_DW_LAUNCH(KH_, KW_, S_) \
  hipLaunchKernelGGL((dw_kernel<KH_, KW_, S_, DGRAD>), grid, dim3(kT), 0, st, s, wt, d, g, tl)
  if (unit && g.KH == 3 && g.KW == 3 && g.SH == 1)
    MDTF_DW_LAUNCH(3, 3, 1);
  else if (unit && g.KH == 3 && g.KW == 3 && g.SH == 2)
    MDTF_DW_LAUNCH(3, 3, 2);
  else if (unit && g.KH == 5 && g.KW == 5 && g.SH == 1)
    MDTF_DW_LAUNCH(5, 5, 1);
  else if (unit && g.KH == 5 && g.KW == 5 && g.SH == 2)
    MDTF_DW_LAUNCH(5, 5, 2);
  else
    MDTF_DW_LAUNCH(0, 0, 0);
#undef MDTF_DW_LAUNCH
  MDTF_LAUNCH_CHECK();
  return 0;
}

WgPlan wgrad_plan(long long P, int C, int T) {
  WgPlan pl;
  const int CG = C >> 3;
  pl.cgb = pow2_cgb(CG);
  pl.cgblocks = static_cast<int>(ceil_div(CG, pl.cgb));
  pl.tgroups = static_cast<int>(ceil_div(T, kTG));
  const int pb = kT / pl.cgb;
  const long long target = kTargetBlocks / ((long long)pl.cgblocks * pl.tgroups);
  long long ch = ceil_div(P > 0 ? P : 1, target > 0 ? target : 1);
  ch = ceil_div(ch, pb) * pb;
  if (ch < (long long)kMinIters * pb) ch = (long long)kMinIters * pb;
  pl.chunk = static_cast<int>(ch);                             // <= P + 16 * 256 < 2^31 + ...: P < 2^31 - 2^13 is checked
  pl.nchunks = static_cast<int>(ceil_div(P > 0 ? P : 1, ch));
  return pl;
}

inline bool wgrad_sizes_ok(int N, int OH, int OW, int C, int KH, int KW) {
  return N >= 0 && OH >= 1 && OW >= 1 && C >= 8 && C <= (1 << 24) && !(C & 7) && KH >= 1 && KW >= 1 && (long long)KH * KW <= kMaxTaps &&
         (long long)N * OH * OW < (1ll << 31) - (1ll << 13);
}

}  // namespace

// y = depthwise_conv2d(x, w): x bf16 [N, H, W, C], w bf16 [KH, KW, C, 1], y bf16 [N, OH, OW, C], all contiguous and
// 16-byte aligned.  OH = (H + PT + PB - (KH - 1) * DH - 1) / SH + 1 and the same for OW, or MDTF_EINVAL.
MDTF_EXPORT int mdtf_dwconv_fwd(const void* x, const void* w, void* y, int N, int H, int W, int C, int OH, int OW,
                                int KH, int KW, int SH, int SW, int DH, int DW, int PT, int PB, int PL, int PR,
                                hipStream_t st) {
  if (!geometry_ok(N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PB, PL, PR)) return MDTF_EINVAL;
  if (!x || !w || !y || !aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16)) return MDTF_EINVAL;
  if (N == 0) return 0;
  const DwGeo g{N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PL};
  return launch_dw<false>(x, w, y, g, st);
}

// dx = the gradient of mdtf_dwconv_fwd with respect to x for dy [N, OH, OW, C]; every element of dx is stored
MDTF_EXPORT int mdtf_dwconv_dgrad(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int OH, int OW,
                                  int KH, int KW, int SH, int SW, int DH, int DW, int PT, int PB, int PL, int PR,
                                  hipStream_t st) {
  if (!geometry_ok(N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PB, PL, PR)) return MDTF_EINVAL;
  if (!dy || !w || !dx || !aligned(dy, 16) || !aligned(w, 16) || !aligned(dx, 16)) return MDTF_EINVAL;
  if (N == 0) return 0;
  const DwGeo g{N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PL};
  return launch_dw<true>(dy, w, dx, g, st);
}

// floats of workspace mdtf_dwconv_wgrad writes and mdtf_dwconv_wgrad_finalize reads: [chunks][KH * KW][C]
// (0 for sizes the kernels refuse)
MDTF_EXPORT long long mdtf_dwconv_wgrad_ws(int N, int OH, int OW, int C, int KH, int KW) {
  if (!wgrad_sizes_ok(N, OH, OW, C, KH, KW)) return 0;
  const WgPlan pl = wgrad_plan((long long)N * OH * OW, C, KH * KW);
  return (long long)pl.nchunks * KH * KW * C;
}

// output pixels per chunk (one partial each) for these sizes
MDTF_EXPORT long long mdtf_dwconv_wgrad_chunk(int N, int OH, int OW, int C, int KH, int KW) {
  if (!wgrad_sizes_ok(N, OH, OW, C, KH, KW)) return 0;
  return wgrad_plan((long long)N * OH * OW, C, KH * KW).chunk;
}

// phase 1: the per-chunk partial sums of dw into ws (mdtf_dwconv_wgrad_ws floats, 16-byte aligned)
MDTF_EXPORT int mdtf_dwconv_wgrad(const void* x, const void* dy, float* ws, int N, int H, int W, int C, int OH, int OW,
                                  int KH, int KW, int SH, int SW, int DH, int DW, int PT, int PB, int PL, int PR,
                                  hipStream_t st) {
  if (!geometry_ok(N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PB, PL, PR)) return MDTF_EINVAL;
  if (!wgrad_sizes_ok(N, OH, OW, C, KH, KW)) return MDTF_EINVAL;
  if (!x || !dy || !ws || !aligned(x, 16) || !aligned(dy, 16) || !aligned(ws, 16)) return MDTF_EINVAL;
  const long long P = (long long)N * OH * OW;
  const WgPlan pl = wgrad_plan(P, C, KH * KW);
  const long long blocks = (long long)pl.nchunks * pl.cgblocks * pl.tgroups;
  if (blocks >= (1ll << 31)) return MDTF_EINVAL;
  const DwGeo g{N, H, W, C, OH, OW, KH, KW, SH, SW, DH, DW, PT, PL};
  hipLaunchKernelGGL(dw_wgrad_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kT), 0, st,
                     static_cast<const bf16_t*>(x), static_cast<const bf16_t*>(dy), ws, g, pl, static_cast<int>(P));
  MDTF_LAUNCH_CHECK();
  return 0;
}

// phase 2: dw[KH, KW, C, 1] (fp32) = (accumulate ? dw : 0) + the partials of ws in chunk order, summed in fp64
MDTF_EXPORT int mdtf_dwconv_wgrad_finalize(const float* ws, float* dw, int N, int OH, int OW, int C, int KH, int KW,
                                           int accumulate, hipStream_t st) {
  if (!wgrad_sizes_ok(N, OH, OW, C, KH, KW)) return MDTF_EINVAL;
  if (!ws || !dw || !aligned(ws, 16) || !aligned(dw, 4)) return MDTF_EINVAL;
  const WgPlan pl = wgrad_plan((long long)N * OH * OW, C, KH * KW);
  const int TC = KH * KW * C;
  hipLaunchKernelGGL(dw_wgrad_finalize_kernel, dim3(static_cast<unsigned>(ceil_div(TC, kT))), dim3(kT), 0, st, ws, dw,
                     pl.nchunks, TC, accumulate != 0);
  MDTF_LAUNCH_CHECK();
  return 0;
}
