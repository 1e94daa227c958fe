// Grouped 3x3 convolution (the conv2 of a ResNeXt bottleneck) on bf16 NHWC: forward, data gradient and weight
// gradient as streaming kernels that feed zero-padded block-diagonal filter fragments to the MFMA units.
//
//   x [N, H, W, C], w [3, 3, Cg, C] (HWIO with the per-group input count), G = C / Cg groups, C in = C out:
//   fwd     y[n, oh, ow, co]  = sum_{ky, kx, j} x[n, oh s + ky - pt, ow s + kx - pl, g Cg + j] w[ky, kx, j, co],  g = co / Cg
//   dgrad   dx[n, ih, iw, ci] = sum over the taps whose (ih + pt - ky) / s, (iw + pl - kx) / s are exact and inside
//                               the OH x OW plane, and over the Cg output channels of ci's group
//   wgrad   dw[ky, kx, j, co] = sum_{n, oh, ow} x[n, oh s + ky - pt, ow s + kx - pl, g Cg + j] dy[n, oh, ow, co]
//   taps outside the image contribute 0; fp32 accumulation, one rounding to bf16.
//   Taken: Cg in {4, 8, 16, 32}, C % 32 == 0, stride 1 or 2, dilation 1, every pad <= 2, any N, H, W >= 1 (one image
//   below 2 GiB).  Everything else returns MDTF_EUNSUPPORTED and the caller runs the library.
//
// Why not the implicit GEMMs: per group this is a GEMM with N = 4..32 and K = 36..288, far below an MFMA tile, and
// the op is memory-bound (56 x 56 x 128 at batch 256 reads and writes 205 MB each).  So every activation byte moves
// once and spare matrix throughput is spent on padding:
//   * Work split.  Groups never mix, so the channel axis splits without redundancy into 32-channel slabs of 8, 4,
//     2 or 1 whole groups.  A 256-thread block owns one slab, one tile of `band` output rows x `tw` output columns
//     (tw = the whole row up to 64 columns) and a strided set of images, for which it keeps its filter fragments.
//     Slabs are the fastest block index, so the blocks that read the two halves of a 128-B line run together.
//     band <= 8 rows, evened over the image and capped by 40 KiB of LDS: 7 x 32 x 4, 4 x 32 x 8, 2 x 32 x 16 and
//     1 x 32 x 32 = 896 .. 1024 blocks at the four ResNeXt-50 32x4d shapes at batch 32.  Only the halo rows of a
//     band (and the halo columns of a column tile) are read twice.
//   * Resident: the filter.  Each wave expands the slab's 9 taps once, global -> registers, into 9 x 2 A fragments
//     (M = 16 output channels, K = input channels): Cg = 32 two dense 16x16x32 fragments per tap; Cg = 16 the two
//     diagonal 16 x 16 blocks as 16x16x16 fragments (no zero work); Cg = 8 / 4 the same two blocks with the
//     off-group entries zero (2x / 4x padded work).  72 / 36 VGPRs.
//   * Streams: the input.  The tile's (band - 1) s + 3 input rows x (tw - 1) s + 3 columns of the slab are staged
//     once in LDS by LDS-DMA, 64 B per pixel; halo rows / columns and everything outside the image are zero-filled
//     through the buffer descriptor, so the MFMA loop has no bounds tests.  Placement: staged pixel q keeps its
//     16-B channel chunk c at slot c ^ ((q >> 2) & 3): 16 consecutive pixels x one chunk cover the 64 banks once
//     (ds_read_b128, Cg = 32), and 16 pixels x the two 8-B halves of a chunk too (ds_read_b64, Cg <= 16).  At stride
//     2 the columns of a staged row are de-interleaved (even columns first, odd columns from `half`), so the
//     every-other-pixel reads of a tap are pixel step 1 in LDS as well.  Bytes per block and image:
//     rows_in x wps x 64, e.g. 10 x 58 x 64 = 36 KiB (56 x 56, band 8), 9 x 58 x 64 = 33 KiB (56 -> 28, band 4).
//   * Pixel fragments are 16 output pixels of the flattened tile (p = r tw + c), so a 7 x 7 map fills 49 of 64
//     MFMA columns instead of 28 of 112; tail lanes are clamped on load and masked on store.  A wave runs two
//     fragments (four independent accumulators) per pass over the 9 taps.
//   * Stride-1 data gradient: the same kernel with src = dy, pads 2 - pt / 2 - pl and wmode = 1 (the filter flipped
//     and transposed inside each group while the fragments are expanded).
//   * Stride-2 data gradient: gather by parity class.  The dx pixels with one (ih & 1, iw & 1) share their taps
//     (ky = (ih + pt) mod 2 (+ 2)), and their dy sources are adjacent pixels of a staged dy row: a fragment is 16
//     same-class dx pixels read at pixel step 1, the four classes are four passes over the staged dy tile
//     (band + 2 rows x tw + 2 columns) with 4, 2, 2 and 1 taps.  Every dx element is stored exactly once.
//   * Weight gradient: per slab and tap a 32 x 32 product over K = pixels.  Both operands are channel-contiguous,
//     so both are read from the staged x / dy tiles with ds_read_b64_tr_b16 (K = 32 pixels per MFMA); only the
//     16 x 16 tiles that hold a group block are computed (4 at Cg = 32, else the 2 diagonal ones: 36 / 18
//     accumulator tiles).  The waves of a block split the 32-pixel steps, a block walks the tiles of its chunk and
//     then adds its four waves in wave order through LDS into one fp32 partial [chunk][tap][C][Cg]
//     (co-major).  mdtf_gconv_wgrad_finalize sums the partials in chunk order in fp64 and stores to, or adds
//     into, the fp32 HWIO destination.  No atomics: bitwise repeatable.
//
// Resource summary (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage): no kernel spills
// (scratch 0 bytes per lane, 0 SGPR / VGPR spills in all of them).
//   gconv_kernel<dense, conv>    VGPR 101  AGPR 24   4 waves / SIMD     gconv_kernel<diag, conv>    VGPR 66  AGPR 24   5
//   gconv_kernel<dense, parity>  VGPR 102  AGPR 24   4                  gconv_kernel<diag, parity>  VGPR 64  AGPR 24   5
//   gconv_wgrad_kernel<dense>    VGPR 78   AGPR 144  2                  gconv_wgrad_kernel<diag>    VGPR 40  AGPR 72   4
//   LDS is dynamic: at most 40 KiB when a band of 2 or more rows fits, never above 64 KiB (wgrad: at least 16 KiB).
//
// Nothing is read back by the host and nothing is allocated: every launch replays inside a captured step.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int kT = 256;
constexpr unsigned kOOB = 0x80000000u;   // buffer offset past num_records -> the load returns zeros
constexpr int kBandMax = 8;              // output rows per block, at most
constexpr int kTileW = 64;               // output columns per block, at most
constexpr int kLdsTarget = 40 * 1024;    // bands grow up to this much LDS
constexpr int kLdsMax = 64 * 1024;
constexpr int kTargetBlocks = 2048;      // fwd / dgrad: images are strided over blocks beyond this many
constexpr int kWgTargetBlocks = 1024;    // wgrad: chunks x slabs

// source plane SH x SW, destination plane DH x DW (forward: x -> y; data gradient: dy -> dx)
struct GcGeo {
  int N, SH, SW, DH, DW, C, lg, S, PT, PL;   // lg = log2(Cg)
};

struct GcPlan {
  int band, tw, bands, ctiles, slabs;   // tile rows / columns, tiles per image, 32-channel slabs
  int rows_in, wps, half;               // staged rows, staged pixels per row, first odd column's position (0: linear)
  int nq, nqd;                          // 16-B chunks of the staged source / dy planes (multiples of kT)
  int lds;
};

template <bool DENSE>
struct Frag {
  typedef v4s type;
};
template <>
struct Frag<true> {
  typedef bf16x8_t type;
};

// Rows [y0, y0 + rows) x columns x0 + {0 .. wps - 1} of one image's 32-channel slab -> a plane of 64-B pixels.
// LDS-DMA writes lane-linear, so the placement is applied to the source address: chunk idx = 4 q + slot of the
// plane holds channel chunk slot ^ ((q >> 2) & 3) of staged pixel q = r wps + j, column x = j (linear) or
// 2 j / 2 (j - half) + 1 (de-interleaved); zeros outside the image and past `rows`.
__device__ __forceinline__ void stage_plane(const bf16_t* img, int img_bytes, char* plane, int nq, int rows, int wps,
                                            int half, int y0, int x0, int SH, int SW, int C, int ch0, int tid,
                                            int wave) {
  const i32x4_t rs = buffer_rsrc(img, img_bytes);
  for (int base = 0; base < nq; base += kT) {
    const int idx = base + tid, q = idx >> 2, slot = idx & 3;
    const int r = q / wps, j = q - r * wps;
    const int x = half ? (j < half ? 2 * j : 2 * (j - half) + 1) : j;
    const int iy = y0 + r, ix = x0 + x;
    const bool ok = r < rows && (unsigned)iy < (unsigned)SH && (unsigned)ix < (unsigned)SW;
    const int c = slot ^ ((q >> 2) & 3);
    const unsigned vo = ok ? ((unsigned)(iy * SW + ix) * (unsigned)C + (unsigned)(ch0 + 8 * c)) * 2u : kOOB;
    dma16_asm(rs, plane + base * 16 + wave * 1024, vo);
  }
}

// The filter entry that couples source channel kin to destination channel mout (both slab-local) at filter tap
// tf, 0 across groups.  tr: the data gradient (the destination is the filter's input channel).
__device__ __forceinline__ short wget(const bf16_t* __restrict__ w, int tf, int kin, int mout, int lg, int C, int ch0,
                                      int tr) {
  if ((kin >> lg) != (mout >> lg)) return 0;
  const int ci = tr ? mout : kin, co = tr ? kin : mout;
  return static_cast<short>(w[((long long)((tf << lg) + (ci & ((1 << lg) - 1)))) * C + ch0 + co]);
}

template <bool DENSE>
__device__ __forceinline__ void load_filter(const bf16_t* __restrict__ w, typename Frag<DENSE>::type (&wf)[9][2],
                                            int lg, int C, int ch0, int tr, int flip, int gq, int li) {
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int tf = flip ? 8 - t : t;
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
      if (tr) {
        // the fragment's k run (source = the filter's output channels) is contiguous in HWIO: one vector load
        const int mout = 16 * ob + li, k0 = DENSE ? 8 * gq : 16 * ob + 4 * gq;
        const bf16_t* p = w + ((long long)((tf << lg) + (mout & ((1 << lg) - 1)))) * C + ch0 + k0;
        if constexpr (DENSE) {
          wf[t][ob] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p));
        } else {
          const uint2 v = (k0 >> lg) == (mout >> lg) ? *reinterpret_cast<const uint2*>(p) : make_uint2(0u, 0u);
          wf[t][ob] = __builtin_bit_cast(v4s, v);
        }
        continue;
      }
      if constexpr (DENSE) {
        short8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = wget(w, tf, 8 * gq + j, 16 * ob + li, lg, C, ch0, tr);
        wf[t][ob] = __builtin_bit_cast(bf16x8_t, v);
      } else {
        v4s v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = wget(w, tf, 16 * ob + 4 * gq + j, 16 * ob + li, lg, C, ch0, tr);
        wf[t][ob] = v;
      }
    }
  }
}

// one tap of one pixel fragment: staged pixel q of this lane, both 16-channel output blocks
template <bool DENSE>
__device__ __forceinline__ void tap_mma(const char* plane, int q, int gq, const typename Frag<DENSE>::type& w0,
                                        const typename Frag<DENSE>::type& w1, float4v& a0, float4v& a1) {
  const int sw = (q >> 2) & 3;
  const char* p = plane + q * 64;
  if constexpr (DENSE) {
    const bf16x8_t b = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p + ((gq ^ sw) << 4)));
    a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, b, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, b, a1, 0, 0, 0);
  } else {
    const int h = (gq & 1) * 8;
    const v4s b0 = *reinterpret_cast<const v4s*>(p + (((gq >> 1) ^ sw) << 4) + h);
    const v4s b1 = *reinterpret_cast<const v4s*>(p + (((2 + (gq >> 1)) ^ sw) << 4) + h);
    a0 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w0, b0, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(w1, b1, a1, 0, 0, 0);
  }
}

// lane (gq, li) holds channels 4 gq .. + 3 of both 16-channel blocks of its pixel: two 8-B stores
__device__ __forceinline__ void store_pixel(bf16_t* p, int gq, const float4v& a0, const float4v& a1) {
  *reinterpret_cast<uint2*>(p + 4 * gq) = make_uint2(pack_bf2(a0[0], a0[1]), pack_bf2(a0[2], a0[3]));
  *reinterpret_cast<uint2*>(p + 16 + 4 * gq) = make_uint2(pack_bf2(a1[0], a1[1]), pack_bf2(a1[2], a1[3]));
}

// MODE 0: the convolution form (forward at stride 1 / 2; stride-1 data gradient with wmode 1).  Tiles run over the
//         destination plane.
// MODE 1: the stride-2 data gradient by parity class.  Tiles run over (ih >> 1, iw >> 1).
template <bool DENSE, int MODE>
__global__ void __launch_bounds__(kT) gconv_kernel(const bf16_t* __restrict__ src, const bf16_t* __restrict__ wgt,
                                                   bf16_t* __restrict__ dst, GcGeo g, GcPlan pl, int wmode) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gq = lane >> 4, li = lane & 15;
  int b = blockIdx.x;
  const int slab = b % pl.slabs;
  b /= pl.slabs;
  const int ct = b % pl.ctiles, bd = b / pl.ctiles;
  const int ch0 = slab * 32;
  const int TH = MODE == 0 ? g.DH : (g.DH + 1) >> 1, TW = MODE == 0 ? g.DW : (g.DW + 1) >> 1;
  const int r0 = bd * pl.band, c0 = ct * pl.tw;
  const int th = min(pl.band, TH - r0), tw = min(pl.tw, TW - c0), P = th * tw;
  const int s = MODE == 0 ? g.S : 1;
  const int y0 = MODE == 0 ? r0 * s - g.PT : r0 - 1, x0 = MODE == 0 ? c0 * s - g.PL : c0 - 1;
  const int rows = MODE == 0 ? (th - 1) * s + 3 : th + 2;
  const int wps = pl.wps;
  const int nfrag = (P + 15) >> 4;

  typename Frag<DENSE>::type wf[9][2];
  load_filter<DENSE>(wgt, wf, g.lg, g.C, ch0, MODE == 1 ? 1 : wmode, MODE == 0 && wmode != 0, gq, li);

  const long long src_img = (long long)g.SH * g.SW * g.C, dst_img = (long long)g.DH * g.DW * g.C;
  for (int n = blockIdx.z; n < g.N; n += gridDim.z) {
    __syncthreads();                                  // every wave is done with the previous image's tile
    stage_plane(src + n * src_img, (int)(src_img * 2), lds, pl.nq, rows, wps, pl.half, y0, x0, g.SH, g.SW, g.C, ch0,
                tid, wave);
    wait_vmcnt<0>();
    __syncthreads();
    bf16_t* dimg = dst + n * dst_img + ch0;

    if constexpr (MODE == 0) {
      for (int f = 2 * wave; f < nfrag; f += 8) {
        int qb[2], pr[2], pc[2];
        bool live[2];
        float4v acc[2][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int p = 16 * (f + u) + li;
          live[u] = p < P;
          const int pcl = live[u] ? p : P - 1;
          pr[u] = pcl / tw;
          pc[u] = pcl - pr[u] * tw;
          qb[u] = pr[u] * s * wps + pc[u];
          acc[u][0] = acc[u][1] = float4v{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int ky = t / 3, kx = t % 3;
          const int toff = ky * wps + (pl.half ? (kx & 1) * pl.half + (kx >> 1) : kx);
#pragma unroll
          for (int u = 0; u < 2; ++u) tap_mma<DENSE>(lds, qb[u] + toff, gq, wf[t][0], wf[t][1], acc[u][0], acc[u][1]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (live[u])
            store_pixel(dimg + ((long long)(r0 + pr[u]) * g.DW + c0 + pc[u]) * g.C, gq, acc[u][0], acc[u][1]);
      }
    } else {
#pragma unroll
      for (int cy = 0; cy < 2; ++cy) {
#pragma unroll
        for (int cx = 0; cx < 2; ++cx) {
          // class (py, px) of dx pixels: the taps are ky = cy (+ 2), kx = cx (+ 2), exact quotients by construction
          const int py = (cy + g.PT) & 1, px = (cx + g.PL) & 1;
          const int ey = py + g.PT, ex = px + g.PL;
          for (int f = 2 * wave; f < nfrag; f += 8) {
            int qb[2], pr[2], pc[2];
            bool live[2];
            float4v acc[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int p = 16 * (f + u) + li;
              live[u] = p < P;
              const int pcl = live[u] ? p : P - 1;
              pr[u] = pcl / tw;
              pc[u] = pcl - pr[u] * tw;
              qb[u] = (pr[u] + 1) * wps + pc[u] + 1;
              acc[u][0] = acc[u][1] = float4v{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ky = cy; ky < 3; ky += 2) {
#pragma unroll
              for (int kx = cx; kx < 3; kx += 2) {
                const int toff = ((ey - ky) >> 1) * wps + ((ex - kx) >> 1);     // each quotient is -1, 0 or 1
#pragma unroll
                for (int u = 0; u < 2; ++u)
                  tap_mma<DENSE>(lds, qb[u] + toff, gq, wf[ky * 3 + kx][0], wf[ky * 3 + kx][1], acc[u][0], acc[u][1]);
              }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int iy = 2 * (r0 + pr[u]) + py, ix = 2 * (c0 + pc[u]) + px;
              if (live[u] && iy < g.DH && ix < g.DW)
                store_pixel(dimg + ((long long)iy * g.DW + ix) * g.C, gq, acc[u][0], acc[u][1]);
            }
          }
        }
      }
    }
  }
}

// one ds_read_b64_tr_b16 pair: the MFMA operand X^T[col0 + (lane & 15)][k = 8 (lane >> 4) + 0 .. 7] from staged pixels
// (k rows) qlo (k + 0 .. 3) / qhi (k + 4 .. 7) of this lane, 16-column block cb of the slab
__device__ __forceinline__ bf16x8_t tr_frag(const char* plane, int qlo, int qhi, int cb, int p4) {
  const int ch = cb * 2 + (p4 >> 1), h = (p4 & 1) * 8;
  const char* a = plane + qlo * 64 + ((ch ^ ((qlo >> 2) & 3)) << 4) + h;
  const char* c = plane + qhi * 64 + ((ch ^ ((qhi >> 2) & 3)) << 4) + h;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)a);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)c);
  const short8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, f);
}

// g: SH x SW = the x plane, DH x DW = the dy plane.  Block = (chunk of `upc` tiles, slab).
template <bool DENSE>
__global__ void __launch_bounds__(kT) gconv_wgrad_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                         float* __restrict__ ws, GcGeo g, GcPlan pl, int upc,
                                                         int nunits) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = DENSE ? 4 : 2;                    // accumulator tiles per tap
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fq = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  const int slab = blockIdx.x % pl.slabs, ck = blockIdx.x / pl.slabs;
  const int ch0 = slab * 32;
  const int wps = pl.wps, s = g.S;
  char* xpl = lds;
  char* dpl = lds + pl.nq * 16;
  const int zq = pl.nqd >> 2;                          // a pixel of zeros behind the dy plane

  float4v acc[9][NT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[t][i] = float4v{0.f, 0.f, 0.f, 0.f};

  const long long x_img = (long long)g.SH * g.SW * g.C, dy_img = (long long)g.DH * g.DW * g.C;
  const int u1 = min(nunits, (ck + 1) * upc);
  for (int u = ck * upc; u < u1; ++u) {
    const int ct = u % pl.ctiles, t2 = u / pl.ctiles;
    const int bd = t2 % pl.bands, n = t2 / pl.bands;
    const int r0 = bd * pl.band, c0 = ct * pl.tw;
    const int th = min(pl.band, g.DH - r0), tw = min(pl.tw, g.DW - c0), P = th * tw;
    __syncthreads();
    stage_plane(x + n * x_img, (int)(x_img * 2), xpl, pl.nq, (th - 1) * s + 3, wps, pl.half, r0 * s - g.PT,
                c0 * s - g.PL, g.SH, g.SW, g.C, ch0, tid, wave);
    stage_plane(dy + n * dy_img, (int)(dy_img * 2), dpl, pl.nqd, th, pl.tw, 0, r0, c0, g.DH, g.DW, g.C, ch0, tid, wave);
    if (tid < 4) reinterpret_cast<uint4*>(dpl + zq * 64)[tid] = make_uint4(0u, 0u, 0u, 0u);
    wait_vmcnt<0>();
    __syncthreads();

    const int nks = (P + 31) >> 5;
    for (int ks = wave; ks < nks; ks += 4) {
      // this lane's two k rows (output pixels); past the tile: dy reads the zero pixel, x any staged pixel
      int qx[2], qd[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int p = 32 * ks + 8 * fq + 4 * h + q4;
        const bool in = p < P;
        const int pcl = in ? p : 0;
        const int r = pcl / tw, c = pcl - r * tw;
        qd[h] = in ? r * pl.tw + c : zq;
        qx[h] = r * s * wps + c;
      }
      bf16x8_t df[2];
#pragma unroll
      for (int cob = 0; cob < 2; ++cob) df[cob] = tr_frag(dpl, qd[0], qd[1], cob, p4);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t % 3;
        const int toff = ky * wps + (pl.half ? (kx & 1) * pl.half + (kx >> 1) : kx);
        bf16x8_t xf[2];
#pragma unroll
        for (int cib = 0; cib < 2; ++cib) xf[cib] = tr_frag(xpl, qx[0] + toff, qx[1] + toff, cib, p4);
        if constexpr (DENSE) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[i >> 1], df[i & 1], acc[t][i], 0, 0, 0);
        } else {
#pragma unroll
          for (int i = 0; i < 2; ++i)
            acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[i], df[i], acc[t][i], 0, 0, 0);
        }
      }
    }
  }

  // the block's four waves, added in wave order, one tap per round; lane (gq, li) of a tile holds input channels
  // 4 gq .. + 3 (rows) of output channel li (column): 4 consecutive floats of the [co][j] partial
  float4* red = reinterpret_cast<float4*>(lds);
  const int Cg = 1 << g.lg;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i)
      red[(wave * NT + i) * 64 + lane] = make_float4(acc[t][i][0], acc[t][i][1], acc[t][i][2], acc[t][i][3]);
    __syncthreads();
    if (wave < NT) {
      float4 sum = red[wave * 64 + lane];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float4 v = red[(w * NT + wave) * 64 + lane];
        sum.x += v.x;
        sum.y += v.y;
        sum.z += v.z;
        sum.w += v.w;
      }
      const int cib = DENSE ? wave >> 1 : wave, cob = DENSE ? wave & 1 : wave;
      const int ci = 16 * cib + 4 * (lane >> 4), co = 16 * cob + (lane & 15);
      if ((ci >> g.lg) == (co >> g.lg))
        *reinterpret_cast<float4*>(ws + ((((long long)ck * 9 + t) * g.C + ch0 + co) << g.lg) + (ci & (Cg - 1))) = sum;
    }
  }
}

// dst [3, 3, Cg, C] (fp32) = (accumulate ? dst : 0) + the partials [chunk][tap][C][Cg] in chunk order, in fp64
__global__ void __launch_bounds__(kT) gconv_wgrad_finalize_kernel(const float* __restrict__ ws, float* __restrict__ dst,
                                                                  int nchunks, int C, int lg, int accumulate) {
  const int e = blockIdx.x * kT + threadIdx.x;
  const int per_tap = C << lg;
  if (e >= 9 * per_tap) return;
  const int t = e / per_tap, r = e - t * per_tap;
  const int j = r / C, co = r - j * C;
  const long long at = (((long long)t * C + co) << lg) + j, stride = 9ll * per_tap;
  double sum = 0.0;
  for (int ck = 0; ck < nchunks; ++ck) sum += static_cast<double>(ws[ck * stride + at]);
  if (accumulate) sum += static_cast<double>(dst[e]);
  dst[e] = static_cast<float>(sum);
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// 0, MDTF_EINVAL (sizes that describe no convolution) or MDTF_EUNSUPPORTED (one the kernels do not take)
int check_geometry(int N, int H, int W, int C, int Cg, int OH, int OW, int KH, int KW, int S, int D, int PT, int PB,
                   int PL, int PR) {
  if (N < 0 || H < 1 || W < 1 || C < 1 || Cg < 1 || C % Cg || OH < 1 || OW < 1) return MDTF_EINVAL;
  if (KH < 1 || KW < 1 || S < 1 || D < 1 || PT < 0 || PB < 0 || PL < 0 || PR < 0) return MDTF_EINVAL;
  const long long eh = (long long)(KH - 1) * D + 1, ew = (long long)(KW - 1) * D + 1;
  const long long fh = (long long)H + PT + PB - eh, fw = (long long)W + PL + PR - ew;
  if (fh < 0 || fw < 0 || fh / S + 1 != OH || fw / S + 1 != OW) return MDTF_EINVAL;
  if (KH != 3 || KW != 3 || D != 1 || S > 2) return MDTF_EUNSUPPORTED;
  if ((Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32) || C % 32) return MDTF_EUNSUPPORTED;
  if (PT > 2 || PB > 2 || PL > 2 || PR > 2) return MDTF_EUNSUPPORTED;
  // one image is one buffer descriptor (byte offsets below 2^31); pixel counts fit an int
  if ((long long)H * W * C >= (1ll << 30) || (long long)N * H * W >= (1ll << 31)) return MDTF_EUNSUPPORTED;
  return 0;
}

inline int log2i(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// Tiles of a TH x TWD plane.  mode 0: the convolution form at stride S; mode 1: the parity form (the staged plane is
// the tile plus one pixel all round).  wgrad: a dy tile and a zero pixel are staged behind the source tile.
bool make_plan(int mode, int TH, int TWD, int C, int S, bool wgrad, GcPlan* pl) {
  pl->slabs = C / 32;
  pl->ctiles = static_cast<int>(ceil_div(TWD, kTileW));
  pl->tw = static_cast<int>(ceil_div(TWD, pl->ctiles));
  pl->half = mode == 0 && S == 2 ? pl->tw + 1 : 0;
  pl->wps = mode == 0 && S == 2 ? 2 * pl->tw + 2 : pl->tw + 2;
  auto rows_in = [&](int b) { return mode == 0 ? (b - 1) * S + 3 : b + 2; };
  auto bytes = [&](int b) {
    return round_up(rows_in(b) * pl->wps * 4, kT) * 16 + (wgrad ? round_up(b * pl->tw * 4, kT) * 16 + 64 : 0);
  };
  int bmax = 1;
  for (int b = 2; b <= kBandMax && b <= TH; ++b)
    if (bytes(b) <= kLdsTarget) bmax = b;
  pl->bands = static_cast<int>(ceil_div(TH, bmax));
  pl->band = static_cast<int>(ceil_div(TH, pl->bands));
  pl->rows_in = rows_in(pl->band);
  pl->nq = round_up(pl->rows_in * pl->wps * 4, kT);
  pl->nqd = wgrad ? round_up(pl->band * pl->tw * 4, kT) : 0;
  pl->lds = bytes(pl->band);
  if (wgrad && pl->lds < 16 * 1024) pl->lds = 16 * 1024;          // the cross-wave reduction's 4 x 4 KiB
  return pl->lds <= kLdsMax && (long long)pl->slabs * pl->ctiles * pl->bands < (1ll << 31);
}

template <int MODE>
int launch_conv(const void* src, const void* w, void* dst, const GcGeo& g, int wmode, hipStream_t st) {
  GcPlan pl;
  const int TH = MODE == 0 ? g.DH : (g.DH + 1) / 2, TWD = MODE == 0 ? g.DW : (g.DW + 1) / 2;
  if (!make_plan(MODE, TH, TWD, g.C, g.S, false, &pl)) return MDTF_EUNSUPPORTED;
  const long long gx = (long long)pl.slabs * pl.ctiles * pl.bands;
  long long gz = ceil_div(kTargetBlocks, gx);
  gz = gz < 1 ? 1 : gz;
  gz = gz > g.N ? g.N : gz;
  gz = gz > 65535 ? 65535 : gz;
  const dim3 grid(static_cast<unsigned>(gx), 1, static_cast<unsigned>(gz));
  const bf16_t* s = static_cast<const bf16_t*>(src);
  const bf16_t* wt = static_cast<const bf16_t*>(w);
  bf16_t* d = static_cast<bf16_t*>(dst);
  if (g.lg == 5)
    hipLaunchKernelGGL((gconv_kernel<true, MODE>), grid, dim3(kT), pl.lds, st, s, wt, d, g, pl, wmode);
  else
    hipLaunchKernelGGL((gconv_kernel<false, MODE>), grid, dim3(kT), pl.lds, st, s, wt, d, g, pl, wmode);
  MDTF_LAUNCH_CHECK();
  return 0;
}

struct WgPlan {
  GcPlan t;
  int upc, nunits, nchunks;   // tiles per chunk, tiles, chunks
};

bool wgrad_plan(int N, int C, int OH, int OW, int S, WgPlan* wp) {
  if (!make_plan(0, OH, OW, C, S, true, &wp->t)) return false;
  const long long nunits = (long long)(N > 0 ? N : 1) * wp->t.bands * wp->t.ctiles;
  if (nunits >= (1ll << 31)) return false;
  long long target = kWgTargetBlocks / wp->t.slabs;
  target = target < 1 ? 1 : target;
  const long long upc = ceil_div(nunits, target);
  wp->upc = static_cast<int>(upc);
  wp->nunits = static_cast<int>(N > 0 ? nunits : 0);
  wp->nchunks = static_cast<int>(ceil_div(nunits, upc));
  return (long long)wp->nchunks * wp->t.slabs < (1ll << 31);
}

// the sizes the queries and the finalize take: no filter or pads, so only what the plan depends on
int check_sizes(int N, int H, int W, int C, int Cg, int OH, int OW, int S) {
  if (N < 0 || H < 1 || W < 1 || C < 1 || Cg < 1 || C % Cg || OH < 1 || OW < 1 || S < 1) return MDTF_EINVAL;
  if ((Cg != 4 && Cg != 8 && Cg != 16 && Cg != 32) || C % 32 || S > 2) return MDTF_EUNSUPPORTED;
  if ((long long)H * W * C >= (1ll << 30) || (long long)N * H * W >= (1ll << 31)) return MDTF_EUNSUPPORTED;
  return 0;
}

}  // namespace

// y = grouped conv2d(x, w): x bf16 [N, H, W, C], w bf16 [3, 3, Cg, C], y bf16 [N, OH, OW, C], contiguous and 16-byte
// aligned; S is the stride and D the dilation of both axes.  OH = (H + PT + PB - (KH - 1) D - 1) / S + 1 and the same
// for OW, or MDTF_EINVAL; a geometry the kernels do not take: MDTF_EUNSUPPORTED (nothing is launched).
MDTF_EXPORT int mdtf_gconv_fwd(const void* x, const void* w, void* y, int N, int H, int W, int C, int Cg, int OH, int OW,
                               int KH, int KW, int S, int D, int PT, int PB, int PL, int PR, hipStream_t st) {
  if (!x || !w || !y || !aligned(x, 16) || !aligned(w, 16) || !aligned(y, 16)) return MDTF_EINVAL;
  const int rc = check_geometry(N, H, W, C, Cg, OH, OW, KH, KW, S, D, PT, PB, PL, PR);
  if (rc != 0) return rc;
  if (N == 0) return 0;
  const GcGeo g{N, H, W, OH, OW, C, log2i(Cg), S, PT, PL};
  return launch_conv<0>(x, w, y, g, 0, st);
}

// dx = the gradient of mdtf_gconv_fwd with respect to x for dy [N, OH, OW, C]; every element of dx is stored
MDTF_EXPORT int mdtf_gconv_dgrad(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int Cg, int OH,
                                 int OW, int KH, int KW, int S, int D, int PT, int PB, int PL, int PR, hipStream_t st) {
  if (!dy || !w || !dx || !aligned(dy, 16) || !aligned(w, 16) || !aligned(dx, 16)) return MDTF_EINVAL;
  const int rc = check_geometry(N, H, W, C, Cg, OH, OW, KH, KW, S, D, PT, PB, PL, PR);
  if (rc != 0) return rc;
  if ((long long)OH * OW * C >= (1ll << 30)) return MDTF_EUNSUPPORTED;
  if (N == 0) return 0;
  if (S == 1) {
    // dx[ih] = sum_ky dy[ih + pt - ky] w[ky]: the forward form over dy with pads 2 - pt and the filter flipped
    const GcGeo g{N, OH, OW, H, W, C, log2i(Cg), 1, 2 - PT, 2 - PL};
    return launch_conv<0>(dy, w, dx, g, 1, st);
  }
  const GcGeo g{N, OH, OW, H, W, C, log2i(Cg), 2, PT, PL};
  return launch_conv<1>(dy, w, dx, g, 1, st);
}

// output rows per block of mdtf_gconv_fwd for these sizes (0: sizes the kernels refuse)
MDTF_EXPORT long long mdtf_gconv_band(int N, int H, int W, int C, int Cg, int OH, int OW, int S) {
  GcPlan pl;
  if (check_sizes(N, H, W, C, Cg, OH, OW, S) != 0 || !make_plan(0, OH, OW, C, S, false, &pl)) return 0;
  return pl.band;
}

// floats of workspace mdtf_gconv_wgrad writes and mdtf_gconv_wgrad_finalize reads: [chunks][9][C][Cg]
MDTF_EXPORT long long mdtf_gconv_wgrad_ws(int N, int H, int W, int C, int Cg, int OH, int OW, int S) {
  WgPlan wp;
  if (check_sizes(N, H, W, C, Cg, OH, OW, S) != 0 || !wgrad_plan(N, C, OH, OW, S, &wp)) return 0;
  return (long long)wp.nchunks * 9 * C * Cg;
}

// output pixels per chunk (one partial each), at most
MDTF_EXPORT long long mdtf_gconv_wgrad_chunk(int N, int H, int W, int C, int Cg, int OH, int OW, int S) {
  WgPlan wp;
  if (check_sizes(N, H, W, C, Cg, OH, OW, S) != 0 || !wgrad_plan(N, C, OH, OW, S, &wp)) return 0;
  return (long long)wp.upc * wp.t.band * wp.t.tw;
}

// phase 1: the per-chunk partial sums of dw into ws (mdtf_gconv_wgrad_ws floats, 16-byte aligned)
MDTF_EXPORT int mdtf_gconv_wgrad(const void* x, const void* dy, float* ws, int N, int H, int W, int C, int Cg, int OH,
                                 int OW, int KH, int KW, int S, int D, int PT, int PB, int PL, int PR, hipStream_t st) {
  if (!x || !dy || !ws || !aligned(x, 16) || !aligned(dy, 16) || !aligned(ws, 16)) return MDTF_EINVAL;
  const int rc = check_geometry(N, H, W, C, Cg, OH, OW, KH, KW, S, D, PT, PB, PL, PR);
  if (rc != 0) return rc;
  WgPlan wp;
  if ((long long)OH * OW * C >= (1ll << 30) || !wgrad_plan(N, C, OH, OW, S, &wp)) return MDTF_EUNSUPPORTED;
  const GcGeo g{N, H, W, OH, OW, C, log2i(Cg), S, PT, PL};
  const dim3 grid(static_cast<unsigned>((long long)wp.nchunks * wp.t.slabs));
  const bf16_t* xs = static_cast<const bf16_t*>(x);
  const bf16_t* ds = static_cast<const bf16_t*>(dy);
  if (g.lg == 5)
    hipLaunchKernelGGL(gconv_wgrad_kernel<true>, grid, dim3(kT), wp.t.lds, st, xs, ds, ws, g, wp.t, wp.upc, wp.nunits);
  else
    hipLaunchKernelGGL(gconv_wgrad_kernel<false>, grid, dim3(kT), wp.t.lds, st, xs, ds, ws, g, wp.t, wp.upc, wp.nunits);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// phase 2: dw [3, 3, Cg, C] (fp32) = (accumulate ? dw : 0) + the partials of ws in chunk order, summed in fp64
MDTF_EXPORT int mdtf_gconv_wgrad_finalize(const float* ws, float* dw, int N, int H, int W, int C, int Cg, int OH, int OW,
                                          int S, int accumulate, hipStream_t st) {
  if (!ws || !dw || !aligned(ws, 16) || !aligned(dw, 4)) return MDTF_EINVAL;
  const int rc = check_sizes(N, H, W, C, Cg, OH, OW, S);
  if (rc != 0) return rc;
  WgPlan wp;
  if (!wgrad_plan(N, C, OH, OW, S, &wp)) return MDTF_EUNSUPPORTED;
  const int total = 9 * C * Cg;
  hipLaunchKernelGGL(gconv_wgrad_finalize_kernel, dim3(static_cast<unsigned>(ceil_div(total, kT))), dim3(kT), 0, st, ws,
                     dw, wp.nchunks, C, log2i(Cg), accumulate != 0);
  MDTF_LAUNCH_CHECK();
  return 0;
}
