// tf.image on a uint8 NHWC batch: per-image crop boxes and flips drawn on the device, the exact box statistics of
// per_image_standardization, and one fused pass crop / flip / bilinear resize / normalize -> bf16, fp32 or uint8 NHWC.
//
//   params     one thread per image.  r(i, k) = mix((i * 1024 + k) * 0x9E3779B1 ^ s), mix the 32-bit finalizer of the
//              dropout hash (transformer.hip: drop_keep) and s = step_seed(seed, seed_off) as there, so a replayed
//              hipGraph draws anew every step.  k: 0 crop y, 1 crop x, 2 flip, 4 + 4a + {0 area, 1 aspect, 2 y, 3 x}
//              for attempt a of the distorted box.  Offsets are mulhi_u32(r, n) (uniform over [0, n), integers only),
//              flips r >> 31, fractions (r >> 8) * 2^-24.
//   stats      one block per image: S = sum v, Q = sum v^2 over the OH x OW box at (y0, x0), integers (pixels of the
//              box outside the image are 0), then fp64 mean = S / N, adj = max(sqrt(max(Q / N - mean^2, 0)),
//              1 / sqrt(N)); {mean, 1 / adj} as fp32.
//   transform  out[b, y, x, c] = (v - mean) * inv with xs = flip ? OW - 1 - x : x and
//                copy path (bh == OH and bw == OW):  v = src[b, y0 + y, x0 + xs, c], 0 outside the image
//                resize path:  in = (y + o) * sy - o, lo = max(floor(in), 0), hi = min(ceil(in), bh - 1),
//                              t = in - floor(in), the same in x; top = tl + (tr - tl) * tx, bot likewise,
//                              v = top + (bot - top) * ty; every source index is clamped into the image.
//
// Every source byte is fetched by its own index after the bounds test or the clamp, so no box value, row length or
// base alignment can take a load outside the images.  Nothing is read back by the host and nothing is atomic: the
// three launches replay inside a captured step.
#include "mdtf_common.h"

using namespace mdtf;

namespace {

constexpr int kT = 256;
constexpr int kVec = 8;                          // outputs per thread: one 16-byte bf16 store
constexpr int kFlush = 32;                       // stats: 32 * 255^2 < 2^32 by a wide margin (66051 would still fit)

// the finalizer of transformer.hip's drop_keep, and its per-step seed
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint32_t step_seed(uint32_t seed, const long long* seed_off) {
  return seed_off ? seed ^ ((uint32_t)(*seed_off) * 0x85EBCA6Bu) : seed;
}
__device__ __forceinline__ uint32_t draw(uint32_t i, uint32_t k, uint32_t s) {
  return mix32((i * 1024u + k) * 0x9E3779B1u ^ s);
}
__device__ __forceinline__ int below(uint32_t r, int n) { return static_cast<int>(__umulhi(r, static_cast<uint32_t>(n))); }
__device__ __forceinline__ float unit(uint32_t r) { return static_cast<float>(r >> 8) * 5.9604644775390625e-8f; }

enum { kBoxNone = 0, kBoxCrop = 1, kBoxDistorted = 2 };

__global__ void __launch_bounds__(kT) params_kernel(int* __restrict__ boxes, int* __restrict__ flips, int B, int mode,
                                                    int H, int W, int th, int tw, int off, float area_lo,
                                                    float area_hi, float ar_lo, float ar_hi, int max_attempts,
                                                    uint32_t seed, const long long* __restrict__ seed_off) {
#pragma clang fp contract(off)                    // the box sides as written, so the PyTorch expression draws the same
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= B) return;
  const uint32_t s = step_seed(seed, seed_off);
  if (flips) flips[i] = static_cast<int>(draw(i, 2, s) >> 31);
  if (!boxes || mode == kBoxNone) return;
  int y0 = 0, x0 = 0, bh = H, bw = W;
  if (mode == kBoxCrop) {
    bh = th;
    bw = tw;
    y0 = below(draw(i, 0, s), H - th + 1) - off;
    x0 = below(draw(i, 1, s), W - tw + 1) - off;
  } else {
    const float hw = static_cast<float>(H) * static_cast<float>(W);
    for (int a = 0; a < max_attempts; ++a) {
      const uint32_t k = 4u + 4u * a;
      const float area = area_lo + unit(draw(i, k, s)) * (area_hi - area_lo);
      const float ar = ar_lo + unit(draw(i, k + 1, s)) * (ar_hi - ar_lo);
      const float fw = rintf(sqrtf(area * hw * ar)), fh = rintf(sqrtf(area * hw / ar));
      if (fh >= 1.f && fh <= static_cast<float>(H) && fw >= 1.f && fw <= static_cast<float>(W)) {
        bh = static_cast<int>(fh);
        bw = static_cast<int>(fw);
        y0 = below(draw(i, k + 2, s), H - bh + 1);
        x0 = below(draw(i, k + 3, s), W - bw + 1);
        break;
      }
    }
  }
  reinterpret_cast<int4*>(boxes)[i] = make_int4(y0, x0, bh, bw);
}

struct Box {
  int y0, x0, bh, bw;
};

// the image's own box, or the one box every image shares when there are none per image
__device__ __forceinline__ Box load_box(const int* boxes, int b, Box shared) {
  if (!boxes) return shared;
  const int4 q = reinterpret_cast<const int4*>(boxes)[b];
  return Box{q.x, q.y, q.z, q.w};
}

__global__ void __launch_bounds__(kT) stats_kernel(const uint8_t* __restrict__ src, int H, int W, int C,
                                                   const int* __restrict__ boxes, Box shared, int OH, int OW,
                                                   float* __restrict__ stats) {
  __shared__ unsigned long long rs[kT], rq[kT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Box bx = load_box(boxes, b, shared);
  const uint8_t* img = src + (long long)b * H * W * C;
  const int rowc = OW * C;
  const long long n = (long long)OH * rowc;
  unsigned long long S = 0, Q = 0;
  uint32_t s32 = 0, q32 = 0;
  int pending = 0;
  for (long long e = tid; e < n; e += kT) {
    const int y = static_cast<int>(e / rowc), r = static_cast<int>(e - (long long)y * rowc);
    const int x = r / C, c = r - x * C;
    const long long yy = (long long)bx.y0 + y, xx = (long long)bx.x0 + x;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const uint32_t v = img[(yy * W + xx) * C + c];
      s32 += v;
      q32 += v * v;
    }
    if (++pending == kFlush) {
      S += s32;
      Q += q32;
      s32 = q32 = 0;
      pending = 0;
    }
  }
  rs[tid] = S + s32;
  rq[tid] = Q + q32;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      rs[tid] += rs[tid + o];
      rq[tid] += rq[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma clang fp contract(off)                    // Q / N - mean * mean as written: two roundings, as the host mirror
    const double N = static_cast<double>(n);
    const double mean = static_cast<double>(rs[0]) / N;
    const double var = fmax(static_cast<double>(rq[0]) / N - mean * mean, 0.0);
    const double adj = fmax(sqrt(var), 1.0 / sqrt(N));
    stats[2 * b] = static_cast<float>(mean);
    stats[2 * b + 1] = static_cast<float>(1.0 / adj);
  }
}

enum { kOutBf16 = 0, kOutF32 = 1, kOutU8 = 2 };
enum { kMapLegacy = 0, kMapHalfPixel = 1, kMapAlignCorners = 2 };
enum { kScaleNone = 0, kScaleChannel = 1, kScaleImage = 2 };

struct Scale {
  float m0, m1, m2, m3, i0, i1, i2, i3;
};

// one axis of the bilinear mapping: the two source indices (box-relative, then clamped into the image) and the weight
struct Tap {
  int lo, hi;
  float t;
};
__device__ __forceinline__ Tap axis_tap(int o, float scale, float half, int box0, int boxn, int limit) {
  const float in = (static_cast<float>(o) + half) * scale - half;
  const float fl = floorf(in);
  const int lo = max(static_cast<int>(fl), 0), hi = min(static_cast<int>(ceilf(in)), boxn - 1);
  Tap t;
  t.lo = static_cast<int>(min(max((long long)box0 + lo, 0ll), (long long)limit - 1));      // any box: inside the image
  t.hi = static_cast<int>(min(max((long long)box0 + hi, 0ll), (long long)limit - 1));
  t.t = in - fl;
  return t;
}
__device__ __forceinline__ float axis_scale(int boxn, int outn, int mapping) {
  if (mapping == kMapAlignCorners) return outn > 1 ? static_cast<float>(boxn - 1) / static_cast<float>(outn - 1) : 0.f;
  return static_cast<float>(boxn) / static_cast<float>(outn);
}

// Image b owns the flat outputs [b * P, (b + 1) * P), P = OH * OW * C.  A thread owns one group of 8 outputs aligned
// to 8 in the flat index of the whole batch (a 16-byte bf16 store, two for fp32, 8 bytes of uint8); the groups an
// image shares with its neighbours are written element by element by each side.
template <int OUT>
__global__ void __launch_bounds__(kT) transform_kernel(const uint8_t* __restrict__ src, int H, int W, int C,
                                                       const int* __restrict__ boxes, Box shared,
                                                       const int* __restrict__ flips, void* __restrict__ out, int OH, int OW, int mapping,
                                                       int scale_mode, Scale sc, const float* __restrict__ stats,
                                                       int force_copy, int blocks_per_image) {
  const int b = blockIdx.x / blocks_per_image;
  const int rowc = OW * C;
  const int P = OH * rowc;                                    // at most 2^30, as H * W * C (the launcher checks)
  const long long base = (long long)b * P;
  const int lead = static_cast<int>(base & (kVec - 1));
  const int e0 = ((blockIdx.x - b * blocks_per_image) * kT + threadIdx.x) * kVec - lead;      // image-relative
  if (e0 >= P) return;
  const Box bx = load_box(boxes, b, shared);
  const bool flip = flips && flips[b] != 0;
  const bool copy = force_copy || (bx.bh == OH && bx.bw == OW);
  const uint8_t* img = src + (long long)b * H * W * C;
  const float half = mapping == kMapHalfPixel ? 0.5f : 0.f;
  const float sy = axis_scale(bx.bh, OH, mapping), sx = axis_scale(bx.bw, OW, mapping);
  float im = 0.f, ii = 1.f;
  if (scale_mode == kScaleImage) {
    im = stats[2 * b];
    ii = stats[2 * b + 1];
  }

  // (y, x, c) walks the group's elements from max(e0, 0).  Nothing in the loops branches on a lane's own data: an
  // element outside the image (e < 0 or e >= P: never stored) or outside the source is computed from clamped indices.
  // Each path is three straight-line passes (offsets, byte loads, arithmetic), so a thread's 8 or 32 loads are
  // independent and in flight together.
  const int es = max(e0, 0);
  int y = es / rowc;
  const int r = es - y * rowc;
  int x = r / C, c = r - x * C;
  auto advance = [&](int j) {                                 // the elements before the image do not move the walk
    c += e0 + j >= 0 ? 1 : 0;
    const bool endx = c == C;
    c = endx ? 0 : c;
    x += endx ? 1 : 0;
    const bool endy = x == OW;
    x = endy ? 0 : x;
    y += endy ? 1 : 0;
  };
  float v[kVec];
  int ch[kVec];
  if (copy) {                                                 // block-uniform
    int off[kVec];
    bool inside[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const long long yy = (long long)bx.y0 + y, xx = (long long)bx.x0 + (flip ? OW - 1 - x : x);
      inside[j] = yy >= 0 && yy < H && xx >= 0 && xx < W;
      const int yc = static_cast<int>(min(max(yy, 0ll), (long long)H - 1));
      const int xc = static_cast<int>(min(max(xx, 0ll), (long long)W - 1));
      off[j] = (yc * W + xc) * C + c;
      ch[j] = c;
      advance(j);
    }
    uint8_t raw[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) raw[j] = img[off[j]];
#pragma unroll
    for (int j = 0; j < kVec; ++j) v[j] = inside[j] ? static_cast<float>(raw[j]) : 0.f;
  } else {
    int r0[kVec], r1[kVec], c0[kVec], c1[kVec];
    float wx[kVec], wy[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const Tap ty = axis_tap(y, sy, half, bx.y0, bx.bh, H);
      const Tap tx = axis_tap(flip ? OW - 1 - x : x, sx, half, bx.x0, bx.bw, W);
      r0[j] = ty.lo * W * C + c;
      r1[j] = ty.hi * W * C + c;
      c0[j] = tx.lo * C;
      c1[j] = tx.hi * C;
      wx[j] = tx.t;
      wy[j] = ty.t;
      ch[j] = c;
      advance(j);
    }
    uint8_t tl[kVec], tr[kVec], bl[kVec], br[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      tl[j] = img[r0[j] + c0[j]];
      tr[j] = img[r0[j] + c1[j]];
      bl[j] = img[r1[j] + c0[j]];
      br[j] = img[r1[j] + c1[j]];
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const float ftl = tl[j], ftr = tr[j], fbl = bl[j], fbr = br[j];
      const float top = ftl + (ftr - ftl) * wx[j], bot = fbl + (fbr - fbl) * wx[j];
      v[j] = top + (bot - top) * wy[j];
    }
  }
  if (scale_mode == kScaleChannel) {
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      const int k = ch[j];
      const float m = k == 0 ? sc.m0 : k == 1 ? sc.m1 : k == 2 ? sc.m2 : sc.m3;
      const float s = k == 0 ? sc.i0 : k == 1 ? sc.i1 : k == 2 ? sc.i2 : sc.i3;
      v[j] = (v[j] - m) * s;
    }
  } else if (scale_mode == kScaleImage) {
#pragma unroll
    for (int j = 0; j < kVec; ++j) v[j] = (v[j] - im) * ii;
  }

  const long long f0 = base + e0;                             // flat index in the batch: a multiple of 8
  if (e0 >= 0 && e0 + kVec <= P) {
    if constexpr (OUT == kOutBf16) {
      store_bf8(static_cast<bf16_t*>(out) + f0, v);
    } else if constexpr (OUT == kOutF32) {
      float4* o = reinterpret_cast<float4*>(static_cast<float*>(out) + f0);
      o[0] = make_float4(v[0], v[1], v[2], v[3]);
      o[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
      uint32_t w[2] = {0u, 0u};
#pragma unroll
      for (int j = 0; j < kVec; ++j) w[j >> 2] |= static_cast<uint32_t>(v[j]) << (8 * (j & 3));
      *reinterpret_cast<uint2*>(static_cast<uint8_t*>(out) + f0) = make_uint2(w[0], w[1]);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const int e = e0 + j;
    if (e < 0 || e >= P) continue;
    if constexpr (OUT == kOutBf16)
      static_cast<bf16_t*>(out)[f0 + j] = f2bf(v[j]);
    else if constexpr (OUT == kOutF32)
      static_cast<float*>(out)[f0 + j] = v[j];
    else
      static_cast<uint8_t*>(out)[f0 + j] = static_cast<uint8_t>(v[j]);
  }
}

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// boxes (int32 [B, 4] = {y0, x0, bh, bw}, nullable) and flips (int32 [B], nullable) for B images.  mode 1: a th x tw
// box uniformly inside H x W, its offsets moved by -off (H x W is then an image already padded by off); mode 2: the
// distorted box over H x W, at most max_attempts (<= 255) attempts, then the whole image.
MDTF_EXPORT int mdtf_image_params(int* boxes, int* flips, int B, int mode, int H, int W, int th, int tw, int off,
                                  float area_lo, float area_hi, float ar_lo, float ar_hi, int max_attempts,
                                  unsigned seed, const long long* seed_off, hipStream_t st) {
  if (B < 0 || (!boxes && !flips) || (boxes && !aligned(boxes, 16))) return MDTF_EINVAL;
  if (boxes) {
    if (H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return MDTF_EINVAL;
    if (mode == kBoxCrop && (th < 1 || tw < 1 || th > H || tw > W || off < 0)) return MDTF_EINVAL;
    if (mode == kBoxDistorted && (max_attempts < 1 || max_attempts > 255 || !(area_lo > 0.f) || area_hi < area_lo ||
                                  !(ar_lo > 0.f) || ar_hi < ar_lo))
      return MDTF_EINVAL;
    if (mode != kBoxCrop && mode != kBoxDistorted) return MDTF_EINVAL;
  }
  if (B == 0) return 0;
  hipLaunchKernelGGL(params_kernel, dim3(static_cast<unsigned>(ceil_div(B, kT))), dim3(kT), 0, st, boxes, flips, B,
                     boxes ? mode : kBoxNone, H, W, th, tw, off, area_lo, area_hi, ar_lo, ar_hi, max_attempts, seed,
                     seed_off);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// stats (fp32 [B, 2] = {mean, 1 / adjusted stddev}) of the OH x OW box of every image; boxes nullable: every image
// then takes the box at (y0, x0)
MDTF_EXPORT int mdtf_image_stats(const void* images, int B, int H, int W, int C, const int* boxes, int y0, int x0,
                                 int OH, int OW, float* stats, hipStream_t st) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || C > 4 || OH < 1 || OW < 1) return MDTF_EINVAL;
  if ((long long)OW * C >= (1ll << 31) || (boxes && !aligned(boxes, 16))) return MDTF_EINVAL;
  if (B == 0) return 0;
  if (!images || !stats) return MDTF_EINVAL;
  hipLaunchKernelGGL(stats_kernel, dim3(B), dim3(kT), 0, st, static_cast<const uint8_t*>(images), H, W, C, boxes,
                     Box{y0, x0, OH, OW}, OH, OW, stats);
  MDTF_LAUNCH_CHECK();
  return 0;
}

// The fused pass.  images: uint8 [B, H, W, C] contiguous, any base alignment.  out: [B, OH, OW, C] contiguous, 16-byte
// aligned; boxes nullable: every image then takes the box {y0, x0, bh, bw}; out_dtype 0 bf16, 1 fp32, 2 uint8 (identity scale only; every image then takes the copy path, as with
// per-image stats).  mean_inv: 8 host floats {mean[4], inv[4]} for scale_mode 1.
MDTF_EXPORT int mdtf_image_transform(const void* images, int B, int H, int W, int C, const int* boxes, int y0,
                                     int x0, int bh, int bw, const int* flips, void* out, int out_dtype, int OH, int OW, int mapping,
                                     int scale_mode, const float* mean_inv, const float* stats, hipStream_t st) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || C > 4 || OH < 1 || OW < 1) return MDTF_EINVAL;
  if (out_dtype < kOutBf16 || out_dtype > kOutU8 || mapping < kMapLegacy || mapping > kMapAlignCorners ||
      scale_mode < kScaleNone || scale_mode > kScaleImage)
    return MDTF_EINVAL;
  if (out_dtype == kOutU8 && scale_mode != kScaleNone) return MDTF_EINVAL;
  if ((scale_mode == kScaleChannel && !mean_inv) || (scale_mode == kScaleImage && !stats)) return MDTF_EINVAL;
  const long long P = (long long)OH * OW * C;
  if ((long long)H * W * C > (1ll << 30) || P > (1ll << 30)) return MDTF_EUNSUPPORTED;     // one image: 32-bit offsets
  if (B == 0) return 0;
  if (!images || !out || !aligned(out, 16) || (boxes && !aligned(boxes, 16))) return MDTF_EINVAL;
  const long long bpi = ceil_div((P + 2 * (kVec - 1)) / kVec, kT);      // ceil((lead + P) / 8) groups for any lead
  if (bpi * B >= (1ll << 31)) return MDTF_EINVAL;
  Scale sc = {0.f, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.f};
  if (scale_mode == kScaleChannel)
    sc = Scale{mean_inv[0], mean_inv[1], mean_inv[2], mean_inv[3], mean_inv[4], mean_inv[5], mean_inv[6], mean_inv[7]};
  const int force_copy = out_dtype == kOutU8 || scale_mode == kScaleImage;
  const dim3 grid(static_cast<unsigned>(bpi * B));
  const uint8_t* s8 = static_cast<const uint8_t*>(images);
  const int ibpi = static_cast<int>(bpi);
  const Box shared = {y0, x0, bh, bw};
#define MDTF_IMAGE_LAUNCH(OUT)                                                                                       \
  hipLaunchKernelGGL(transform_kernel<OUT>, grid, dim3(kT), 0, st, s8, H, W, C, boxes, shared, flips, out, OH, OW,   \
                     mapping, scale_mode, sc, stats, force_copy, ibpi)
  if (out_dtype == kOutBf16)
    MDTF_IMAGE_LAUNCH(kOutBf16);
  else if (out_dtype == kOutF32)
    MDTF_IMAGE_LAUNCH(kOutF32);
  else
    MDTF_IMAGE_LAUNCH(kOutU8);
#undef MDTF_IMAGE_LAUNCH
  MDTF_LAUNCH_CHECK();
  return 0;
}
