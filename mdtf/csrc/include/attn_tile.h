// Device helpers shared by the tiled attention kernels (attention_flash.hip, attention_causal.hip): 128-B-row LDS
// tile images filled by LDS-DMA, the MFMA fragment reads of both orientations, the dropout counter hash and the
// Dq = rowsum(dO * O) kernel.  Everything has internal linkage: each including file gets its own copy.
#pragma once
#include "mdtf_common.h"

using namespace mdtf;

namespace {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

constexpr int NT = 256;   // 4 waves

// 16-B chunk swizzles of 128-B-row images (involutions)
struct SwzA {    // read 16 rows at a time with ds_read_b128
  __device__ static int f(int r, int c) { return c ^ ((r >> 1) & 7); }
};
struct SwzV {    // read transposed, rows {4g+q} / {16+4g+q}
  __device__ static int f(int r, int c) { return c ^ (((r >> 1) & 3) << 1); }
};

__device__ __forceinline__ float4v mfma(const bf16x8_t& a, const bf16x8_t& b, const float4v& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
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

// keep bit of attention-dropout element (bh, q, k) -- the same stream as attention.hip at S = 128
__device__ __forceinline__ bool keep_elem(uint32_t seed, int bh, int S, int q, int k, uint32_t thr) {
  const uint32_t idx = ((uint32_t)bh * S + (uint32_t)q) * S + (uint32_t)k;
  return hash_u32(idx * 0x9E3779B1u ^ seed) >= thr;
}

// DMA rows [r0, r0 + R) x 64 columns (elements col0 .. col0 + 63 of row r at t + (rowbase + r*ld)) into a
// R x 128-B image; NWV waves, one 1-KiB (8-row) piece per wave instruction
template <class SW, int R>
__device__ __forceinline__ void load_tile(const bf16_t* t, int tbytes, long long rowbase, int ld, int col0, char* img,
                                          int wave, int lane) {
#pragma unroll
  for (int jj = 0; jj < R / 32; ++jj) {
    const int j = wave + 4 * jj;                  // 8-row block
    const int r = 8 * j + (lane >> 3);
    const int c = SW::f(r, lane & 7);
    const unsigned voff = (unsigned)((rowbase + (long long)r * ld + col0 + c * 8) * 2);
    dma16(t, tbytes, img + j * 1024, voff, 0);
  }
}

template <class SW>
__device__ __forceinline__ bf16x8_t row_frag(const char* img, int r0, int c0, int lane) {
  const int r = r0 + (lane & 15);
  const int c = c0 + (lane >> 4);
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(img + r * 128 + (SW::f(r, c) << 4)));
}

__device__ __forceinline__ v4s tr4(const char* img, int r, int col) {
  const char* p = img + r * 128 + (SwzV::f(r, col >> 3) << 4) + (col & 7) * 2;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)p);
}

// A operand X^T[col][k] from a [k rows][64 cols] image (SwzV), 32-deep k-step at kb, k order
// {4g..4g+3, 16+4g..16+4g+3} (the order of two stacked 16x16 accumulator tiles used as a B operand)
__device__ __forceinline__ bf16x8_t trp_frag(const char* img, int kb, int col0, int lane) {
  const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p4 = i & 3;
  const v4s lo = tr4(img, kb + 4 * g + q4, col0 + 4 * p4);
  const v4s hi = tr4(img, kb + 16 + 4 * g + q4, col0 + 4 * p4);
  const short8 f = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, f);
}

// two stacked 16x16 fp32 accumulator tiles -> one bf16 B fragment (k order as trp_frag)
__device__ __forceinline__ bf16x8_t pack_acc(const float4v& a0, const float4v& a1) {
  const uint4 w = make_uint4(pack_bf2(a0[0], a0[1]), pack_bf2(a0[2], a0[3]), pack_bf2(a1[0], a1[1]),
                             pack_bf2(a1[2], a1[3]));
  return __builtin_bit_cast(bf16x8_t, w);
}

__device__ __forceinline__ bf16x8_t gfrag(const bf16_t* p) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(p));
}

__device__ __forceinline__ float4 mask4(const float* mask, long long off) {
  return mask ? *reinterpret_cast<const float4*>(mask + off) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// Dq[bh][q] = sum_d dO[q][d] * O[q][d]; one wave per (q, head) row group of 64 elements x 8 rows
__global__ void __launch_bounds__(256) attn_bwd_pre(const bf16_t* __restrict__ out, const bf16_t* __restrict__ dout,
                                                    float* __restrict__ dq, int B, int S, int nh, int D) {
  const long long row = (long long)blockIdx.x * 32 + (threadIdx.x >> 3);   // (b*S + q) * nh + h
  const int sub = threadIdx.x & 7;
  const long long total = (long long)B * S * nh;
  float part = 0.f;
  if (row < total) {
    const long long bq = row / nh;
    const int h = (int)(row - bq * nh);
    const long long base = bq * nh * D + (long long)h * D;
    for (int d = sub * 8; d < D; d += 64) {
      float o8[8], g8[8];
      load_bf8(out + base + d, o8);
      load_bf8(dout + base + d, g8);
#pragma unroll
      for (int e = 0; e < 8; ++e) part += o8[e] * g8[e];
    }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) part += __shfl_xor(part, o, 64);
  if (row < total && sub == 0) {
    const long long bq = row / nh;
    const int h = (int)(row - bq * nh);
    const long long b = bq / S;
    const int q = (int)(bq - b * S);
    dq[(b * nh + h) * S + q] = part;
  }
}

// ---- encoder-decoder attention (attention_cross.hip): Sq queries against Sk keys of another sequence
// keep bit of element (bh, q, k) of a [B*nh, Sq, Sk] probability tensor; with Sq == Sk the stream of keep_elem
__device__ __forceinline__ bool keep_elem_x(uint32_t seed, int bh, int Sq, int Sk, int q, int k, uint32_t thr) {
  const uint32_t idx = ((uint32_t)bh * Sq + (uint32_t)q) * Sk + (uint32_t)k;
  return hash_u32(idx * 0x9E3779B1u ^ seed) >= thr;
}

// number of visible keys of batch item b: kv_len[b] clamped to [0, Sk], Sk without a length buffer.  b is
// block-uniform, so this is one scalar load per block.
__device__ __forceinline__ int kv_length(const int* kv_len, int b, int Sk) {
  return kv_len ? min(max(__builtin_amdgcn_readfirstlane(kv_len[b]), 0), Sk) : Sk;
}

// zero `rows` rows x D bf16 columns at p (row stride ld elements) with 16-B stores, all NT threads of the block
template <int D>
__device__ __forceinline__ void zero_rows(bf16_t* p, int rows, int ld, int tid) {
  constexpr int CH = D / 8;                      // 16-B chunks per row
  for (int c = tid; c < rows * CH; c += NT)
    *reinterpret_cast<uint4*>(p + (long long)(c / CH) * ld + (c % CH) * 8) = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace
