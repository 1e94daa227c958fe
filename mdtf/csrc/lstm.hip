// LSTM recurrence (TF LSTMCell / BasicLSTMCell, gate order i, j, f, o) for gfx950: one launch per time step, the
// whole cell update in the epilogue of a skinny MFMA GEMM.  bf16 activations and weights, fp32 accumulation and cell
// state.  ops/rnn.py is the caller; the input half (x @ kernel[:I] + bias over all T * B rows), the weight gradients
// and dx are ordinary GEMMs and stay on the dense routes.
//
//   [i j f o] = xg_t + h_{t-1} @ kernel[I:]                       kernel [I + H, 4H]
//   c_t = c_{t-1} * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)
//   h_t = tanh(c_t) * sigmoid(o)
//
// Work split.  A block owns U hidden units (16 or 32) of one 16-row batch tile and computes the four gate strips of
// those units, so a lane's accumulators hold i, j, f, o of the same (row, unit) in matching slots and the cell update
// needs no exchange between gates.  The batch is small (16..256 rows), so the tiles are small and K is split over the
// block's four waves in interleaved 32-wide steps; the four partial tiles meet in LDS and are summed in wave order
// (fixed, so bitwise repeatable).  Each wave then runs the epilogue of a quarter of the tile's rows.
//
// Operands.  Both MFMA operands are 16-byte K-contiguous vectors loaded straight into VGPRs through a two-slot
// register ring (the load of step s + 2 is issued when step s is consumed): h_{t-1} is K-contiguous as it is, and
// lstm_pack_w repacks kernel[I:] once per forward call into wt[H / U][4][U][H], the four gate strips of a unit slice
// adjacent.  The backward's prologue GEMM dG_{t+1} @ kernel[I + slice, :]^T (K = 4H) reads both operands in their
// natural layouts.  No LDS staging, no transposed reads.
//
// No kernel spans time steps, no block waits for another, no float atomics: every (row, unit) of the state and of the
// carried cell gradient has exactly one owner lane in exactly one block per launch.
//
// lstm_step_fwd / lstm_step_bwd run full-length, forward-in-time sequences (mdtf_lstm_fwd / mdtf_lstm_bwd);
// lstm_seq_fwd / lstm_seq_bwd further down add per-row lengths, the reverse direction and two directions per launch
// (mdtf_lstm_fwd_seq / mdtf_lstm_bwd_seq) on the same GEMM, reduction and cell arithmetic.
#include "rnn_tile.h"

namespace {

// kernel[I:] ([H, 4H], k-major) -> wt[H / U][4][U][H] (K-contiguous): 32 x 32 tiles through LDS, both sides coalesced
__global__ __launch_bounds__(256) void lstm_pack_w(const bf16_t* __restrict__ wh, bf16_t* __restrict__ wt, int H,
                                                   int U) {
  __shared__ bf16_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[ty + 8 * r][tx] = wh[static_cast<int64_t>(k0 + ty + 8 * r) * (4 * H) + n0 + tx];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = n0 + ty + 8 * r;
    const int g = col / H, unit = col - g * H;
    const int s = unit / U, u = unit - s * U;
    wt[(static_cast<int64_t>(s * 4 + g) * U + u) * H + k0 + tx] = tile[tx][ty + 8 * r];
  }
}

struct FwdArgs {
  const bf16_t* xg;      // [B, 4H] of this step
  const bf16_t* wt;      // packed recurrent weights
  const bf16_t* h_prev;  // [B, H]
  const float* c_prev;   // [B, H]
  bf16_t* h;             // [B, H]
  float* c;              // [B, H]
  bf16_t* gates;         // [B, 4H], post-activation i, j, f, o
  int B, H;
  float forget_bias;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void lstm_step_fwd(FwdArgs a) {
  constexpr int NT = U / 16, NB = 4 * NT;          // strip g * NT + nt: gate g, units nt * 16 .. + 15 of the slice
  __shared__ float red[kWaves * NB * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float4v acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
  const int arow = row0 + lr;
  const bool a_ok = arow < a.B;
  const bf16_t* a_lane = a.h_prev + static_cast<int64_t>(a_ok ? arow : 0) * H + lk;
  const bf16_t* b_lane = a.wt + (static_cast<int64_t>(slice) * 4 * U + lr) * H + lk;
  skinny_gemm<NB>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);

  float pre[NB];
  reduce_waves<NB>(red, acc, wave, lane, pre);

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 4 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    const float pi = pre[0 * NT + nt] + bf2f(a.xg[g0]);
    const float pj = pre[1 * NT + nt] + bf2f(a.xg[g0 + H]);
    const float pf = pre[2 * NT + nt] + bf2f(a.xg[g0 + 2 * H]) + a.forget_bias;
    const float po = pre[3 * NT + nt] + bf2f(a.xg[g0 + 3 * H]);
    const float gi = sigmoid_fast(pi), gj = tanh_fast(pj), gf = sigmoid_fast(pf), go = sigmoid_fast(po);
    const float c = a.c_prev[s0] * gf + gi * gj;
    a.c[s0] = c;
    a.h[s0] = f2bf(tanh_fast(c) * go);
    a.gates[g0] = f2bf(gi);
    a.gates[g0 + H] = f2bf(gj);
    a.gates[g0 + 2 * H] = f2bf(gf);
    a.gates[g0 + 3 * H] = f2bf(go);
  }
}

struct BwdArgs {
  const bf16_t* dg_next;  // dG[t + 1] [B, 4H], null: no prologue GEMM (t = T - 1)
  const bf16_t* wh;       // kernel[I:] [H, 4H]
  const bf16_t* gates;    // gates[t] [B, 4H], null: GEMM only (the dh0 launch)
  const float* c;         // cs[t]
  const float* c_prev;    // cs[t - 1] or c0
  const bf16_t* dh_out;   // dhs[t] [B, H]
  const bf16_t* dh_last;  // the final state's dh, added at t = T - 1 (else null)
  float* dc_carry;        // [B, H] fp32, in place: in dL/dc_t from later steps, out dL/dc_{t-1}
  bf16_t* dg;             // dG[t] [B, 4H]
  bf16_t* dh0;            // the GEMM-only launch's output [B, H]
  int B, H;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void lstm_step_bwd(BwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float dhr[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dhr[nt] = 0.f;
  if (a.dg_next != nullptr) {                      // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const int arow = row0 + lr;
    const bool a_ok = arow < a.B;
    const bf16_t* a_lane = a.dg_next + static_cast<int64_t>(a_ok ? arow : 0) * 4 * H + lk;
    const bf16_t* b_lane = a.wh + static_cast<int64_t>(slice * U + lr) * 4 * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * 4 * H, 4 * H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, dhr);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 4 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (a.gates == nullptr) {
      a.dh0[s0] = f2bf(dhr[nt]);
      continue;
    }
    float dh = dhr[nt] + bf2f(a.dh_out[s0]);
    if (a.dh_last != nullptr) dh += bf2f(a.dh_last[s0]);
    const float gi = bf2f(a.gates[g0]), gj = bf2f(a.gates[g0 + H]);
    const float gf = bf2f(a.gates[g0 + 2 * H]), go = bf2f(a.gates[g0 + 3 * H]);
    const float tc = tanh_fast(a.c[s0]);
    const float dc = a.dc_carry[s0] + dh * go * (1.0f - tc * tc);
    a.dg[g0] = f2bf(dc * gj * gi * (1.0f - gi));
    a.dg[g0 + H] = f2bf(dc * gi * (1.0f - gj * gj));
    a.dg[g0 + 2 * H] = f2bf(dc * a.c_prev[s0] * gf * (1.0f - gf));
    a.dg[g0 + 3 * H] = f2bf(dh * tc * go * (1.0f - go));
    a.dc_carry[s0] = dc * gf;
  }
}

// ---- per-row lengths and direction (tf.nn.dynamic_rnn(sequence_length=), bidirectional_dynamic_rnn) ----------------
//
// Row b is live at step t iff t < len[b]; a dead row emits zeros and keeps (h, c).  A reverse direction visits
// t = T - 1 .. 0 under the same rule (TF's reverse_sequence -> LSTM -> reverse_sequence without reversing anything):
// its padding steps come first and leave the initial state in place.  The state is never copied: the A operand of
// skinny_gemm is per lane (a lane owns row l % 16), so each row reads hs[previously visited step], or h0 where it was
// not live there, and a dead row is read as zeros.  A 16-row tile with no live row skips the GEMM (the test is the
// same in every wave: a wave's lanes cover all 16 rows) and only writes zeros.  blockIdx.z is the direction; launch s
// runs step s of a forward direction and step T - 1 - s of a reverse one.  `lens` is read here and nowhere on the
// host; null: every row has length T.

constexpr int kDirs = 2;

__device__ __forceinline__ int row_len(const int* lens, int row, int T) {
  return lens != nullptr ? min(max(lens[row], 0), T) : T;
}

struct SeqFwdDir {
  const bf16_t* xg;      // [T, B, ldx] (this direction's 4H columns of the input half)
  const bf16_t* wt;      // packed recurrent weights
  const bf16_t* h0;      // [B, H]
  const float* c0;       // [B, H]
  bf16_t* hs;            // [T, B, H], zeros at dead (t, b)
  float* cs;             // [T, B, H], written at live (t, b) only
  bf16_t* gates;         // [T, B, 4H], written at live (t, b) only
  bf16_t* h_fin;         // [B, H]: the state after the row's last visited live step (h0 / c0 for length 0)
  float* c_fin;
  int reverse;
};

struct SeqFwdArgs {
  SeqFwdDir d[kDirs];
  const int* lens;       // [B] or null
  int s, T, B, H, ldx;
  float forget_bias;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void lstm_seq_fwd(SeqFwdArgs a) {
  constexpr int NT = U / 16, NB = 4 * NT;
  __shared__ float red[kWaves * NB * 4 * kWave];
  const SeqFwdDir& d = a.d[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;
  const bool rev = d.reverse != 0;
  const int t = rev ? a.T - 1 - a.s : a.s, tp = rev ? t + 1 : t - 1;     // tp: the step visited before this one
  const int64_t sh = static_cast<int64_t>(a.B) * H;

  const int arow = row0 + lr;
  bool a_ok = false;
  const bf16_t* a_lane = d.h0 + lk;
  if (arow < a.B) {
    const int len = row_len(a.lens, arow, a.T);
    a_ok = t < len;
    const bool first = rev ? t + 1 >= len : t == 0;
    a_lane = (first ? d.h0 : d.hs + tp * sh) + static_cast<int64_t>(arow) * H + lk;
  }
  float pre[NB];
  if (__ballot(a_ok) != 0) {                       // block-uniform: some row of the tile is live
    float4v acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const bf16_t* b_lane = d.wt + (static_cast<int64_t>(slice) * 4 * U + lr) * H + lk;
    skinny_gemm<NB>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);
    reduce_waves<NB>(red, acc, wave, lane, pre);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0, last = rev ? t == 0 : t + 1 == len;
  const float* c_prev = first ? d.c0 : d.cs + tp * sh;
  const bf16_t* xg = d.xg + (static_cast<int64_t>(t) * a.B + row) * a.ldx;
  bf16_t* h_out = d.hs + t * sh;
  float* c_out = d.cs + t * sh;
  bf16_t* gates = d.gates + t * 4 * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 4 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (!live) {
      h_out[s0] = f2bf(0.f);
      if (len == 0 && a.s == 0) {
        d.h_fin[s0] = d.h0[s0];
        d.c_fin[s0] = d.c0[s0];
      }
      continue;
    }
    const float pi = pre[0 * NT + nt] + bf2f(xg[unit]);
    const float pj = pre[1 * NT + nt] + bf2f(xg[unit + H]);
    const float pf = pre[2 * NT + nt] + bf2f(xg[unit + 2 * H]) + a.forget_bias;
    const float po = pre[3 * NT + nt] + bf2f(xg[unit + 3 * H]);
    const float gi = sigmoid_fast(pi), gj = tanh_fast(pj), gf = sigmoid_fast(pf), go = sigmoid_fast(po);
    const float c = c_prev[s0] * gf + gi * gj;
    const bf16_t h = f2bf(tanh_fast(c) * go);
    c_out[s0] = c;
    h_out[s0] = h;
    gates[g0] = f2bf(gi);
    gates[g0 + H] = f2bf(gj);
    gates[g0 + 2 * H] = f2bf(gf);
    gates[g0 + 3 * H] = f2bf(go);
    if (last) {
      d.h_fin[s0] = h;
      d.c_fin[s0] = c;
    }
  }
}

struct SeqBwdDir {
  const bf16_t* wh;       // kernel[I:] [H, 4H]
  const bf16_t* gates;    // [T, B, 4H]
  const float* cs;        // [T, B, H]
  const float* c0;        // [B, H]
  const bf16_t* dhs;      // [T, B, H]
  const bf16_t* dh_last;  // the final state's dh [B, H] or null: added at the row's last visited live step
  float* dc_carry;        // [B, H] fp32, in place; a dead row leaves it alone, which carries dL/dc_T to its last step
  bf16_t* dg;             // dG [T, B, 4H], zeros at dead (t, b)
  bf16_t* dh0;            // [B, H]
  int reverse;
};

struct SeqBwdArgs {
  SeqBwdDir d[kDirs];
  const int* lens;
  int s, T, B, H;         // s = T: the GEMM-only launch for dh0
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void lstm_seq_bwd(SeqBwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const SeqBwdDir& d = a.d[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;
  const bool rev = d.reverse != 0, fin = a.s == a.T;
  // the forward visited tp, t, tn in this order; this pass has written dG[tn] and writes dG[t]
  const int t = rev ? a.s : a.T - 1 - a.s, tp = rev ? t + 1 : t - 1, tn = rev ? t - 1 : t + 1;
  const int64_t sh = static_cast<int64_t>(a.B) * H;

  const int arow = row0 + lr;
  bool a_ok = false;
  const bf16_t* a_lane = d.dg + lk;
  if (arow < a.B) {
    const int len = row_len(a.lens, arow, a.T);
    // dh0 reads dG of the row's first visited live step; a step reads dG[tn] where the row was live at tn
    a_ok = fin ? len > 0 : t < len && (rev ? t > 0 : t + 1 < len);
    const int src = fin ? (rev ? len - 1 : 0) : tn;
    if (a_ok) a_lane = d.dg + (src * sh + static_cast<int64_t>(arow) * H) * 4 + lk;
  }
  float dhr[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dhr[nt] = 0.f;
  if (__ballot(a_ok) != 0) {                       // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const bf16_t* b_lane = d.wh + static_cast<int64_t>(slice * U + lr) * 4 * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * 4 * H, 4 * H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, dhr);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0, last = rev ? t == 0 : t + 1 == len;
  // (the dh0 launch dereferences none of these)
  const bf16_t* gates = d.gates + t * 4 * sh;
  const float* c_cur = d.cs + t * sh;
  const float* c_prev = first ? d.c0 : d.cs + tp * sh;
  const bf16_t* dh_out = d.dhs + t * sh;
  bf16_t* dg = d.dg + t * 4 * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 4 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (fin) {
      float v = dhr[nt];
      if (len == 0 && d.dh_last != nullptr) v += bf2f(d.dh_last[s0]);
      d.dh0[s0] = f2bf(v);
      continue;
    }
    if (!live) {
      dg[g0] = dg[g0 + H] = dg[g0 + 2 * H] = dg[g0 + 3 * H] = f2bf(0.f);
      continue;
    }
    float dh = dhr[nt] + bf2f(dh_out[s0]);
    if (last && d.dh_last != nullptr) dh += bf2f(d.dh_last[s0]);
    const float gi = bf2f(gates[g0]), gj = bf2f(gates[g0 + H]);
    const float gf = bf2f(gates[g0 + 2 * H]), go = bf2f(gates[g0 + 3 * H]);
    const float tc = tanh_fast(c_cur[s0]);
    const float dc = d.dc_carry[s0] + dh * go * (1.0f - tc * tc);
    dg[g0] = f2bf(dc * gj * gi * (1.0f - gi));
    dg[g0 + H] = f2bf(dc * gi * (1.0f - gj * gj));
    dg[g0 + 2 * H] = f2bf(dc * c_prev[s0] * gf * (1.0f - gf));
    dg[g0 + 3 * H] = f2bf(dh * tc * go * (1.0f - go));
    d.dc_carry[s0] = dc * gf;
  }
}

constexpr int kBf16 = 0;       // the dtype code of the entry points (1: fp32, refused)

// hidden units per block: 32 where that still gives every CU of the device a block, else 16
int pick_u(int B, int H) {
  const int64_t tiles = ceil_div(B, kRows);
  return tiles * (H / 32) >= 256 ? 32 : 16;
}

bool supported(int T, int B, int H, int dtype) {
  return dtype == kBf16 && T >= 1 && B >= 1 && H >= 32 && H % 32 == 0 && static_cast<int64_t>(B) * 4 * H < (1LL << 31) &&
         ceil_div(B, kRows) <= 65535;
}

}  // namespace

// Units per block the step kernels use for this problem (16 or 32); 0 where the entry points refuse it.
MDTF_EXPORT int mdtf_lstm_units(int T, int B, int H, int dtype) { return supported(T, B, H, dtype) ? pick_u(B, H) : 0; }

// The recurrence over t = 0 .. T - 1: one pack launch and T step launches on `st`.  xg [T, B, 4H] bf16 (input half,
// bias included), wh = kernel[I:] [H, 4H] bf16, wt: workspace of 4 * H * H bf16, h0 [B, H] bf16, c0 [B, H] fp32;
// out: hs [T, B, H] bf16, cs [T, B, H] fp32, gates [T, B, 4H] bf16.  Every pointer 16-byte aligned.
MDTF_EXPORT int mdtf_lstm_fwd(const void* xg, const void* wh, void* wt, const void* h0, const float* c0, void* hs,
                              float* cs, void* gates, int T, int B, int H, float forget_bias, int dtype,
                              hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!xg || !wh || !wt || !h0 || !c0 || !hs || !cs || !gates) return MDTF_EINVAL;
  const int U = pick_u(B, H);
  lstm_pack_w<<<dim3(4 * H / 32, H / 32), 256, 0, st>>>(static_cast<const bf16_t*>(wh), static_cast<bf16_t*>(wt), H, U);
  MDTF_LAUNCH_CHECK();
  const int64_t sh = static_cast<int64_t>(B) * H;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)));
  for (int t = 0; t < T; ++t) {
    FwdArgs a;
    a.xg = static_cast<const bf16_t*>(xg) + t * 4 * sh;
    a.wt = static_cast<const bf16_t*>(wt);
    a.h_prev = t ? static_cast<const bf16_t*>(hs) + (t - 1) * sh : static_cast<const bf16_t*>(h0);
    a.c_prev = t ? cs + (t - 1) * sh : c0;
    a.h = static_cast<bf16_t*>(hs) + t * sh;
    a.c = cs + t * sh;
    a.gates = static_cast<bf16_t*>(gates) + t * 4 * sh;
    a.B = B;
    a.H = H;
    a.forget_bias = forget_bias;
    if (U == 32)
      lstm_step_fwd<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      lstm_step_fwd<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// The recurrence backwards, t = T - 1 .. 0, then the GEMM-only launch for dh0: T + 1 launches on `st`.
// wh = kernel[I:] [H, 4H] bf16; gates, cs, c0 as the forward left them; dhs [T, B, H] bf16; dh_last [B, H] bf16 or
// null; dc_carry [B, H] fp32 holds dL/dc_T on entry and dL/dc_0 on return; out: dg [T, B, 4H] bf16, dh0 [B, H] bf16.
MDTF_EXPORT int mdtf_lstm_bwd(const void* wh, const void* gates, const float* cs, const float* c0, const void* dhs,
                              const void* dh_last, float* dc_carry, void* dg, void* dh0, int T, int B, int H,
                              int dtype, hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!wh || !gates || !cs || !c0 || !dhs || !dc_carry || !dg || !dh0) return MDTF_EINVAL;
  const int U = pick_u(B, H);
  const int64_t sh = static_cast<int64_t>(B) * H;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)));
  for (int t = T - 1; t >= -1; --t) {
    BwdArgs a;
    a.dg_next = t < T - 1 ? static_cast<const bf16_t*>(dg) + (t + 1) * 4 * sh : nullptr;
    a.wh = static_cast<const bf16_t*>(wh);
    a.gates = t >= 0 ? static_cast<const bf16_t*>(gates) + t * 4 * sh : nullptr;
    a.c = t >= 0 ? cs + t * sh : nullptr;
    a.c_prev = t > 0 ? cs + (t - 1) * sh : c0;
    a.dh_out = t >= 0 ? static_cast<const bf16_t*>(dhs) + t * sh : nullptr;
    a.dh_last = t == T - 1 ? static_cast<const bf16_t*>(dh_last) : nullptr;
    a.dc_carry = dc_carry;
    a.dg = t >= 0 ? static_cast<bf16_t*>(dg) + t * 4 * sh : nullptr;
    a.dh0 = static_cast<bf16_t*>(dh0);
    a.B = B;
    a.H = H;
    if (U == 32)
      lstm_step_bwd<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      lstm_step_bwd<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// The length- and direction-aware recurrence of `ndir` (1 or 2) independent LSTMs over the same T, B, H and the same
// lengths, every step of all of them in one launch: ndir pack launches and T step launches on `st`.  Bit d of
// `reverse`: direction d visits t = T - 1 .. 0.  `lens`: int32 [B] on the device (clamped to [0, T], never read by
// the host) or null.  `tab` (host memory, read before the call returns) holds 10 pointers per direction, in the order
// xg, wh, wt, h0, c0, hs, cs, gates, h_fin, c_fin: as mdtf_lstm_fwd, except that xg rows are `ldx` elements apart (the
// directions may be column ranges of one [T * B, ndir * 4H] product) and that h_fin [B, H] bf16 / c_fin [B, H] fp32
// receive the final state.  hs is zero at dead (t, b); cs and gates are left unwritten there.
MDTF_EXPORT int mdtf_lstm_fwd_seq(const void* const* tab, int ndir, int reverse, const int* lens, int T, int B, int H,
                                  int ldx, float forget_bias, int dtype, hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!tab || ndir < 1 || ndir > kDirs || ldx < 4 * H || ldx % 8) return MDTF_EINVAL;
  for (int i = 0; i < 10 * ndir; ++i)
    if (!tab[i]) return MDTF_EINVAL;
  const int U = pick_u(B, H);
  SeqFwdArgs a;
  for (int d = 0; d < kDirs; ++d) {
    const void* const* p = tab + 10 * (d < ndir ? d : 0);     // (an unused slot repeats direction 0; no block reads it)
    if (d < ndir) {
      lstm_pack_w<<<dim3(4 * H / 32, H / 32), 256, 0, st>>>(static_cast<const bf16_t*>(p[1]),
                                                           static_cast<bf16_t*>(const_cast<void*>(p[2])), H, U);
      MDTF_LAUNCH_CHECK();
    }
    SeqFwdDir& q = a.d[d];
    q.xg = static_cast<const bf16_t*>(p[0]);
    q.wt = static_cast<const bf16_t*>(p[2]);
    q.h0 = static_cast<const bf16_t*>(p[3]);
    q.c0 = static_cast<const float*>(p[4]);
    q.hs = static_cast<bf16_t*>(const_cast<void*>(p[5]));
    q.cs = static_cast<float*>(const_cast<void*>(p[6]));
    q.gates = static_cast<bf16_t*>(const_cast<void*>(p[7]));
    q.h_fin = static_cast<bf16_t*>(const_cast<void*>(p[8]));
    q.c_fin = static_cast<float*>(const_cast<void*>(p[9]));
    q.reverse = (reverse >> d) & 1;
  }
  a.lens = lens;
  a.T = T;
  a.B = B;
  a.H = H;
  a.ldx = ldx;
  a.forget_bias = forget_bias;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)), ndir);
  for (a.s = 0; a.s < T; ++a.s) {
    if (U == 32)
      lstm_seq_fwd<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      lstm_seq_fwd<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// Its backward: T + 1 launches on `st`, the last one the GEMM-only launch for dh0.  `tab`: 9 pointers per direction,
// in the order wh, gates, cs, c0, dhs, dh_last (may be null), dc_carry, dg, dh0, as mdtf_lstm_bwd.  dg is zero at dead
// (t, b); dc_carry of a row of length 0 is returned as it came, and its dh0 is dh_last.
MDTF_EXPORT int mdtf_lstm_bwd_seq(const void* const* tab, int ndir, int reverse, const int* lens, int T, int B, int H,
                                  int dtype, hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!tab || ndir < 1 || ndir > kDirs) return MDTF_EINVAL;
  for (int i = 0; i < 9 * ndir; ++i)
    if (!tab[i] && i % 9 != 5) return MDTF_EINVAL;
  const int U = pick_u(B, H);
  SeqBwdArgs a;
  for (int d = 0; d < kDirs; ++d) {
    const void* const* p = tab + 9 * (d < ndir ? d : 0);
    SeqBwdDir& q = a.d[d];
    q.wh = static_cast<const bf16_t*>(p[0]);
    q.gates = static_cast<const bf16_t*>(p[1]);
    q.cs = static_cast<const float*>(p[2]);
    q.c0 = static_cast<const float*>(p[3]);
    q.dhs = static_cast<const bf16_t*>(p[4]);
    q.dh_last = static_cast<const bf16_t*>(p[5]);
    q.dc_carry = static_cast<float*>(const_cast<void*>(p[6]));
    q.dg = static_cast<bf16_t*>(const_cast<void*>(p[7]));
    q.dh0 = static_cast<bf16_t*>(const_cast<void*>(p[8]));
    q.reverse = (reverse >> d) & 1;
  }
  a.lens = lens;
  a.T = T;
  a.B = B;
  a.H = H;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)), ndir);
  for (a.s = 0; a.s <= T; ++a.s) {
    if (U == 32)
      lstm_seq_bwd<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      lstm_seq_bwd<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}
