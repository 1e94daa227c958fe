// GRU recurrence (TF GRUCell: the reset gate is applied before the candidate product) for gfx950: two launches per
// time step, each a skinny MFMA GEMM with the cell arithmetic in its epilogue.  bf16 activations and weights, fp32
// accumulation, and an fp32 copy of the state that every step updates.  ops/gru.py is the caller; the input half
// (x @ [gates/kernel[:I] | candidate/kernel[:I]] + biases over all T * B rows), the weight gradients and dx are
// ordinary GEMMs and stay on the dense routes.
//
//   [r u] = sigmoid(xg_t[:, :2H] + h_{t-1} @ gates/kernel[I:])               gates/kernel     [I + H, 2H]
//   c     = tanh(xg_t[:, 2H:] + (r * h_{t-1}) @ candidate/kernel[I:])        candidate/kernel [I + H, H]
//   h_t   = u * h_{t-1} + (1 - u) * c
//
// Why two launches.  The candidate GEMM's K operand is r * h over all H units, so no block that owns a slice of units
// can finish the cell by itself: gru_gate_fwd makes r, u and rh = bf16(r * h) for its units, and gru_cand_fwd, a
// launch later, multiplies all of rh and finishes h for the same units.  The gate launch reads all of hs[t - 1] and
// writes only rh[t], the r | u thirds of gates[t] and its own elements of hf[t]; the candidate launch reads all of
// rh[t] and, of hs[t], hf[t] and the c third of gates[t], only touches its own elements.  So no launch reads what a
// concurrent block of the same launch writes.
//
// The carry.  h is a leaky integrator: where u is near 1 a step adds (1 - u) * (c - h), which a bf16 h would round
// away.  hf [T, B, H] holds h in fp32; every elementwise use of h_{t-1} (r * h, the update, the backward's h_prev)
// reads it, and hs = bf16(hf) exists as the GEMM operand and as the layer's output.  The same goes for u: near 1,
// bf16 leaves 1 - u with two or three significant bits, an error as large as a bf16 carry's.  Between the two
// launches of step t, hf[t] therefore holds u in fp32 (the gate launch's owner lane writes it, the candidate
// launch's owner lane reads it and overwrites it with h_t); the bf16 u in gates[t] is for the backward.
//
// Work split (rnn_tile.h, as lstm.hip).  A block owns U hidden units (16 or 32) of one 16-row batch tile, the r and u
// strips of them in the gate launch (2 * U / 16 strips), one strip set in the candidate launch (U / 16); K is split
// over the block's four waves in interleaved 32-wide steps, both operands are 16-byte K-contiguous vectors loaded
// into VGPRs through a two-slot register ring, and the four partial tiles are summed through LDS in wave order (fixed,
// so bitwise repeatable).  gru_pack_w repacks the recurrent rows of both kernels once per forward call:
// gates/kernel[I:] -> wt_g[H / Ug][2][Ug][H] and candidate/kernel[I:] -> wt_c[H / Uc][Uc][H], K-contiguous.
//
// Backward, t = T - 1 .. 0, dG [T, B, 3H] = [dpr | dpu | dpc] (pre-activation gradients), dh_carry [B, H] fp32 in
// place (dL/dh_T in, dL/dh_0 out):
//
//   gru_bwd_a   dh = dh_carry + dG[t + 1][:, :2H] @ gates/kernel[I + slice, :]^T + dhs[t]     (K = 2H, natural layouts)
//               dpc = dh (1 - u) (1 - c^2),  dpu = dh (h_prev - c) u (1 - u),  dh_carry = dh u
//   gru_bwd_b   d_rh = dG[t][:, 2H:] @ candidate/kernel[I + slice, :]^T                          (K = H, natural layouts)
//               dpr = d_rh h_prev r (1 - r),  dh_carry += d_rh r
//
// and one last gru_bwd_a launch (t = -1) that runs only the GEMM over dG[0]: dh_carry += gemm.  gru_bwd_a at step t
// reads the r | u columns of dG[t + 1] and writes the u | c columns of dG[t]; gru_bwd_b reads the c columns of dG[t]
// and writes its r columns: each launch reads columns or steps of dG that no block of the same launch writes.
//
// No kernel spans time steps, no block waits for another, no float atomics: every (row, unit) of every output has
// exactly one owner lane in exactly one block per launch.  The entry points allocate nothing and loop over t
// themselves, so they replay inside a hipGraph.
//
// gru_gate_fwd / gru_cand_fwd / gru_bwd_a / gru_bwd_b run full-length, forward-in-time sequences (mdtf_gru_fwd /
// mdtf_gru_bwd); gru_gate_seq / gru_cand_seq / gru_bwd_a_seq / gru_bwd_b_seq further down add per-row lengths, the
// reverse direction and two directions per launch (mdtf_gru_fwd_seq / mdtf_gru_bwd_seq) on the same GEMM, reduction
// and cell arithmetic, and give the same bits where every row has length T.  All of the above holds for them; the
// comment in front of them says how liveness, the previous-state operand and the dG rule carry over.  The lengths
// are read by the kernels only, so results are bitwise repeatable and a captured call replays after the lengths
// change in place.  A full-length launch of the seq kernels costs 0.6 to 0.9 us more than its plain counterpart
// (profiles/gru.md, "Lengths and two directions"), which is why the plain ones stay.
#include "rnn_tile.h"

namespace {

// gates/kernel[I:] ([H, 2H], k-major) -> wt_g[H / Ug][2][Ug][H] and candidate/kernel[I:] ([H, H]) ->
// wt_c[H / Uc][Uc][H] (K-contiguous) in one launch: 32 x 32 tiles through LDS, both sides coalesced.  blockIdx.x
// counts 32-column tiles of [gates | candidate].
__global__ __launch_bounds__(256) void gru_pack_w(const bf16_t* __restrict__ wg, const bf16_t* __restrict__ wc,
                                                  bf16_t* __restrict__ wt_g, bf16_t* __restrict__ wt_c, int H, int Ug,
                                                  int Uc) {
  __shared__ bf16_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const bool cand = static_cast<int>(blockIdx.x) >= 2 * H / 32;            // block-uniform
  const bf16_t* w = cand ? wc : wg;
  bf16_t* wt = cand ? wt_c : wt_g;
  const int G = cand ? 1 : 2, U = cand ? Uc : Ug;
  const int k0 = blockIdx.y * 32, n0 = (cand ? blockIdx.x - 2 * H / 32 : blockIdx.x) * 32;
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[ty + 8 * r][tx] = w[static_cast<int64_t>(k0 + ty + 8 * r) * (G * H) + n0 + tx];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int col = n0 + ty + 8 * r;
    const int g = col / H, unit = col - g * H;
    const int s = unit / U, u = unit - s * U;
    wt[(static_cast<int64_t>(s * G + g) * U + u) * H + k0 + tx] = tile[tx][ty + 8 * r];
  }
}

struct FwdArgs {
  const bf16_t* xg;      // [B, 3H] of this step: the input half of r | u | c, biases included
  const bf16_t* wt;      // wt_g (gate launch) or wt_c (candidate launch)
  const bf16_t* a;       // the GEMM's A operand [B, H]: hs[t - 1] / h0 (gate), rh[t] (candidate)
  const float* h_prev;   // [B, H] fp32: hf[t - 1] / h0
  bf16_t* rh;            // [B, H], written by the gate launch
  bf16_t* gates;         // [B, 3H], post-activation r | u | c
  bf16_t* h;             // [B, H], written by the candidate launch
  float* hf;             // [B, H]: u from the gate launch, then h from the candidate launch
  int B, H;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_gate_fwd(FwdArgs a) {
  constexpr int NT = U / 16, NB = 2 * NT;          // strip g * NT + nt: gate g (r, u), units nt * 16 .. + 15
  __shared__ float red[kWaves * NB * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float4v acc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
  const int arow = row0 + lr;
  const bool a_ok = arow < a.B;
  const bf16_t* a_lane = a.a + static_cast<int64_t>(a_ok ? arow : 0) * H + lk;
  const bf16_t* b_lane = a.wt + (static_cast<int64_t>(slice) * 2 * U + lr) * H + lk;
  skinny_gemm<NB>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);

  float pre[NB];
  reduce_waves<NB>(red, acc, wave, lane, pre);

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    const float r = sigmoid_fast(pre[nt] + bf2f(a.xg[g0]));
    const float u = sigmoid_fast(pre[NT + nt] + bf2f(a.xg[g0 + H]));
    a.gates[g0] = f2bf(r);
    a.gates[g0 + H] = f2bf(u);
    a.rh[s0] = f2bf(r * a.h_prev[s0]);
    a.hf[s0] = u;                                  // fp32, for the candidate launch of this step (see "The carry")
  }
}

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_cand_fwd(FwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float4v acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
  const int arow = row0 + lr;
  const bool a_ok = arow < a.B;
  const bf16_t* a_lane = a.a + static_cast<int64_t>(a_ok ? arow : 0) * H + lk;
  const bf16_t* b_lane = a.wt + (static_cast<int64_t>(slice) * U + lr) * H + lk;
  skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);

  float pre[NT];
  reduce_waves<NT>(red, acc, wave, lane, pre);

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    const float c = tanh_fast(pre[nt] + bf2f(a.xg[g0 + 2 * H]));
    const float u = a.hf[s0];                      // left here in fp32 by the gate launch; h replaces it below
    const float h = u * a.h_prev[s0] + (1.0f - u) * c;
    a.hf[s0] = h;
    a.h[s0] = f2bf(h);
    a.gates[g0 + 2 * H] = f2bf(c);
  }
}

struct BwdArgs {
  const bf16_t* dg_src;   // the GEMM's A rows [B, 3H]: dG[t + 1] (a; null at t = T - 1: no GEMM), dG[t] (b)
  const bf16_t* w;        // gates/kernel[I:] [H, 2H] (a) or candidate/kernel[I:] [H, H] (b)
  const bf16_t* gates;    // gates[t] [B, 3H]; null: GEMM only (the t = -1 launch of a)
  const float* h_prev;    // hf[t - 1] or h0, fp32 [B, H]
  const bf16_t* dh_out;   // dhs[t] [B, H]
  float* dh_carry;        // [B, H] fp32, in place
  bf16_t* dg;             // dG[t] [B, 3H]
  int B, H;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_bwd_a(BwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float dhr[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dhr[nt] = 0.f;
  if (a.dg_src != nullptr) {                       // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const int arow = row0 + lr;
    const bool a_ok = arow < a.B;
    const bf16_t* a_lane = a.dg_src + static_cast<int64_t>(a_ok ? arow : 0) * 3 * H + lk;
    const bf16_t* b_lane = a.w + static_cast<int64_t>(slice * U + lr) * 2 * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * 2 * H, 2 * H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, dhr);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (a.gates == nullptr) {
      a.dh_carry[s0] += dhr[nt];
      continue;
    }
    const float dh = a.dh_carry[s0] + dhr[nt] + bf2f(a.dh_out[s0]);
    const float u = bf2f(a.gates[g0 + H]), c = bf2f(a.gates[g0 + 2 * H]);
    a.dg[g0 + 2 * H] = f2bf(dh * (1.0f - u) * (1.0f - c * c));
    a.dg[g0 + H] = f2bf(dh * (a.h_prev[s0] - c) * u * (1.0f - u));
    a.dh_carry[s0] = dh * u;
  }
}

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_bwd_b(BwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;

  float4v acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
  const int arow = row0 + lr;
  const bool a_ok = arow < a.B;
  const bf16_t* a_lane = a.dg_src + static_cast<int64_t>(a_ok ? arow : 0) * 3 * H + 2 * H + lk;
  const bf16_t* b_lane = a.w + static_cast<int64_t>(slice * U + lr) * H + lk;
  skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);
  float drh[NT];
  reduce_waves<NT>(red, acc, wave, lane, drh);

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    const float r = bf2f(a.gates[g0]);
    a.dg[g0] = f2bf(drh[nt] * a.h_prev[s0] * r * (1.0f - r));
    a.dh_carry[s0] += drh[nt] * r;
  }
}

// ---- per-row lengths and direction (tf.nn.dynamic_rnn(sequence_length=), a forward plus a reverse GRU) --------------
//
// Row b is live at step t iff t < clamp(lens[b], 0, T); a dead row emits zeros and keeps its state.  A reverse
// direction visits t = T - 1 .. 0 under the same rule (TF's reverse_sequence -> GRU -> reverse_sequence with nothing
// reversed in memory): its padding steps come first and leave the initial state in place.  The state is never copied
// through dead steps: the A operand of skinny_gemm is per lane (a lane owns row l % 16), so each live row reads
// hs[the step visited before] / hf[the same], or h0 / h0f at its first visited live step (t = 0 forward, t = len - 1
// reverse), and a dead row is read as zeros.  Both launches of a step derive liveness from `lens` alone, so the fp32
// u that hf[t] hands from the gate launch to the candidate launch exists exactly where the candidate launch reads it.
// A 16-row tile with no live row skips its GEMM (the ballot is the same in every wave: a wave's lanes cover all 16
// rows) and only writes zeros.  Dead (t, b) of hs, hf, rh, gates and dG are written as zeros, because the caller
// multiplies whole [T * B, .] buffers into the weight gradients and dx.  blockIdx.z is the direction; launch s runs
// step s of a forward direction and step T - 1 - s of a reverse one.  `lens` is read here and nowhere on the host;
// null: every row has length T.
//
// dG in both directions.  With tn the step the forward visited after t (t + 1 forward, t - 1 reverse), gru_bwd_a_seq
// at step t reads the r | u columns of dG[tn] and writes the u | c columns of dG[t], and tn != t; its closing launch
// reads, per row, the r | u columns of dG[that row's first visited live step] and writes no dG at all.
// gru_bwd_b_seq reads the c columns of dG[t] and writes its r columns.  Each direction has a dG of its own.  So in
// either direction a launch reads only columns or steps of dG that none of its blocks writes.

constexpr int kDirs = 2;

__device__ __forceinline__ int row_len(const int* lens, int row, int T) {
  return lens != nullptr ? min(max(lens[row], 0), T) : T;
}

struct SeqFwdDir {
  const bf16_t* xg;      // [T, B, ldx]: this direction's 3H columns of the input half
  const bf16_t* wt_g;    // packed recurrent weights of the gate launch
  const bf16_t* wt_c;    // ... of the candidate launch
  const bf16_t* h0;      // [B, H]
  const float* h0f;      // [B, H], the same state in fp32
  bf16_t* hs;            // [T, B, H], zeros at dead (t, b), as are hf, rh and gates
  float* hf;             // [T, B, H]
  bf16_t* rh;            // [T, B, H]
  bf16_t* gates;         // [T, B, 3H]
  bf16_t* h_fin;         // [B, H]: hs at the row's last visited live step (h0 for length 0)
  int reverse;
};

struct SeqFwdArgs {
  SeqFwdDir d[kDirs];
  const int* lens;       // [B] or null
  int s, T, B, H, ldx;
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_gate_seq(SeqFwdArgs a) {
  constexpr int NT = U / 16, NB = 2 * NT;
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
    const bf16_t* b_lane = d.wt_g + (static_cast<int64_t>(slice) * 2 * U + lr) * H + lk;
    skinny_gemm<NB>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);
    reduce_waves<NB>(red, acc, wave, lane, pre);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0;
  const float* h_prev = first ? d.h0f : d.hf + tp * sh;
  const bf16_t* xg = d.xg + (static_cast<int64_t>(t) * a.B + row) * a.ldx;
  bf16_t* gates = d.gates + t * 3 * sh;
  bf16_t* rh = d.rh + t * sh;
  float* hf = d.hf + t * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (!live) {
      gates[g0] = gates[g0 + H] = rh[s0] = f2bf(0.f);
      continue;
    }
    const float r = sigmoid_fast(pre[nt] + bf2f(xg[unit]));
    const float u = sigmoid_fast(pre[NT + nt] + bf2f(xg[unit + H]));
    gates[g0] = f2bf(r);
    gates[g0 + H] = f2bf(u);
    rh[s0] = f2bf(r * h_prev[s0]);
    hf[s0] = u;                                    // fp32, for the candidate launch of this step (see "The carry")
  }
}

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_cand_seq(SeqFwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const SeqFwdDir& d = a.d[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;
  const bool rev = d.reverse != 0;
  const int t = rev ? a.T - 1 - a.s : a.s, tp = rev ? t + 1 : t - 1;
  const int64_t sh = static_cast<int64_t>(a.B) * H;

  const int arow = row0 + lr;
  const bool a_ok = arow < a.B && t < row_len(a.lens, arow, a.T);
  const bf16_t* a_lane = d.rh + t * sh + static_cast<int64_t>(a_ok ? arow : 0) * H + lk;
  float pre[NT];
  if (__ballot(a_ok) != 0) {                       // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const bf16_t* b_lane = d.wt_c + (static_cast<int64_t>(slice) * U + lr) * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, pre);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0, last = rev ? t == 0 : t + 1 == len;
  const float* h_prev = first ? d.h0f : d.hf + tp * sh;
  const bf16_t* xg = d.xg + (static_cast<int64_t>(t) * a.B + row) * a.ldx;
  bf16_t* gates = d.gates + t * 3 * sh;
  bf16_t* hs = d.hs + t * sh;
  float* hf = d.hf + t * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (!live) {
      gates[g0 + 2 * H] = hs[s0] = f2bf(0.f);
      hf[s0] = 0.f;
      if (len == 0 && a.s == 0) d.h_fin[s0] = d.h0[s0];
      continue;
    }
    const float c = tanh_fast(pre[nt] + bf2f(xg[unit + 2 * H]));
    const float u = hf[s0];                        // left here in fp32 by the gate launch; h replaces it below
    const float h = u * h_prev[s0] + (1.0f - u) * c;
    hf[s0] = h;
    hs[s0] = f2bf(h);
    gates[g0 + 2 * H] = f2bf(c);
    if (last) d.h_fin[s0] = f2bf(h);
  }
}

struct SeqBwdDir {
  const bf16_t* wg;       // gates/kernel[I:] [H, 2H]
  const bf16_t* wc;       // candidate/kernel[I:] [H, H]
  const bf16_t* gates;    // [T, B, 3H]
  const float* hf;        // [T, B, H]
  const float* h0f;       // [B, H]
  const bf16_t* dhs;      // [T, B, H]
  float* dh_carry;        // [B, H] fp32, in place; a dead row leaves it alone, which carries dL/dh_T to its last step
  bf16_t* dg;             // dG [T, B, 3H], zeros at dead (t, b)
  int reverse;
};

struct SeqBwdArgs {
  SeqBwdDir d[kDirs];
  const int* lens;
  int s, T, B, H;         // s = T: the closing GEMM-only launch of gru_bwd_a_seq
};

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_bwd_a_seq(SeqBwdArgs a) {
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
    // the closing launch reads dG of the row's first visited live step; a step reads dG[tn] where the row was live
    a_ok = fin ? len > 0 : t < len && (rev ? t > 0 : t + 1 < len);
    const int src = fin ? (rev ? len - 1 : 0) : tn;
    if (a_ok) a_lane = d.dg + (src * sh + static_cast<int64_t>(arow) * H) * 3 + lk;
  }
  float dhr[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) dhr[nt] = 0.f;
  if (__ballot(a_ok) != 0) {                       // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const bf16_t* b_lane = d.wg + static_cast<int64_t>(slice * U + lr) * 2 * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * 2 * H, 2 * H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, dhr);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0;
  // (the closing launch dereferences none of these)
  const bf16_t* gates = d.gates + t * 3 * sh;
  const float* h_prev = first ? d.h0f : d.hf + tp * sh;
  const bf16_t* dh_out = d.dhs + t * sh;
  bf16_t* dg = d.dg + t * 3 * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (fin) {
      if (len > 0) d.dh_carry[s0] += dhr[nt];      // a row of length 0 returns dL/dh_T as it came
      continue;
    }
    if (!live) {
      dg[g0 + H] = dg[g0 + 2 * H] = f2bf(0.f);
      continue;
    }
    const float dh = d.dh_carry[s0] + dhr[nt] + bf2f(dh_out[s0]);
    const float u = bf2f(gates[g0 + H]), c = bf2f(gates[g0 + 2 * H]);
    dg[g0 + 2 * H] = f2bf(dh * (1.0f - u) * (1.0f - c * c));
    dg[g0 + H] = f2bf(dh * (h_prev[s0] - c) * u * (1.0f - u));
    d.dh_carry[s0] = dh * u;
  }
}

template <int U>
__global__ __launch_bounds__(kWaves* kWave) void gru_bwd_b_seq(SeqBwdArgs a) {
  constexpr int NT = U / 16;
  __shared__ float red[kWaves * NT * 4 * kWave];
  const SeqBwdDir& d = a.d[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slice = blockIdx.x, row0 = blockIdx.y * kRows;
  const int H = a.H, lr = lane & 15, lk = (lane >> 4) * 8;
  const bool rev = d.reverse != 0;
  const int t = rev ? a.s : a.T - 1 - a.s, tp = rev ? t + 1 : t - 1;
  const int64_t sh = static_cast<int64_t>(a.B) * H;

  const int arow = row0 + lr;
  const bool a_ok = arow < a.B && t < row_len(a.lens, arow, a.T);
  const bf16_t* a_lane = d.dg + (t * sh + static_cast<int64_t>(a_ok ? arow : 0) * H) * 3 + 2 * H + lk;
  float drh[NT];
  if (__ballot(a_ok) != 0) {                       // block-uniform
    float4v acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = float4v{0.f, 0.f, 0.f, 0.f};
    const bf16_t* b_lane = d.wc + static_cast<int64_t>(slice * U + lr) * H + lk;
    skinny_gemm<NT>(a_lane, a_ok, b_lane, static_cast<int64_t>(16) * H, H / kStep, wave, acc);
    reduce_waves<NT>(red, acc, wave, lane, drh);
  }

  const int row = row0 + (lane >> 4) * 4 + wave;
  if (row >= a.B) return;
  const int len = row_len(a.lens, row, a.T);
  const bool live = t < len, first = rev ? t + 1 >= len : t == 0;
  const bf16_t* gates = d.gates + t * 3 * sh;
  const float* h_prev = first ? d.h0f : d.hf + tp * sh;
  bf16_t* dg = d.dg + t * 3 * sh;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int unit = slice * U + nt * 16 + lr;
    const int64_t g0 = static_cast<int64_t>(row) * 3 * H + unit, s0 = static_cast<int64_t>(row) * H + unit;
    if (!live) {
      dg[g0] = f2bf(0.f);
      continue;
    }
    const float r = bf2f(gates[g0]);
    dg[g0] = f2bf(drh[nt] * h_prev[s0] * r * (1.0f - r));
    d.dh_carry[s0] += drh[nt] * r;
  }
}

constexpr int kBf16 = 0;       // the dtype code of the entry points (1: fp32, refused)

// Hidden units per block.  The candidate launch and both backward launches (one strip per 16 units) follow
// lstm.hip's rule: 32 where that still gives every CU of the device a block, else 16.  The gate launch (two strips per
// 16 units) takes 16: at the three shapes of bench/gru_probe.py --units a forward step was 0.4 to 1.4 us slower with
// gru_gate_fwd<32>, also where the rule says 32 (profiles/gru.md, "U").  mdtf_gru_force_units keeps <32> reachable
// for that probe.
int pick_u(int B, int H) {
  const int64_t tiles = ceil_div(B, kRows);
  return tiles * (H / 32) >= 256 ? 32 : 16;
}

int g_force_ug = 0, g_force_uc = 0;    // mdtf_gru_force_units
int units_gate(int, int) { return g_force_ug ? g_force_ug : 16; }
int units_cand(int B, int H) { return g_force_uc ? g_force_uc : pick_u(B, H); }

bool supported(int T, int B, int H, int dtype) {
  return dtype == kBf16 && T >= 1 && B >= 1 && H >= 32 && H % 32 == 0 && static_cast<int64_t>(B) * 3 * H < (1LL << 31) &&
         ceil_div(B, kRows) <= 65535;
}

}  // namespace

// Units per block the step kernels use for this problem: the gate launch's U (16 or 32) in the low byte, the U of
// the candidate launch and of both backward launches in the next; 0 where the entry points refuse the problem.
MDTF_EXPORT int mdtf_gru_units(int T, int B, int H, int dtype) {
  return supported(T, B, H, dtype) ? units_gate(B, H) | (units_cand(B, H) << 8) : 0;
}

// For bench/gru_probe.py: force U of the gate launch / of the other launches to 16 or 32 (0: the rule decides).
MDTF_EXPORT int mdtf_gru_force_units(int gate, int cand) {
  for (int u : {gate, cand})
    if (u != 0 && u != 16 && u != 32) return MDTF_EINVAL;
  g_force_ug = gate;
  g_force_uc = cand;
  return MDTF_OK;
}

// The recurrence over t = 0 .. T - 1: one pack launch and 2T step launches on `st`.  xg [T, B, 3H] bf16 (input half
// of r | u | c, biases included), wg = gates/kernel[I:] [H, 2H] bf16, wc = candidate/kernel[I:] [H, H] bf16, wt:
// workspace of 3 * H * H bf16, h0 [B, H] bf16 and the same state in fp32 (h0f); out: hs [T, B, H] bf16, hf [T, B, H]
// fp32, rh [T, B, H] bf16, gates [T, B, 3H] bf16 (post-activation r | u | c).  Every pointer 16-byte aligned.
MDTF_EXPORT int mdtf_gru_fwd(const void* xg, const void* wg, const void* wc, void* wt, const void* h0, const float* h0f,
                             void* hs, float* hf, void* rh, void* gates, int T, int B, int H, int dtype,
                             hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!xg || !wg || !wc || !wt || !h0 || !h0f || !hs || !hf || !rh || !gates) return MDTF_EINVAL;
  const int Ug = units_gate(B, H), Uc = units_cand(B, H);
  bf16_t* wt_g = static_cast<bf16_t*>(wt);
  bf16_t* wt_c = wt_g + static_cast<int64_t>(2) * H * H;
  gru_pack_w<<<dim3(3 * H / 32, H / 32), 256, 0, st>>>(static_cast<const bf16_t*>(wg), static_cast<const bf16_t*>(wc),
                                                       wt_g, wt_c, H, Ug, Uc);
  MDTF_LAUNCH_CHECK();
  const int64_t sh = static_cast<int64_t>(B) * H;
  const unsigned tiles = static_cast<unsigned>(ceil_div(B, kRows));
  for (int t = 0; t < T; ++t) {
    FwdArgs a;
    a.xg = static_cast<const bf16_t*>(xg) + t * 3 * sh;
    a.wt = wt_g;
    a.a = t ? static_cast<const bf16_t*>(hs) + (t - 1) * sh : static_cast<const bf16_t*>(h0);
    a.h_prev = t ? hf + (t - 1) * sh : h0f;
    a.rh = static_cast<bf16_t*>(rh) + t * sh;
    a.gates = static_cast<bf16_t*>(gates) + t * 3 * sh;
    a.h = static_cast<bf16_t*>(hs) + t * sh;
    a.hf = hf + t * sh;
    a.B = B;
    a.H = H;
    if (Ug == 32)
      gru_gate_fwd<32><<<dim3(H / 32, tiles), kWaves * kWave, 0, st>>>(a);
    else
      gru_gate_fwd<16><<<dim3(H / 16, tiles), kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
    a.wt = wt_c;
    a.a = a.rh;
    if (Uc == 32)
      gru_cand_fwd<32><<<dim3(H / 32, tiles), kWaves * kWave, 0, st>>>(a);
    else
      gru_cand_fwd<16><<<dim3(H / 16, tiles), kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// The recurrence backwards, t = T - 1 .. 0, two launches per step, then the GEMM-only launch: 2T + 1 launches on
// `st`.  wg, wc as the forward's; gates, hf as the forward left them; h0f [B, H] fp32; dhs [T, B, H] bf16; dh_carry
// [B, H] fp32 holds dL/dh_T on entry and dL/dh_0 on return; out: dg [T, B, 3H] bf16 = [dpr | dpu | dpc].
MDTF_EXPORT int mdtf_gru_bwd(const void* wg, const void* wc, const void* gates, const float* hf, const float* h0f,
                             const void* dhs, float* dh_carry, void* dg, int T, int B, int H, int dtype,
                             hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!wg || !wc || !gates || !hf || !h0f || !dhs || !dh_carry || !dg) return MDTF_EINVAL;
  const int U = units_cand(B, H);
  const int64_t sh = static_cast<int64_t>(B) * H;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)));
  for (int t = T - 1; t >= -1; --t) {
    BwdArgs a;
    a.dg_src = t < T - 1 ? static_cast<const bf16_t*>(dg) + (t + 1) * 3 * sh : nullptr;
    a.w = static_cast<const bf16_t*>(wg);
    a.gates = t >= 0 ? static_cast<const bf16_t*>(gates) + t * 3 * sh : nullptr;
    a.h_prev = t > 0 ? hf + (t - 1) * sh : h0f;
    a.dh_out = t >= 0 ? static_cast<const bf16_t*>(dhs) + t * sh : nullptr;
    a.dh_carry = dh_carry;
    a.dg = t >= 0 ? static_cast<bf16_t*>(dg) + t * 3 * sh : nullptr;
    a.B = B;
    a.H = H;
    if (U == 32)
      gru_bwd_a<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      gru_bwd_a<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
    if (t < 0) break;
    a.dg_src = a.dg;
    a.w = static_cast<const bf16_t*>(wc);
    if (U == 32)
      gru_bwd_b<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      gru_bwd_b<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// The length- and direction-aware recurrence of `ndir` (1 or 2) independent GRUs over the same T, B, H and the same
// lengths, every step of all of them in the same two launches: ndir pack launches and 2T step launches on `st`.  Bit
// d of `reverse`: direction d visits t = T - 1 .. 0.  `lens`: int32 [B] on the device (clamped to [0, T], never read
// by the host) or null.  `tab` (host memory, read before the call returns) holds 11 pointers per direction, in the
// order xg, wg, wc, wt, h0, h0f, hs, hf, rh, gates, h_fin: as mdtf_gru_fwd, except that xg rows are `ldx` elements
// apart (the directions may be column ranges of one [T * B, ndir * 3H] product) and that h_fin [B, H] bf16 receives
// the final state.  hs, hf, rh and gates are zero at dead (t, b).
MDTF_EXPORT int mdtf_gru_fwd_seq(const void* const* tab, int ndir, int reverse, const int* lens, int T, int B, int H,
                                 int ldx, int dtype, hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!tab || ndir < 1 || ndir > kDirs || ldx < 3 * H || ldx % 8) return MDTF_EINVAL;
  for (int i = 0; i < 11 * ndir; ++i)
    if (!tab[i]) return MDTF_EINVAL;
  const int Ug = units_gate(B, H), Uc = units_cand(B, H);
  SeqFwdArgs a;
  for (int d = 0; d < kDirs; ++d) {
    const void* const* p = tab + 11 * (d < ndir ? d : 0);     // (an unused slot repeats direction 0; no block reads it)
    bf16_t* wt_g = static_cast<bf16_t*>(const_cast<void*>(p[3]));
    bf16_t* wt_c = wt_g + static_cast<int64_t>(2) * H * H;
    if (d < ndir) {
      gru_pack_w<<<dim3(3 * H / 32, H / 32), 256, 0, st>>>(static_cast<const bf16_t*>(p[1]),
                                                           static_cast<const bf16_t*>(p[2]), wt_g, wt_c, H, Ug, Uc);
      MDTF_LAUNCH_CHECK();
    }
    SeqFwdDir& q = a.d[d];
    q.xg = static_cast<const bf16_t*>(p[0]);
    q.wt_g = wt_g;
    q.wt_c = wt_c;
    q.h0 = static_cast<const bf16_t*>(p[4]);
    q.h0f = static_cast<const float*>(p[5]);
    q.hs = static_cast<bf16_t*>(const_cast<void*>(p[6]));
    q.hf = static_cast<float*>(const_cast<void*>(p[7]));
    q.rh = static_cast<bf16_t*>(const_cast<void*>(p[8]));
    q.gates = static_cast<bf16_t*>(const_cast<void*>(p[9]));
    q.h_fin = static_cast<bf16_t*>(const_cast<void*>(p[10]));
    q.reverse = (reverse >> d) & 1;
  }
  a.lens = lens;
  a.T = T;
  a.B = B;
  a.H = H;
  a.ldx = ldx;
  const unsigned tiles = static_cast<unsigned>(ceil_div(B, kRows));
  for (a.s = 0; a.s < T; ++a.s) {
    if (Ug == 32)
      gru_gate_seq<32><<<dim3(H / 32, tiles, ndir), kWaves * kWave, 0, st>>>(a);
    else
      gru_gate_seq<16><<<dim3(H / 16, tiles, ndir), kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
    if (Uc == 32)
      gru_cand_seq<32><<<dim3(H / 32, tiles, ndir), kWaves * kWave, 0, st>>>(a);
    else
      gru_cand_seq<16><<<dim3(H / 16, tiles, ndir), kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}

// Its backward: 2T + 1 launches on `st`, the last one the GEMM-only launch that turns the carry into dL/dh_0.  `tab`:
// 8 pointers per direction, in the order wg, wc, gates, hf, h0f, dhs, dh_carry, dg, as mdtf_gru_bwd.  dg is zero at
// dead (t, b); dh_carry of a row of length 0 is returned as it came.
MDTF_EXPORT int mdtf_gru_bwd_seq(const void* const* tab, int ndir, int reverse, const int* lens, int T, int B, int H,
                                 int dtype, hipStream_t st) {
  if (!supported(T, B, H, dtype)) return MDTF_EUNSUPPORTED;
  if (!tab || ndir < 1 || ndir > kDirs) return MDTF_EINVAL;
  for (int i = 0; i < 8 * ndir; ++i)
    if (!tab[i]) return MDTF_EINVAL;
  const int U = units_cand(B, H);
  SeqBwdArgs a;
  for (int d = 0; d < kDirs; ++d) {
    const void* const* p = tab + 8 * (d < ndir ? d : 0);
    SeqBwdDir& q = a.d[d];
    q.wg = static_cast<const bf16_t*>(p[0]);
    q.wc = static_cast<const bf16_t*>(p[1]);
    q.gates = static_cast<const bf16_t*>(p[2]);
    q.hf = static_cast<const float*>(p[3]);
    q.h0f = static_cast<const float*>(p[4]);
    q.dhs = static_cast<const bf16_t*>(p[5]);
    q.dh_carry = static_cast<float*>(const_cast<void*>(p[6]));
    q.dg = static_cast<bf16_t*>(const_cast<void*>(p[7]));
    q.reverse = (reverse >> d) & 1;
  }
  a.lens = lens;
  a.T = T;
  a.B = B;
  a.H = H;
  const dim3 grid(H / U, static_cast<unsigned>(ceil_div(B, kRows)), ndir);
  for (a.s = 0; a.s <= T; ++a.s) {
    if (U == 32)
      gru_bwd_a_seq<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      gru_bwd_a_seq<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
    if (a.s == T) break;
    if (U == 32)
      gru_bwd_b_seq<32><<<grid, kWaves * kWave, 0, st>>>(a);
    else
      gru_bwd_b_seq<16><<<grid, kWaves * kWave, 0, st>>>(a);
    MDTF_LAUNCH_CHECK();
  }
  return MDTF_OK;
}
