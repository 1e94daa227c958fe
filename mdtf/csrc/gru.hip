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
