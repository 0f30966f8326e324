// One inference timestep of a single-layer LSTM (the baseline captioner's recurrence, reference
// models/baseline.py:81-111 with torch.nn.LSTM's gate order i,f,g,o) in one launch:
//
//   gates[r] = pre[r] + x[r] W_ih^T + h_prev[r] W_hh^T + b_ih + b_hh      (each term optional)
//   c = sig(f) c_prev + sig(i) tanh(g);  h = sig(o) tanh(c)
//
// Only h_out / c_out [R][H] are written: no 4H-wide gate tensor and no activation history reach HBM. It
// stands for the three launches of the training forward's step (recurrent GEMM, hoisted input GEMM,
// capmi_lstm_cell_fwd) in the validation pass and the beam search, which keep nothing for a backward.
//
// Tile ownership: a workgroup owns 64 rows x 16 hidden units WITH ALL FOUR GATES of those units (the
// gate-interleaved 64-column tile of decoder_step.hip: LDS row 16 q + u = W row q H + unit) and the WHOLE
// k range (x's M, then h's H). So nothing is handed between workgroups: no split-K, no atomics, no
// counters. Inside the workgroup the k-tiles are dealt to four k-groups of four waves (contiguous ranges,
// fixed by M and H alone) whose accumulators meet in LDS and are added in group order by the thread that
// owns the (row, unit): the four gates of a unit sit in the same tile, so the cell runs right there, on all
// 1024 threads. A row's value depends on its own inputs and on (M, H) only: the same bits at R = 1 and
// inside R = 65.
//
// Arithmetic: the fp32-accurate x3 split on v_mfma_f32_16x16x32_bf16 (six products per block, smallest
// first, fp32 accumulation), as the other decoder GEMMs (gemm_x3.hip, decoder_step.hip). The split happens
// once per value, on the way into LDS (three bf16 planes); the cell's activations are taken in fp64.
//
// Training (below the inference kernel's body): the TRAIN arm of the same kernel also stores the activations
// (capmi_lstm_step_fwd_train), and lstm_step_bwd_kernel is one backward-through-time step with the same
// ownership (capmi_lstm_step_bwd).
#include "gemm_args.h"

namespace {

typedef float f32x4_l __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_l __attribute__((ext_vector_type(8)));
typedef unsigned u32x4_l __attribute__((ext_vector_type(4)));

constexpr int LS_ROWS = 64;   // rows per workgroup
constexpr int LS_UNITS = 16;  // hidden units per workgroup (x 4 gates = 64 columns)
constexpr int LS_NT = 4 * LS_UNITS;
constexpr int LS_BK = 32;     // k per k-tile
constexpr int LS_LDW = 20;    // LDS row stride of a bf16 plane in dwords: 16 hold the 32 k, 4 pad, so the 16 rows
                              // of a ds_read_b128 group start 20 dwords apart and cover the 64 banks once
constexpr int LS_KG = 4;      // k-groups of four waves (1024 threads)
constexpr int LS_DEPTH = 4;   // k-tiles a k-group keeps in flight
constexpr int LS_PLANE = (LS_ROWS + LS_NT) * LS_LDW;  // dwords of one bf16 term of a staging tile (A rows, W rows)
constexpr int LS_GBUF = 3 * LS_PLANE;                 // ... of one k-group's staging tile: the three terms
static_assert(LS_GBUF >= LS_ROWS * LS_NT, "the cross-group sum reuses the staging tile");

struct LsArgs {
  const float *pre, *x, *h_prev, *c_prev, *w_ih, *w_hh, *b_ih, *b_hh;
  long long ld_pre, ld_x, ld_h, ld_c;
  int M, H, R;
  int kt_x, kt;  // k-tiles of the x segment, and of both
  float *h_out, *c_out;
  float* act_out;  // TRAIN arm only: [R][4H] = (sig i | sig f | tanh g | sig o), what a backward step reads
};

__device__ __forceinline__ double sig_l(double v) { return 1.0 / (1.0 + exp(-v)); }

// TRAIN: the training forward step. The same tile, k-group order and fp64 cell, so h_out / c_out are the
// inference arm's bits; the four fp64 activations are also stored, rounded to fp32, in capmi_lstm_cell_fwd's
// act_out layout.
template <bool TRAIN>
__global__ void __launch_bounds__(256 * LS_KG) lstm_step_kernel(const LsArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned lds[LS_KG * LS_GBUF];
  const int tid = threadIdx.x, grp = tid >> 8, t = tid & 255, lane = t & 63, w = t >> 6;
  const int tn = blockIdx.x, m0 = blockIdx.y * LS_ROWS;
  const int R = a.R, H = a.H;
  // this k-group's k-tiles [g0, g0 + ng); ngmax is the same for every thread of the workgroup
  const int g0 = a.kt * grp / LS_KG, ng = a.kt * (grp + 1) / LS_KG - g0;
  const int ngmax = (a.kt + LS_KG - 1) / LS_KG;
  unsigned* Gs = lds + grp * LS_GBUF;

  // staging: A rows ar, ar + 32 and W tile rows wr, wr + 32, each 16 B at k offset ak
  const int ar = t >> 3, ak = (t & 7) * 4;
  long long wrow[2];
  bool wok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = ar + 32 * i, unit = tn * LS_UNITS + (r & 15);
    wok[i] = unit < H;
    wrow[i] = (long long)(r >> 4) * H + unit;
  }

  f32x4_l acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4_l{0.f, 0.f, 0.f, 0.f};

  struct Stage {
    float4 ra[2], rw[2];
  };
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load = [&](Stage& st, int gk) {
    const bool sx = gk < a.kt_x;  // segment: x . W_ih^T, then h_prev . W_hh^T
    const float* A = sx ? a.x : a.h_prev;
    const float* W = sx ? a.w_ih : a.w_hh;
    const long long lda = sx ? a.ld_x : a.ld_h;
    const int K = sx ? a.M : H;
    const int k = (sx ? gk : gk - a.kt_x) * LS_BK + ak;
    const bool kok = k < K;  // K % 4 == 0: a float4 is inside or outside as a whole; the tail is zero-filled
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = m0 + ar + 32 * i;
      st.ra[i] = (kok && row < R) ? *reinterpret_cast<const float4*>(A + (long long)row * lda + k) : zero4;
      st.rw[i] = (kok && wok[i]) ? *reinterpret_cast<const float4*>(W + wrow[i] * K + k) : zero4;
    }
  };
  // a value is split into its three bf16 terms once, by the thread that staged it (not by every wave that
  // multiplies it): four k of a row become one 8-byte store per term plane
  auto put = [&](const float4 v, int row) {
    unsigned lo[3], hi[3];
    split3_pair(v.x, v.y, lo);
    split3_pair(v.z, v.w, hi);
#pragma unroll
    for (int p = 0; p < 3; ++p)
      *reinterpret_cast<uint2*>(&Gs[p * LS_PLANE + row * LS_LDW + ak / 2]) = make_uint2(lo[p], hi[p]);
  };
  auto store = [&](const Stage& st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      put(st.ra[i], ar + 32 * i);
      put(st.rw[i], LS_ROWS + ar + 32 * i);
    }
  };
  // lane (q = lane / 16, r = lane % 16) reads k 8q .. 8q + 7 of its row: the 16 x 16 x 32 bf16 operand layout
  auto frag = [&](int row, bf16x8_l (&o)[3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      o[p] = __builtin_bit_cast(
          bf16x8_l, *reinterpret_cast<const u32x4_l*>(&Gs[p * LS_PLANE + row * LS_LDW + 4 * (lane >> 4)]));
  };
  auto compute = [&]() {
    bf16x8_l av[3];
    frag(16 * w + (lane & 15), av);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8_l bv[3];
      frag(LS_ROWS + 16 * j + (lane & 15), bv);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[1], acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[2], acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bv[0], acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[1], acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[0], acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[0], acc[j], 0, 0, 0);
    }
  };
  // LS_DEPTH k-tiles are requested before the first is multiplied; a stage's registers are asked for the
  // tile LS_DEPTH further on as soon as they have been parked in LDS
  static_assert(LS_DEPTH == 4, "four named stages below");
  Stage s0, s1, s2, s3;  // named, not an array: each stays in registers across the loop
  s0.ra[0] = s0.ra[1] = s0.rw[0] = s0.rw[1] = zero4;
  s1 = s0;
  s2 = s0;
  s3 = s0;
  if (0 < ng) load(s0, g0);
  if (1 < ng) load(s1, g0 + 1);
  if (2 < ng) load(s2, g0 + 2);
  if (3 < ng) load(s3, g0 + 3);
  auto step = [&](Stage& st, int kt) {  // kt < ngmax: the same for the whole workgroup
    if (kt < ng) {
      store(st);
      if (kt + LS_DEPTH < ng) load(st, g0 + kt + LS_DEPTH);
    }
    __syncthreads();
    if (kt < ng) compute();
    __syncthreads();
  };
  for (int base = 0; base < ngmax; base += LS_DEPTH) {
    step(s0, base);
    if (base + 1 < ngmax) step(s1, base + 1);
    if (base + 2 < ngmax) step(s2, base + 2);
    if (base + 3 < ngmax) step(s3, base + 3);
  }
  // every k-group parks its sums in its own staging tile (lane-linear: the accumulator of wave w, column
  // tile j, lane l at ((4 w + j) 64 + l) 4 + r, r = the lane's four rows)
#pragma unroll
  for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4_l*>(&Gs[((w * 4 + j) * 64 + lane) * 4]) = acc[j];
  __syncthreads();

  // the cell, one (row, unit) per thread of the whole workgroup: the four groups' sums are added in group
  // order, then pre, b_ih and b_hh, and the five activations are taken in fp64, so the step's error is the
  // gate sums' alone (5 transcendentals per element next to 2 (M + H) x 4 multiply-adds)
  const int lrow = tid >> 4, u = tn * LS_UNITS + (tid & 15), row = m0 + lrow;
  if (u >= H || row >= R) return;
  const int slot = (((lrow >> 4) * 4) * 64 + ((lrow & 15) >> 2) * 16 + (tid & 15)) * 4 + (lrow & 3);
  const float* sums = reinterpret_cast<const float*>(lds);
  double g[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float s = sums[slot + q * 256];
#pragma unroll
    for (int k = 1; k < LS_KG; ++k) s += sums[k * LS_GBUF + slot + q * 256];
    double v = (double)s;
    if (a.pre) v += (double)a.pre[(long long)row * a.ld_pre + q * H + u];
    if (a.b_ih) v += (double)a.b_ih[q * H + u];
    if (a.b_hh) v += (double)a.b_hh[q * H + u];
    g[q] = v;
  }
  const double ig = sig_l(g[0]), fg = sig_l(g[1]), cg = tanh(g[2]), og = sig_l(g[3]);
  const double cp = a.c_prev ? (double)a.c_prev[(long long)row * a.ld_c + u] : 0.0;
  const double c = fg * cp + ig * cg;
  const long long o = (long long)row * H + u;
  a.c_out[o] = (float)c;
  a.h_out[o] = (float)(og * tanh(c));
  if constexpr (TRAIN) {
    float* act = a.act_out + (long long)row * 4 * H + u;
    act[0] = (float)ig;
    act[H] = (float)fg;
    act[2 * H] = (float)cg;
    act[3 * H] = (float)og;
  }
}

// --------------------------------------------------------------------------------------------------------
// One backward-through-time step in one launch: the recurrent GEMM first, the cell in its epilogue.
//
//   dh[r][u] = dh_lin[r][u] + sum_{k < 4H} dg_next[r][k] W_hh[k][u]        (each term optional)
//   then lstm_cell_bwd_kernel's formulas (decoder.hip) on act, c_prev, c_cur, dc_in -> dgates, dc_out
//
// Ownership as the forward: a workgroup owns 64 rows x 16 units (H = 512: 32 workgroups) and the whole
// k = 4H range, dealt to the same four k-groups whose sums meet in LDS and are added in group order by the
// thread that owns the (row, unit). Nothing is handed between workgroups.
//
// W_hh is [4H][H] row-major: for this product its n (the unit) is contiguous, not k. It is transposed on the
// way into LDS: a thread takes the two k-rows 2j, 2j + 1 of one unit (the 16 units of a k-row are one 64-byte
// segment), splits the pair and stores one dword per term plane at LDS row = unit, dword j -- the layout the
// forward's W rows have, so the fragment reads and the six products are the forward's. (A (H, 4H) copy made
// once per training step would need a launch and 4 MB of traffic per step for nothing this staging lacks.)
// --------------------------------------------------------------------------------------------------------
constexpr int LB_PLANE = (LS_ROWS + LS_UNITS) * LS_LDW;  // dwords of one bf16 term: 64 A rows, 16 W^T rows
constexpr int LB_GBUF = 3 * LB_PLANE;
static_assert(LB_GBUF >= LS_ROWS * LS_UNITS, "the cross-group sum reuses the staging tile");

struct LbArgs {
  const float *dh_lin, *dg_next, *w_hh, *dc_in, *act, *c_prev, *c_cur;
  long long ld_dh;
  int H, R;
  int kt;  // k-tiles of the 4H range; 0 without dg_next (the last step: no GEMM)
  float *dgates, *dc_out;
};

__global__ void __launch_bounds__(256 * LS_KG) lstm_step_bwd_kernel(const LbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned lds[LS_KG * LB_GBUF];
  const int tid = threadIdx.x, grp = tid >> 8, t = tid & 255, lane = t & 63, w = t >> 6;
  const int tn = blockIdx.x, m0 = blockIdx.y * LS_ROWS;
  const int R = a.R, H = a.H, K = 4 * H;
  const int g0 = a.kt * grp / LS_KG, ng = a.kt * (grp + 1) / LS_KG - g0;
  const int ngmax = (a.kt + LS_KG - 1) / LS_KG;
  unsigned* Gs = lds + grp * LB_GBUF;

  // staging: A (dg_next) rows ar, ar + 32, 16 B at k offset ak; W_hh rows k = 2 bj, 2 bj + 1 of unit bu
  const int ar = t >> 3, ak = (t & 7) * 4;
  const int bj = t >> 4, bu = t & 15;
  const int wunit = tn * LS_UNITS + bu;
  const bool wok = wunit < H;

  f32x4_l acc = f32x4_l{0.f, 0.f, 0.f, 0.f};
  struct Stage {
    float4 ra[2];
    float w0, w1;
  };
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto load = [&](Stage& st, int gk) {
    const int k = gk * LS_BK + ak;
    const bool kok = k < K;  // K % 4 == 0: a float4 is inside or outside as a whole; the tail is zero-filled
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = m0 + ar + 32 * i;
      st.ra[i] = (kok && row < R) ? *reinterpret_cast<const float4*>(a.dg_next + (long long)row * K + k) : zero4;
    }
    const int kb = gk * LS_BK + 2 * bj;  // K is even: the pair is inside or outside as a whole
    const bool bok = wok && kb < K;
    st.w0 = bok ? a.w_hh[(long long)kb * H + wunit] : 0.f;
    st.w1 = bok ? a.w_hh[(long long)(kb + 1) * H + wunit] : 0.f;
  };
  auto store = [&](const Stage& st) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      unsigned lo[3], hi[3];
      split3_pair(st.ra[i].x, st.ra[i].y, lo);
      split3_pair(st.ra[i].z, st.ra[i].w, hi);
#pragma unroll
      for (int p = 0; p < 3; ++p)
        *reinterpret_cast<uint2*>(&Gs[p * LB_PLANE + (ar + 32 * i) * LS_LDW + ak / 2]) = make_uint2(lo[p], hi[p]);
    }
    unsigned wd[3];
    split3_pair(st.w0, st.w1, wd);
#pragma unroll
    for (int p = 0; p < 3; ++p) Gs[p * LB_PLANE + (LS_ROWS + bu) * LS_LDW + bj] = wd[p];
  };
  auto frag = [&](int row, bf16x8_l (&o)[3]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
      o[p] = __builtin_bit_cast(
          bf16x8_l, *reinterpret_cast<const u32x4_l*>(&Gs[p * LB_PLANE + row * LS_LDW + 4 * (lane >> 4)]));
  };
  auto compute = [&]() {
    bf16x8_l av[3], bv[3];
    frag(16 * w + (lane & 15), av);
    frag(LS_ROWS + (lane & 15), bv);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], bv[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], bv[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], bv[0], acc, 0, 0, 0);
  };
  static_assert(LS_DEPTH == 4, "four named stages below");
  Stage s0, s1, s2, s3;
  s0.ra[0] = s0.ra[1] = zero4;
  s0.w0 = s0.w1 = 0.f;
  s1 = s0;
  s2 = s0;
  s3 = s0;
  if (0 < ng) load(s0, g0);
  if (1 < ng) load(s1, g0 + 1);
  if (2 < ng) load(s2, g0 + 2);
  if (3 < ng) load(s3, g0 + 3);
  auto step = [&](Stage& st, int kt) {  // kt < ngmax: the same for the whole workgroup
    if (kt < ng) {
      store(st);
      if (kt + LS_DEPTH < ng) load(st, g0 + kt + LS_DEPTH);
    }
    __syncthreads();
    if (kt < ng) compute();
    __syncthreads();
  };
  for (int base = 0; base < ngmax; base += LS_DEPTH) {
    step(s0, base);
    if (base + 1 < ngmax) step(s1, base + 1);
    if (base + 2 < ngmax) step(s2, base + 2);
    if (base + 3 < ngmax) step(s3, base + 3);
  }
  // every k-group parks its sums in its own staging tile (wave w, lane l at (64 w + l) 4 + r)
  if (a.kt > 0) {  // uniform over the launch
    *reinterpret_cast<f32x4_l*>(&Gs[(w * 64 + lane) * 4]) = acc;
    __syncthreads();
  }

  // the cell, one (row, unit) per thread: lstm_cell_bwd_kernel's fp32 formulas
  const int lrow = tid >> 4, u = tn * LS_UNITS + (tid & 15), row = m0 + lrow;
  if (u >= H || row >= R) return;
  float dh = a.dh_lin ? a.dh_lin[(long long)row * a.ld_dh + u] : 0.f;
  if (a.kt > 0) {
    const int slot = ((lrow >> 4) * 64 + ((lrow & 15) >> 2) * 16 + (tid & 15)) * 4 + (lrow & 3);
    const float* sums = reinterpret_cast<const float*>(lds);
    float s = sums[slot];
#pragma unroll
    for (int k = 1; k < LS_KG; ++k) s += sums[k * LB_GBUF + slot];
    dh += s;
  }
  const long long i = (long long)row * H + u, o = (long long)row * K + u;
  float dc = a.dc_in ? a.dc_in[i] : 0.f;
  const float ig = a.act[o], fg = a.act[o + H], cg = a.act[o + 2 * H], og = a.act[o + 3 * H];
  const float tc = tanhf(a.c_cur[i]);
  const float d_o = dh * tc * og * (1.f - og);
  dc += dh * og * (1.f - tc * tc);
  const float d_i = dc * cg * ig * (1.f - ig);
  const float d_f = dc * (a.c_prev ? a.c_prev[i] : 0.f) * fg * (1.f - fg);
  const float d_g = dc * ig * (1.f - cg * cg);
  a.dgates[o] = d_i;
  a.dgates[o + H] = d_f;
  a.dgates[o + 2 * H] = d_g;
  a.dgates[o + 3 * H] = d_o;
  a.dc_out[i] = dc * fg;
}

int lstm_step_launch(const float* pre, long long ld_pre, const float* x, long long ld_x, int M, const float* h_prev,
                     long long ld_h, const float* c_prev, long long ld_c, const float* w_ih, const float* w_hh,
                     const float* b_ih, const float* b_hh, int R, int H, float* h_out, float* c_out, float* act_out,
                     bool train, void* stream) {
  CAPMI_REQUIRE(h_out && c_out && h_out != c_out && R > 0 && H > 0 && M >= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(M % 4 == 0 && H % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(pre || x || h_prev, CAPMI_EINVAL);
  CAPMI_REQUIRE(!pre || ld_pre >= 4LL * H, CAPMI_EINVAL);
  CAPMI_REQUIRE(!x || (w_ih && M > 0 && ld_x >= M && ld_x % 4 == 0 && aligned16(x) && aligned16(w_ih)), CAPMI_EINVAL);
  CAPMI_REQUIRE(!h_prev || (w_hh && ld_h >= H && ld_h % 4 == 0 && aligned16(h_prev) && aligned16(w_hh)),
                CAPMI_EINVAL);
  CAPMI_REQUIRE(!c_prev || ld_c >= H, CAPMI_EINVAL);
  CAPMI_REQUIRE(h_out != h_prev && h_out != c_prev && c_out != h_prev && c_out != c_prev, CAPMI_EINVAL);
  if (train)
    CAPMI_REQUIRE(act_out && act_out != h_out && act_out != c_out && act_out != pre && act_out != x &&
                      act_out != h_prev && act_out != c_prev,
                  CAPMI_EINVAL);
  CAPMI_REQUIRE(cdiv(R, LS_ROWS) <= 65535u, CAPMI_ERANGE);
  LsArgs a{};
  a.pre = pre, a.x = x, a.h_prev = h_prev, a.c_prev = c_prev;
  a.w_ih = w_ih, a.w_hh = w_hh, a.b_ih = b_ih, a.b_hh = b_hh;
  a.ld_pre = ld_pre, a.ld_x = ld_x, a.ld_h = ld_h, a.ld_c = ld_c;
  a.M = M, a.H = H, a.R = R;
  a.kt_x = x ? (int)cdiv(M, LS_BK) : 0;
  a.kt = a.kt_x + (h_prev ? (int)cdiv(H, LS_BK) : 0);
  a.h_out = h_out, a.c_out = c_out, a.act_out = act_out;
  const dim3 grid(cdiv(H, LS_UNITS), cdiv(R, LS_ROWS));
  if (train)
    hipLaunchKernelGGL(lstm_step_kernel<true>, grid, dim3(256 * LS_KG), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(lstm_step_kernel<false>, grid, dim3(256 * LS_KG), 0, as_stream(stream), a);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int capmi_lstm_step_fwd(const float* pre, long long ld_pre, const float* x, long long ld_x, int M,
                                   const float* h_prev, long long ld_h, const float* c_prev, long long ld_c,
                                   const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                                   int R, int H, float* h_out, float* c_out, void* stream) {
  return lstm_step_launch(pre, ld_pre, x, ld_x, M, h_prev, ld_h, c_prev, ld_c, w_ih, w_hh, b_ih, b_hh, R, H, h_out,
                          c_out, nullptr, false, stream);
}

extern "C" int capmi_lstm_step_fwd_train(const float* pre, long long ld_pre, const float* x, long long ld_x, int M,
                                         const float* h_prev, long long ld_h, const float* c_prev, long long ld_c,
                                         const float* w_ih, const float* w_hh, const float* b_ih,
                                         const float* b_hh, int R, int H, float* h_out, float* c_out,
                                         float* act_out, void* stream) {
  return lstm_step_launch(pre, ld_pre, x, ld_x, M, h_prev, ld_h, c_prev, ld_c, w_ih, w_hh, b_ih, b_hh, R, H, h_out,
                          c_out, act_out, true, stream);
}

extern "C" int capmi_lstm_step_bwd(const float* dh_lin, long long ld_dh, const float* dg_next, const float* w_hh,
                                   const float* dc_in, const float* act, const float* c_prev, const float* c_cur,
                                   int R, int H, float* dgates, float* dc_out, void* stream) {
  CAPMI_REQUIRE(act && c_cur && dgates && dc_out && R > 0 && H > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(H % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(!dh_lin || ld_dh >= H, CAPMI_EINVAL);
  CAPMI_REQUIRE(!dg_next || (w_hh && aligned16(dg_next)), CAPMI_EINVAL);
  const void* ins[] = {dh_lin, dg_next, w_hh, dc_in, act, c_prev, c_cur};
  for (const void* p : ins)
    CAPMI_REQUIRE((const void*)dgates != p && (const void*)dc_out != p, CAPMI_EINVAL);
  CAPMI_REQUIRE((void*)dgates != (void*)dc_out, CAPMI_EINVAL);
  CAPMI_REQUIRE(cdiv(R, LS_ROWS) <= 65535u, CAPMI_ERANGE);
  LbArgs a{};
  a.dh_lin = dh_lin, a.dg_next = dg_next, a.w_hh = w_hh, a.dc_in = dc_in;
  a.act = act, a.c_prev = c_prev, a.c_cur = c_cur;
  a.ld_dh = ld_dh, a.H = H, a.R = R;
  a.kt = dg_next ? (int)cdiv(4LL * H, LS_BK) : 0;
  a.dgates = dgates, a.dc_out = dc_out;
  hipLaunchKernelGGL(lstm_step_bwd_kernel, dim3(cdiv(H, LS_UNITS), cdiv(R, LS_ROWS)), dim3(256 * LS_KG), 0,
                     as_stream(stream), a);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

