// Teacher-forced validation (models/attention.py:454-567 for B captions at once): per-row loss, greedy
// token and target rank in one pass over the (B,T,V) logits, then the per-caption loss (CE mean over the
// caption's own rows + its doubly-stochastic regulariser) and top-1 / top-5 counts.
//
//   capmi_eval_rows     : one workgroup per row r = b*T + t; online max/sum as ce_rows_kernel (loss.hip), with the
//                         (value, index) arg-max and the target's rank carried through the same loop
//   capmi_eval_captions : one workgroup per caption, sums in a fixed order (bit-identical run to run)
//   capmi_eval_rows_at / capmi_eval_captions_ce : the same two for the baseline model's loss (reference
//                         models/baseline.py:267-374): target column t + tgt_off (there 0), no regulariser
//
// lens[b] is the caption's own decode length, not a per-step prefix count: captions come in any order.
#include <limits.h>

#include "common.h"

constexpr int EVAL_T = 256;  // threads per row / caption
constexpr int EVAL_W = EVAL_T / 64;

__device__ __forceinline__ int eval_len(const int* __restrict__ lens, int b, int T) {
  return lens ? min(max(lens[b], 0), T) : T;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide integer sum, red = LDS[>= 16] (block_sum's shape)
__device__ __forceinline__ int block_sum_i(int v, int* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_sum_i(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  int t = 0;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// (value, index) precedes (ov, oi): larger value, or equal with the lower index
__device__ __forceinline__ bool eval_before(float v, int i, float ov, int oi) {
  return v > ov || (v == ov && i < oi);
}

// VEC: V % 4 == 0 and a 16-byte aligned base, so every row is float4-addressable. A thread visits its
// columns in ascending order, so a strict '>' keeps the lowest index of its own maximum.
template <bool VEC>
__global__ void __launch_bounds__(EVAL_T) eval_rows_kernel(
    const float* __restrict__ logits, const long long* __restrict__ caps, int T, int L, int V, int tgt_off,
    const int* __restrict__ lens, float* __restrict__ loss_rows, int* __restrict__ pred,
    int* __restrict__ rank) {
  __shared__ float red[16];
  __shared__ int redi[16];
  __shared__ float rv[EVAL_W];
  __shared__ int rw[EVAL_W];
  const int r = blockIdx.x;  // r = b*T + t
  const int b = r / T, t = r - b * T;
  if (t >= eval_len(lens, b, T)) {
    if (threadIdx.x == 0) {
      loss_rows[r] = 0.f;
      pred[r] = -1;
      if (rank) rank[r] = -1;
    }
    return;
  }
  const float* x = logits + (long long)r * V;
  const long long tgt = caps[(long long)b * L + t + tgt_off];
  const bool in_range = tgt >= 0 && tgt < V;
  const int itgt = in_range ? (int)tgt : 0;
  const float xt = in_range ? x[itgt] : INFINITY;  // every thread the same address: one broadcast load
  float m = -INFINITY, s = 0.f;
  int mi = INT_MAX, cnt = 0;
  auto visit = [&](float xv, int v) {
    if (xv > m) {
      s = s * expf(m - xv) + 1.f;
      m = xv;
      mi = v;
    } else if (m > -INFINITY) {
      s += expf(xv - m);
    }
    cnt += (xv > xt || (xv == xt && v < itgt)) ? 1 : 0;
  };
  if (VEC) {
    for (int v = threadIdx.x * 4; v < V; v += EVAL_T * 4) {
      const float4 q = *reinterpret_cast<const float4*>(x + v);
      visit(q.x, v);
      visit(q.y, v + 1);
      visit(q.z, v + 2);
      visit(q.w, v + 3);
    }
  } else {
    for (int v = threadIdx.x; v < V; v += EVAL_T) visit(x[v], v);
  }
  // arg-max: wave butterfly, then the EVAL_W wave winners in LDS
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float bv = m;
  int bw = mi;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int ow = __shfl_xor(bw, o, 64);
    if (eval_before(ov, ow, bv, bw)) {
      bv = ov;
      bw = ow;
    }
  }
  if (lane == 0) {
    rv[wid] = bv;
    rw[wid] = bw;
  }
  __syncthreads();
  bv = rv[0];
  bw = rw[0];
#pragma unroll
  for (int q = 1; q < EVAL_W; ++q)
    if (eval_before(rv[q], rw[q], bv, bw)) {
      bv = rv[q];
      bw = rw[q];
    }
  const float gm = bv;  // the row maximum
  s = (m == -INFINITY) ? 0.f : s * expf(m - gm);
  s = block_sum(s, red);
  cnt = block_sum_i(cnt, redi);
  if (threadIdx.x == 0) {
    loss_rows[r] = in_range ? (gm + logf(s)) - xt : INFINITY;
    pred[r] = bw < V ? bw : 0;  // no finite / comparable logit (all -inf or NaN): keep a valid index
    if (rank) rank[r] = in_range ? cnt : V;
  }
}

// the launch behind both entry points: the target of row (b, t) is caps[b*L + t + tgt_off]
static int eval_rows_launch(const float* logits, const long long* caps, int B, int T, int L, int V, int tgt_off,
                            const int* lens, float* loss_rows, int* pred, int* rank, void* stream) {
  const hipStream_t st = as_stream(stream);
  if (V % 4 == 0 && aligned16(logits))
    hipLaunchKernelGGL(eval_rows_kernel<true>, dim3(B * T), dim3(EVAL_T), 0, st, logits, caps, T, L, V, tgt_off,
                       lens, loss_rows, pred, rank);
  else
    hipLaunchKernelGGL(eval_rows_kernel<false>, dim3(B * T), dim3(EVAL_T), 0, st, logits, caps, T, L, V, tgt_off,
                       lens, loss_rows, pred, rank);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_eval_rows(const float* logits, const long long* caps, int B, int T, int L, int V,
                               const int* lens, float* loss_rows, int* pred, int* rank, void* stream) {
  CAPMI_REQUIRE(logits && caps && loss_rows && pred, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && T > 0 && V > 0 && L > T && (long long)B * T <= INT_MAX, CAPMI_EINVAL);
  return eval_rows_launch(logits, caps, B, T, L, V, 1, lens, loss_rows, pred, rank, stream);
}

extern "C" int capmi_eval_rows_at(const float* logits, const long long* caps, int B, int T, int L, int V,
                                  int tgt_off, const int* lens, float* loss_rows, int* pred, int* rank,
                                  void* stream) {
  CAPMI_REQUIRE(logits && caps && loss_rows && pred, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && T > 0 && V > 0 && tgt_off >= 0 && (long long)L >= (long long)T + tgt_off &&
                    (long long)B * T <= INT_MAX,
                CAPMI_EINVAL);
  return eval_rows_launch(logits, caps, B, T, L, V, tgt_off, lens, loss_rows, pred, rank, stream);
}

// --------------------------------------------------------------------------------------
// per caption: CE mean over its n rows, regulariser over its P positions (the t sum stops at n: alpha rows
// past the caption's end are never read), top-1 / top-5 counts. Thread -> element assignment and the
// reduction trees are fixed, so two runs give the same bits.
// --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EVAL_T) eval_captions_kernel(
    const float* __restrict__ loss_rows, const int* __restrict__ rank, const float* __restrict__ alphas,
    const int* __restrict__ lens, int T, int P, float alpha_c, float* __restrict__ cap_ce,
    float* __restrict__ cap_reg, float* __restrict__ cap_loss, int* __restrict__ cap_top1,
    int* __restrict__ cap_top5) {
  __shared__ float red[16];
  __shared__ int redi[16];
  const int b = blockIdx.x;
  const int n = eval_len(lens, b, T);
  if (n == 0) {
    if (threadIdx.x == 0) {
      cap_ce[b] = 0.f;
      cap_reg[b] = 0.f;
      cap_loss[b] = 0.f;
      cap_top1[b] = 0;
      cap_top5[b] = 0;
    }
    return;
  }
  const long long row0 = (long long)b * T;
  float ce = 0.f;
  int c1 = 0, c5 = 0;
  for (int t = threadIdx.x; t < n; t += EVAL_T) {
    ce += loss_rows[row0 + t];
    const int rk = rank[row0 + t];
    c1 += rk == 0 ? 1 : 0;
    c5 += (rk >= 0 && rk < 5) ? 1 : 0;
  }
  ce = block_sum(ce, red) / (float)n;
  c1 = block_sum_i(c1, redi);
  c5 = block_sum_i(c5, redi);
  float acc = 0.f;
  for (int p = threadIdx.x; p < P; p += EVAL_T) {
    const float* a = alphas + row0 * P + p;
    float s = 0.f;
    for (int t = 0; t < n; ++t) s += a[(long long)t * P];
    const float d = alpha_c - s;
    acc += d * d;
  }
  const float reg = block_sum(acc, red) / (float)P;
  if (threadIdx.x == 0) {
    cap_ce[b] = ce;
    cap_reg[b] = reg;
    cap_loss[b] = ce + reg;
    cap_top1[b] = c1;
    cap_top5[b] = c5;
  }
}

extern "C" int capmi_eval_captions(const float* loss_rows, const int* rank, const float* alphas,
                                   const int* lens, int B, int T, int P, float alpha_c, float* cap_ce,
                                   float* cap_reg, float* cap_loss, int* cap_top1, int* cap_top5,
                                   void* stream) {
  CAPMI_REQUIRE(loss_rows && rank && alphas && cap_ce && cap_reg && cap_loss && cap_top1 && cap_top5,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && T > 0 && P > 0 && (long long)B * T <= INT_MAX, CAPMI_EINVAL);
  hipLaunchKernelGGL(eval_captions_kernel, dim3(B), dim3(EVAL_T), 0, as_stream(stream), loss_rows, rank,
                     alphas, lens, T, P, alpha_c, cap_ce, cap_reg, cap_loss, cap_top1, cap_top5);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

// --------------------------------------------------------------------------------------
// per caption without the attention regulariser (the baseline model's validation loss is the plain CE mean):
// eval_captions_kernel's CE and count sums, thread -> element assignment and trees unchanged
// --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EVAL_T) eval_captions_ce_kernel(
    const float* __restrict__ loss_rows, const int* __restrict__ rank, const int* __restrict__ lens, int T,
    float* __restrict__ cap_ce, int* __restrict__ cap_top1, int* __restrict__ cap_top5) {
  __shared__ float red[16];
  __shared__ int redi[16];
  const int b = blockIdx.x;
  const int n = eval_len(lens, b, T);
  if (n == 0) {
    if (threadIdx.x == 0) {
      cap_ce[b] = 0.f;
      cap_top1[b] = 0;
      cap_top5[b] = 0;
    }
    return;
  }
  const long long row0 = (long long)b * T;
  float ce = 0.f;
  int c1 = 0, c5 = 0;
  for (int t = threadIdx.x; t < n; t += EVAL_T) {
    ce += loss_rows[row0 + t];
    const int rk = rank[row0 + t];
    c1 += rk == 0 ? 1 : 0;
    c5 += (rk >= 0 && rk < 5) ? 1 : 0;
  }
  ce = block_sum(ce, red) / (float)n;
  c1 = block_sum_i(c1, redi);
  c5 = block_sum_i(c5, redi);
  if (threadIdx.x == 0) {
    cap_ce[b] = ce;
    cap_top1[b] = c1;
    cap_top5[b] = c5;
  }
}

extern "C" int capmi_eval_captions_ce(const float* loss_rows, const int* rank, const int* lens, int B, int T,
                                      float* cap_ce, int* cap_top1, int* cap_top5, void* stream) {
  CAPMI_REQUIRE(loss_rows && rank && cap_ce && cap_top1 && cap_top5, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && T > 0 && (long long)B * T <= INT_MAX, CAPMI_EINVAL);
  hipLaunchKernelGGL(eval_captions_ce_kernel, dim3(B), dim3(EVAL_T), 0, as_stream(stream), loss_rows, rank, lens,
                     T, cap_ce, cap_top1, cap_top5);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
