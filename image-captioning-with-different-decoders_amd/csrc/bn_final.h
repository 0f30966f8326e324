// Train-mode BatchNorm finalize: per-slice (Σ, Σx²) of a conv output -> scale / shift (+ batch mean / var,
// running-stat update), models/encoder.py:97-107 (torchvision BN in train mode, momentum 0.1, unbiased
// running variance). Round 4: one canonical fp64 summation order, independent of the launch shape, that
// the host can restate op for op (tests/test_gpu_bn_final.py).
//
// Canonical order for channel c over the T statistic slices (rows of stats[T][C][2]):
//   q_l = sum of slice t = l, l + 64, l + 128, ... in ascending t   (l = 0..63, fp64)
//   r_w = q_8w + q_8w+1 + ... + q_8w+7                                 (w = 0..7, in order)
//   sum = r_0 + r_1 + ... + r_7                                        (in order)
// Threads: a wave covers 8 channels x 8 slice lanes (one 64-B row segment per slice); the 64 lane groups
// l = 8 w + s of a channel are 8 (virtual) waves w x 8 lanes s.
#pragma once
#include "common.h"

constexpr int BNF_CG = 8;  // channels per finalize group
constexpr int BNF_DEPTH = 16;  // slices a lane has in flight per batch (32 measured slower: DESIGN 4.26)
constexpr int BNF_TAIL = 4;    // the short last batch (at most 64 BNF_TAIL slices left: layer3 and layer4)

struct BnFinArgs {
  const float* gamma;
  const float* beta;
  float* running_mean;
  float* running_var;
  float* scale;
  float* shift;
  float* save_mean;
  float* save_var;
  float momentum, eps;
  long long count;
};

// gamma / beta / running statistics of one channel, requested at kernel entry by the thread that applies them
struct BnFinParams {
  float gamma, beta, rm, rv;
};

__device__ __forceinline__ BnFinParams bnf_params(const BnFinArgs& f, int c) {
  BnFinParams p;
  p.gamma = f.gamma[c];
  p.beta = f.beta[c];
  p.rm = f.running_mean ? f.running_mean[c] : 0.f;
  p.rv = f.running_mean ? f.running_var[c] : 0.f;
  return p;
}

// every operation rounded on its own (no contraction into fma): the result is a function of the sums alone,
// reproducible by any IEEE implementation (tests/test_gpu_bn_final.py)
__device__ __forceinline__ void bnf_apply(const BnFinArgs& f, const BnFinParams& p, int c, double s, double q) {
#pragma clang fp contract(off)
  float ga = p.gamma, be = p.beta, rm = p.rm, rv = p.rv;
  asm volatile("" : "+v"(ga), "+v"(be), "+v"(rm), "+v"(rv));  // consumed here, not where they were requested
  const double n = (double)f.count;
  const double mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0) var = 0;
  const double inv = 1.0 / sqrt(var + (double)f.eps);
  const float sc = (float)((double)ga * inv);
  f.scale[c] = sc;
  f.shift[c] = (float)((double)be - mean * (double)sc);
  if (f.save_mean) f.save_mean[c] = (float)mean;
  if (f.save_var) f.save_var[c] = (float)var;
  if (f.running_mean) {
    const double unb = f.count > 1 ? var * n / (n - 1.0) : var;
    f.running_mean[c] = (1.f - f.momentum) * rm + f.momentum * (float)mean;
    f.running_var[c] = (1.f - f.momentum) * rv + f.momentum * (float)unb;
  }
}

// D slices t, t + 64, ... of one lane: every load is issued before the first add, then the adds run in slice
// order. PRED: slots at or past T re-read slice t (a valid address, the line of slot 0: no branch around a
// load, which would put a wait behind each) and are left out of the add chain, so the association is that of
// the plain sequential sum for every T. The caller guarantees t < T.
template <int D, bool PRED>
__device__ __forceinline__ void bnf_batch(const float2* __restrict__ p, int t, int T, int C, double& sm,
                                          double& sq) {
#pragma clang fp contract(off)
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p) + (long long)t * C;
  const long long step = 64LL * C;
  unsigned long long v[D];  // (sum, sum of squares) of a slice as one register pair
#pragma unroll
  for (int u = 0; u < D; ++u) {
    long long off = (!PRED || t + 64 * u < T) ? u * step : 0;
    // opaque: seeing a second load of slot 0, the compiler would branch around it and wait for the first
    if (PRED) asm("" : "+v"(off));
    v[u] = q[off];
  }
  // nothing that consumes a value (its conversion to fp64 included) is scheduled among the loads
#pragma unroll
  for (int u = 0; u < D; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
  for (int u = 0; u < D; ++u) {
    if (!PRED || t + 64 * u < T) {
      sm += __uint_as_float((unsigned)v[u]);
      sq += __uint_as_float((unsigned)(v[u] >> 32));
    }
  }
}

// Finalize channel group g (channels [8 g, 8 g + 8) below C) with the calling workgroup's NT threads.
// scratch: 72 x 8 double2 in LDS (9 KiB), free on entry; the workgroup meets three times.
// The critical path is one memory round trip per batch of BNF_DEPTH slices per lane (one in all for
// T <= 64 BNF_DEPTH, i.e. every layer2-4 shape at batch 64), three barriers and the fp64 arithmetic.
template <int NT>
__device__ __forceinline__ void bnf_group(const BnFinArgs& f, const float* __restrict__ stats, int T, int C, int g,
                                          double2* scratch) {
  static_assert(NT % 64 == 0 && NT <= 512, "whole waves, at most 8");
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, cl = lane & 7, s = lane >> 3;
  const int c = g * BNF_CG + cl;
  // The applying threads ask for their channel's parameters first, so that the loads travel with the
  // statistics' instead of four serial round trips at the end. Reading running_mean / running_var this early
  // is safe: within a launch a channel's running statistics are read and written by this one thread only.
  const bool applies = tid < BNF_CG && c < C;  // tid < 8: cl == tid
  BnFinParams prm{};
  if (applies) prm = bnf_params(f, c);
#pragma unroll
  for (int vw = w; vw < 8; vw += NT / 64) {
    const int l = vw * 8 + s;
    double sm = 0.0, sq = 0.0;
    if (c < C) {
      const float2* p = reinterpret_cast<const float2*>(stats) + c;
      int base = 0;  // workgroup-uniform: the lane's slice is base + l
      for (; base + BNF_DEPTH * 64 <= T; base += BNF_DEPTH * 64) bnf_batch<BNF_DEPTH, false>(p, base + l, T, C, sm, sq);
      if (base + l < T) {  // the remainder, fewer than BNF_DEPTH slices: one predicated batch, short or full
        if (T - base <= BNF_TAIL * 64) bnf_batch<BNF_TAIL, true>(p, base + l, T, C, sm, sq);
        else bnf_batch<BNF_DEPTH, true>(p, base + l, T, C, sm, sq);
      }
    }
    scratch[l * BNF_CG + cl] = make_double2(sm, sq);
  }
  __syncthreads();
  if (tid < 64) {  // r_w for (w, channel) = (tid / 8, tid % 8): two serial chains of 8 instead of one of 64
    const int w8 = tid >> 3, cc = tid & 7;
    double sm = 0.0, sq = 0.0;
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const double2 v = scratch[(8 * w8 + s8) * BNF_CG + cc];
      sm += v.x;
      sq += v.y;
    }
    scratch[(64 + w8) * BNF_CG + cc] = make_double2(sm, sq);
  }
  __syncthreads();
  if (applies) {
    double sm = 0.0, sq = 0.0;
#pragma unroll
    for (int w8 = 0; w8 < 8; ++w8) {
      const double2 v = scratch[(64 + w8) * BNF_CG + tid];
      sm += v.x;
      sq += v.y;
    }
    bnf_apply(f, prm, c, sm, sq);
  }
  __syncthreads();
}
