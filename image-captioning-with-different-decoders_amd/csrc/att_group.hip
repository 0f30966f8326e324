// Attention backward over row groups that share one image's features: the teacher-forced pass over the
// R = B*n sampled captions of self-critical training (capmi/decoder_group.py). The forward side is
// capmi_beam_att_fwd (beam.hip); this file is its backward.
//
// Row layout (the sampler's, beam.hip's): image i owns rows i*n .. i*n+n-1, 1 <= n <= 16, every row live.
//
//   capmi_att_group_bwd      : the arithmetic of att_ctx_bwd + att_score_bwd (decoder.hip) per row, without dreg
//                              and bt, but one workgroup serves all n rows of an image: each enc / att_enc
//                              element it needs is loaded once and used for n rows (no n-fold copy of either)
//   capmi_att_group_enc_grad : att_enc_grad hoisted over all t AND the n rows of the image; the T*n att_dec
//                              rows of a group do not fit in LDS, so they are staged in chunks of (t, j) pairs
//
// Every sum has one fixed order that does not depend on n or on the row's place in its group (a row alone in
// its own image computes the same bits as inside a group); there are no float atomics.
#include "common.h"

constexpr int GRP_NMAX = 16;

// acc + a . b as four explicit fused multiply-adds in element order: the 4 / 8 / 16-row instantiations are
// optimised separately, and a product-sum left to the compiler's contraction came out with other roundings in
// one arm than in another
__device__ __forceinline__ float dot4_acc(float4 a, float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// --------------------------------------------------------------------------------------
// d = sum of the split-K slabs of d(gate*awe); dawe = d*gate -> LDS [n][E]; dgp = d*awe*gate*(1-gate);
// dalpha[row][p] = dawe[row] . enc[i][p][:]                                   grid (cdiv(P, GRP_PCH), B)
// a wave owns slots p0+wid, p0+wid+4, ...: each enc float4 is loaded once and dotted against the dawe of all n
// rows (R*KM accumulators per lane). A (slot, row) sum is one wave's: lane partials over c ascending, wave_sum.
// --------------------------------------------------------------------------------------
constexpr int GRP_PCH = 13;

template <int KM>
__global__ void __launch_bounds__(256) group_ctx_bwd_kernel(
    const float* __restrict__ part, int S, long long slab, const float* __restrict__ gate,
    const float* __restrict__ awe, const float* __restrict__ enc, int n, int P, int E,
    float* __restrict__ dgp, float* __restrict__ dalpha) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // dawe [n][E]
  const int i = blockIdx.y, p0 = blockIdx.x * GRP_PCH;
  const long long row0 = (long long)i * n;
  const int E4 = E / 4;
  for (int t = threadIdx.x; t < n * E4; t += 256) {
    const int j = t / E4, c = (t - j * E4) * 4;
    const long long o = (row0 + j) * E + c;
    const float4 d = slab_sum(reinterpret_cast<const float4*>(part + slab + o), S - 1, slab / 4,
                              *reinterpret_cast<const float4*>(part + o));
    const float4 g = *reinterpret_cast<const float4*>(gate + o);
    if (blockIdx.x == 0) {
      const float4 a = *reinterpret_cast<const float4*>(awe + o);
      float4 r;
      r.x = d.x * a.x * g.x * (1.f - g.x);
      r.y = d.y * a.y * g.y * (1.f - g.y);
      r.z = d.z * a.z * g.z * (1.f - g.z);
      r.w = d.w * a.w * g.w * (1.f - g.w);
      *reinterpret_cast<float4*>(dgp + o) = r;
    }
    *reinterpret_cast<float4*>(smem + (long long)j * E + c) = d * g;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int pend = min(P, p0 + GRP_PCH);
  constexpr int R = (GRP_PCH + 3) / 4;
  const float* base = enc + ((long long)i * P + p0 + wid) * E;
  float acc[R][KM];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < KM; ++j) acc[r][j] = 0.f;
  for (int c = lane * 4; c < E; c += 256) {
    float4 x[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      x[r] = p0 + wid + 4 * r < pend ? *reinterpret_cast<const float4*>(base + (long long)4 * r * E + c) : f4(0.f);
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < n) {
        const float4 d = *reinterpret_cast<const float4*>(smem + (long long)j * E + c);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][j] = dot4_acc(x[r], d, acc[r][j]);
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = p0 + wid + 4 * r;
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < n && p < pend) {
        const float v = wave_sum(acc[r][j]);
        if (lane == 0) dalpha[(row0 + j) * P + p] = v;
      }
  }
}

// --------------------------------------------------------------------------------------
// softmax backward + ReLU-score backward of the n rows of image i               grid (cdiv(A, 64), B)
// de: one wave per row (rows wid, wid+4, ...), so a row's de does not depend on its position. dad: 16 lanes x
// float4 cover the block's 64 columns, 16 slot groups stride over P; each att_enc float4 is loaded once and
// masked against the att_dec of every row. The 16 group partials are summed in group order, four rows a round.
// --------------------------------------------------------------------------------------
template <int KM>
__global__ void __launch_bounds__(256) group_score_bwd_kernel(
    const float* __restrict__ dalpha, const float* __restrict__ alpha, long long alpha_ld,
    const float* __restrict__ att_enc, const float* __restrict__ att_dec, const float* __restrict__ wf, int n,
    int P, int A, float* __restrict__ de, float* __restrict__ dad) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // des [n][P4]
  __shared__ float4 part4[4 * 256];
  const int P4 = (P + 3) & ~3;
  const int i = blockIdx.y, tid = threadIdx.x;
  const long long row0 = (long long)i * n;
  const int lane = tid & 63, wid = tid >> 6;
  for (int j = wid; j < n; j += 4) {
    const float* da = dalpha + (row0 + j) * P;
    const float* al = alpha + (row0 + j) * alpha_ld;
    float* des = smem + j * P4;
    float s = 0.f;
    for (int p = lane; p < P; p += 64) {
      const float v = da[p];
      des[p] = v;
      s = fmaf(al[p], v, s);
    }
    s = wave_sum(s);
    for (int p = lane; p < P; p += 64) {
      const float v = al[p] * (des[p] - s);
      des[p] = v;
      if (blockIdx.x == 0) de[(row0 + j) * P + p] = v;
    }
  }
  __syncthreads();
  const int c4 = tid & 15, pg = tid >> 4;
  const int a = blockIdx.x * 64 + c4 * 4;
  float4 acc[KM], ad[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    acc[j] = f4(0.f);
    ad[j] = (a < A && j < n) ? *reinterpret_cast<const float4*>(att_dec + (row0 + j) * A + a) : f4(0.f);
  }
  if (a < A) {
    const float* base = att_enc + (long long)i * P * A + a;
#pragma unroll 2
    for (int p = pg; p < P; p += 16) {
      const float4 x = *reinterpret_cast<const float4*>(base + (long long)p * A);
#pragma unroll
      for (int j = 0; j < KM; ++j)
        if (j < n) {
          const float4 s = x + ad[j];
          const float d = smem[j * P4 + p];
          acc[j].x += s.x > 0.f ? d : 0.f;
          acc[j].y += s.y > 0.f ? d : 0.f;
          acc[j].z += s.z > 0.f ? d : 0.f;
          acc[j].w += s.w > 0.f ? d : 0.f;
        }
    }
  }
#pragma unroll
  for (int jb = 0; jb < KM; jb += 4) {
    if (jb < n) {  // n is uniform over the workgroup: every thread takes the same barriers
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) part4[jj * 256 + tid] = acc[jb + jj];
      __syncthreads();
      if (tid < 64) {
        const int jj = tid >> 4, c = tid & 15, j = jb + jj;
        const int a0 = blockIdx.x * 64 + c * 4;
        if (j < n && a0 < A) {
          float4 tot = part4[jj * 256 + c];
          for (int g = 1; g < 16; ++g) tot = tot + part4[jj * 256 + g * 16 + c];
          const float4 w = *reinterpret_cast<const float4*>(wf + a0);
          *reinterpret_cast<float4*>(dad + (row0 + j) * A + a0) = w * tot;
        }
      }
      __syncthreads();
    }
  }
}

template <int KM>
static int group_bwd_launch(const float* dx_part, int S, long long slab, const float* gate, const float* awe,
                            const float* enc, const float* alpha, long long alpha_ld, const float* att_enc,
                            const float* att_dec, const float* wf, int B, int n, int P, int A, int E,
                            float* dalpha_ws, float* dgp, float* de, float* dad, hipStream_t st) {
  const size_t sh_c = (size_t)n * E * sizeof(float);
  const size_t sh_s = (size_t)n * ((P + 3) & ~3) * sizeof(float);
  CAPMI_REQUIRE(sh_c <= 144 * 1024 && sh_s <= 48 * 1024, CAPMI_ERANGE);
  if (sh_c > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)group_ctx_bwd_kernel<KM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)sh_c);
  hipLaunchKernelGGL(group_ctx_bwd_kernel<KM>, dim3(cdiv(P, GRP_PCH), B), dim3(256), sh_c, st, dx_part, S, slab,
                     gate, awe, enc, n, P, E, dgp, dalpha_ws);
  CAPMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_score_bwd_kernel<KM>, dim3(cdiv(A, 64), B), dim3(256), sh_s, st, dalpha_ws, alpha,
                     alpha_ld, att_enc, att_dec, wf, n, P, A, de, dad);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_att_group_bwd(const float* dx_part, int S, long long slab, const float* gate,
                                   const float* awe, const float* enc, const float* alpha, long long alpha_ld,
                                   const float* att_enc, const float* att_dec, const float* wf, int B, int n,
                                   int P, int A, int E, float* dalpha_ws, float* dgp, float* de, float* dad,
                                   void* stream) {
  CAPMI_REQUIRE(dx_part && gate && awe && enc && alpha && att_enc && att_dec && wf, CAPMI_EINVAL);
  CAPMI_REQUIRE(dalpha_ws && dgp && de && dad, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && P > 0 && A > 0 && E > 0 && S >= 1 && n >= 1 && n <= GRP_NMAX && alpha_ld >= P,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(A % 4 == 0 && E % 4 == 0 && slab % 4 == 0 && B <= 65535, CAPMI_ERANGE);
  CAPMI_REQUIRE(aligned16(dx_part) && aligned16(gate) && aligned16(awe) && aligned16(enc) && aligned16(att_enc) &&
                    aligned16(att_dec) && aligned16(wf) && aligned16(dgp) && aligned16(dad),
                CAPMI_EALIGN);
  const hipStream_t st = as_stream(stream);
#define GROUP_BWD(KM)                                                                                           \
  return group_bwd_launch<KM>(dx_part, S, slab, gate, awe, enc, alpha, alpha_ld, att_enc, att_dec, wf, B, n, P, \
                              A, E, dalpha_ws, dgp, de, dad, st)
  if (n <= 4) GROUP_BWD(4);
  if (n <= 8) GROUP_BWD(8);
  GROUP_BWD(16);
#undef GROUP_BWD
}

// --------------------------------------------------------------------------------------
// hoisted d(att_enc) over all (t, j) + full_att weight / bias partials          grid (cdiv(P, GRP_EPCH), B)
// 1024 threads = A/4 float4 columns x (1024 / (A/4)) slot groups; a thread keeps the att_enc float4 and the
// gradient accumulator of its <= GRP_NPP slots in registers for the whole kernel. The Q = T*n (t, j) pairs of
// the image, q = t*n + j, are staged CH at a time (att_dec rows [CH][A] and de [CH][GRP_EPCH] in LDS, CH*A <=
// 8192 floats) and consumed in ascending q: the order t ascending, then j ascending, whatever CH is.
// --------------------------------------------------------------------------------------
constexpr int GRP_EPCH = 28;
constexpr int GRP_ET = 1024;
constexpr int GRP_NPP = 7;  // slots per thread: A/4 <= 256 leaves >= 4 slot groups, 4 * 7 = 28

__global__ void __launch_bounds__(GRP_ET) group_enc_grad_kernel(
    const float* __restrict__ de, const float* __restrict__ att_enc, const float* __restrict__ att_dec,
    const float* __restrict__ wf, int T, int R, int n, int P, int A, int CH, float* __restrict__ datt_enc,
    float* __restrict__ wf_part, float* __restrict__ bf_part) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ads = smem;                       // [CH][A]
  float* des = smem + (long long)CH * A;   // [CH][GRP_EPCH]
  float* wred = des + CH * GRP_EPCH;       // [GRP_ET][4], 16-byte aligned: CH * A and CH * 28 are multiples of 4
  const int i = blockIdx.y, p0 = blockIdx.x * GRP_EPCH, tid = threadIdx.x;
  const int np = min(GRP_EPCH, P - p0);
  const long long row0 = (long long)i * n;
  const int A4 = A / 4, Q = T * n;
  const int ngrp = GRP_ET / A4;
  const int c4 = tid % A4, pg = tid / A4;
  const bool worker = pg < ngrp;
  const int a = c4 * 4;
  float4 x[GRP_NPP], g[GRP_NPP];
#pragma unroll
  for (int k = 0; k < GRP_NPP; ++k) {
    const int pp = pg + k * ngrp;
    g[k] = f4(0.f);
    x[k] = (worker && pp < np) ? *reinterpret_cast<const float4*>(att_enc + ((long long)i * P + p0 + pp) * A + a)
                               : f4(0.f);
  }
  float4 wacc = f4(0.f);
  float bacc = 0.f;
  for (int q0 = 0; q0 < Q; q0 += CH) {
    const int nq = min(CH, Q - q0);
    for (int t = tid; t < nq * A4; t += GRP_ET) {
      const int qq = t / A4, cc = (t - qq * A4) * 4;
      const int q = q0 + qq, tt = q / n, j = q - tt * n;
      *reinterpret_cast<float4*>(ads + qq * A + cc) =
          *reinterpret_cast<const float4*>(att_dec + ((long long)tt * R + row0 + j) * A + cc);
    }
    for (int t = tid; t < nq * GRP_EPCH; t += GRP_ET) {
      const int qq = t / GRP_EPCH, pp = t - qq * GRP_EPCH;
      const int q = q0 + qq, tt = q / n, j = q - tt * n;
      des[t] = pp < np ? de[((long long)tt * R + row0 + j) * P + p0 + pp] : 0.f;
    }
    __syncthreads();
    if (worker) {
      for (int qq = 0; qq < nq; ++qq) {
        const float4 adv = *reinterpret_cast<const float4*>(ads + qq * A + a);
#pragma unroll
        for (int k = 0; k < GRP_NPP; ++k) {
          const int pp = pg + k * ngrp;
          if (pp < np) {
            const float d = des[qq * GRP_EPCH + pp];
            const float4 s = x[k] + adv;
            g[k].x += s.x > 0.f ? d : 0.f;
            g[k].y += s.y > 0.f ? d : 0.f;
            g[k].z += s.z > 0.f ? d : 0.f;
            g[k].w += s.w > 0.f ? d : 0.f;
            wacc = fma4(f4(d), relu4(s), wacc);
          }
        }
      }
    }
    if (tid < GRP_EPCH)
      for (int qq = 0; qq < nq; ++qq) bacc += des[qq * GRP_EPCH + tid];
    __syncthreads();
  }
  if (worker) {
    const float4 w = *reinterpret_cast<const float4*>(wf + a);
#pragma unroll
    for (int k = 0; k < GRP_NPP; ++k) {
      const int pp = pg + k * ngrp;
      if (pp < np) *reinterpret_cast<float4*>(datt_enc + ((long long)i * P + p0 + pp) * A + a) = g[k] * w;
    }
  }
  // the slot groups sharing a column are summed in group order; the 28 per-slot de sums in slot order
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  reinterpret_cast<float4*>(wred)[tid] = wacc;
  __syncthreads();
  if (tid < A4) {
    float4 s = reinterpret_cast<float4*>(wred)[tid];
    for (int gI = 1; gI < ngrp; ++gI) s = s + reinterpret_cast<float4*>(wred)[gI * A4 + tid];
    *reinterpret_cast<float4*>(wf_part + (long long)blk * A + tid * 4) = s;
  }
  __syncthreads();
  if (tid < GRP_EPCH) wred[tid] = bacc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int pp = 0; pp < GRP_EPCH; ++pp) s += wred[pp];
    bf_part[blk] = s;
  }
}

extern "C" int capmi_att_group_enc_grad(const float* de, const float* att_enc, const float* att_dec,
                                        const float* wf, int T, int B, int n, int P, int A, float* datt_enc,
                                        float* wf_part, float* bf_part, int* nblk_out, void* stream) {
  CAPMI_REQUIRE(de && att_enc && att_dec && wf && datt_enc && wf_part && bf_part, CAPMI_EINVAL);
  CAPMI_REQUIRE(T > 0 && B > 0 && P > 0 && A > 0 && n >= 1 && n <= GRP_NMAX, CAPMI_EINVAL);
  CAPMI_REQUIRE(A % 4 == 0 && A / 4 <= 256 && B <= 65535 && (long long)B * n <= INT32_MAX && T <= 65535,
                CAPMI_ERANGE);
  CAPMI_REQUIRE(aligned16(att_enc) && aligned16(att_dec) && aligned16(wf) && aligned16(datt_enc) &&
                    aligned16(wf_part),
                CAPMI_EALIGN);
  const int Q = T * n;
  const int CH = std::max(1, std::min(std::min(Q, 64), 8192 / A));
  const size_t sh = ((size_t)CH * A + (size_t)CH * GRP_EPCH + GRP_ET * 4) * sizeof(float);  // <= 55.0 KiB
  const dim3 grid(cdiv(P, GRP_EPCH), B);
  if (nblk_out) *nblk_out = (int)(grid.x * grid.y);
  hipLaunchKernelGGL(group_enc_grad_kernel, grid, dim3(GRP_ET), sh, as_stream(stream), de, att_enc, att_dec, wf, T,
                     B * n, n, P, A, CH, datt_enc, wf_part, bf_part);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
