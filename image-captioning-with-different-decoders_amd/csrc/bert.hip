// The non-GEMM kernels of the frozen BERT encoder forward (capmi/bert.py): embedding + LayerNorm, ragged
// short-sequence multi-head attention, bias + GELU (erf form), add + LayerNorm and the piece -> word segment
// sum. fp32 throughout; the GEMMs between them are capmi_gemm_sk_ex's.
#include "common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int BERT_MAX_HIDDEN = 8192;  // the row lives in LDS: 32 KiB
constexpr int ATT_D = 64;              // head dim (the only BERT geometry)
constexpr int ATT_BLOCK = 64;          // queries per workgroup (one per lane) and keys per LDS block
constexpr int ATT_MAX_SEQ = 512;

// LayerNorm of the row held in LDS (`row`, H % 4 == 0): two passes over LDS (mean, then the centred sum of
// squares), fp32 statistics; every thread returns with the normalised row written to `out`.
__device__ __forceinline__ void ln_row_store(const float* row, int H, float part, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, float eps, float* __restrict__ out,
                                             float* red) {
  const float mean = block_sum(part, red) / (float)H;
  float sq = 0.f;
  for (int c = threadIdx.x * 4; c < H; c += LN_THREADS * 4) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    const float a = v.x - mean, b = v.y - mean, d = v.z - mean, e = v.w - mean;
    sq += (a * a + b * b) + (d * d + e * e);
  }
  const float var = block_sum(sq, red) / (float)H;
  const float rstd = 1.0f / sqrtf(var + eps);
  for (int c = threadIdx.x * 4; c < H; c += LN_THREADS * 4) {
    const float4 v = *reinterpret_cast<const float4*>(row + c);
    const float4 g = *reinterpret_cast<const float4*>(gamma + c);
    const float4 b = *reinterpret_cast<const float4*>(beta + c);
    float4 o;
    o.x = (v.x - mean) * rstd * g.x + b.x;
    o.y = (v.y - mean) * rstd * g.y + b.y;
    o.z = (v.z - mean) * rstd * g.z + b.z;
    o.w = (v.w - mean) * rstd * g.w + b.w;
    *reinterpret_cast<float4*>(out + c) = o;
  }
}

__global__ __launch_bounds__(LN_THREADS) void bert_embed_ln_kernel(
    const float* __restrict__ word_emb, const float* __restrict__ pos_emb, const float* __restrict__ type_emb,
    const int* __restrict__ ids, const int* __restrict__ pos, int H, int vocab, int npos,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float* __restrict__ out) {
  extern __shared__ __align__(16) float smem[];
  float* row = smem;
  float* red = smem + H;
  const long long r = blockIdx.x;
  // ids / positions are device data: clamp, so a bad index reads a valid row instead of faulting
  const int id = min(max(ids[r], 0), vocab - 1);
  const int ps = min(max(pos[r], 0), npos - 1);
  const float* w = word_emb + (long long)id * H;
  const float* p = pos_emb + (long long)ps * H;
  float part = 0.f;
  for (int c = threadIdx.x * 4; c < H; c += LN_THREADS * 4) {
    const float4 a = *reinterpret_cast<const float4*>(w + c);
    const float4 b = *reinterpret_cast<const float4*>(p + c);
    const float4 t = *reinterpret_cast<const float4*>(type_emb + c);
    const float4 v = (a + b) + t;
    *reinterpret_cast<float4*>(row + c) = v;
    part += (v.x + v.y) + (v.z + v.w);
  }
  ln_row_store(row, H, part, gamma, beta, eps, out + r * H, red);
}

__global__ __launch_bounds__(LN_THREADS) void add_ln_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                            const float* __restrict__ res, int H,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps,
                                                            float* __restrict__ out) {
  extern __shared__ __align__(16) float smem[];
  float* row = smem;
  float* red = smem + H;
  const long long r = blockIdx.x;
  float part = 0.f;
  for (int c = threadIdx.x * 4; c < H; c += LN_THREADS * 4) {
    float4 v = *reinterpret_cast<const float4*>(x + r * H + c);
    if (bias != nullptr) v = v + *reinterpret_cast<const float4*>(bias + c);
    v = v + *reinterpret_cast<const float4*>(res + r * H + c);
    *reinterpret_cast<float4*>(row + c) = v;
    part += (v.x + v.y) + (v.z + v.w);
  }
  ln_row_store(row, H, part, gamma, beta, eps, out + r * H, red);
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__global__ __launch_bounds__(256) void bias_gelu_kernel(float* __restrict__ x, const float* __restrict__ bias,
                                                        long long rows, int cols4, long long ld) {
  const long long n = rows * cols4;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long r = i / cols4;
    const int c = (int)(i - r * cols4) * 4;
    float4 v = *reinterpret_cast<float4*>(x + r * ld + c);
    if (bias != nullptr) v = v + *reinterpret_cast<const float4*>(bias + c);
    v.x = gelu_erf(v.x);
    v.y = gelu_erf(v.y);
    v.z = gelu_erf(v.z);
    v.w = gelu_erf(v.w);
    *reinterpret_cast<float4*>(x + r * ld + c) = v;
  }
}

// One workgroup (one wave) per (query block of 64, head, sequence); lane = query. The query row and the output
// accumulator live in registers; keys and values are staged 64 at a time in LDS and every lane reads the same
// key / value address (a broadcast: no bank conflicts). Online softmax in chunks of 8 keys.
__global__ __launch_bounds__(ATT_BLOCK) void bert_attention_kernel(const float* __restrict__ qkv,
                                                                   const int* __restrict__ seq_off, int hidden,
                                                                   int total_rows, float scale,
                                                                   float* __restrict__ out, long long ld_out) {
  __shared__ __align__(16) float Ks[ATT_BLOCK * ATT_D];
  __shared__ __align__(16) float Vs[ATT_BLOCK * ATT_D];
  const int seq = blockIdx.z, head = blockIdx.y, qb = blockIdx.x;
  int base = seq_off[seq], end = seq_off[seq + 1];
  // offsets are device data: keep every row this block touches inside the buffer
  base = min(max(base, 0), total_rows);
  end = min(max(end, base), total_rows);
  const int n = min(end - base, ATT_MAX_SEQ);
  if (qb * ATT_BLOCK >= n) return;  // (uniform over the workgroup)
  const int lane = threadIdx.x;
  const int qi = qb * ATT_BLOCK + lane;
  const bool active = qi < n;
  const long long ld = 3LL * hidden;
  const float* kbase = qkv + hidden + head * ATT_D;
  const float* vbase = qkv + 2 * hidden + head * ATT_D;

  float q[ATT_D], acc[ATT_D];
  {
    const float* qp = qkv + (long long)(base + (active ? qi : 0)) * ld + head * ATT_D;
#pragma unroll
    for (int c = 0; c < ATT_D; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(qp + c);
      q[c] = v.x * scale, q[c + 1] = v.y * scale, q[c + 2] = v.z * scale, q[c + 3] = v.w * scale;
    }
  }
#pragma unroll
  for (int c = 0; c < ATT_D; ++c) acc[c] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int kb = 0; kb < n; kb += ATT_BLOCK) {
    const int nk = min(ATT_BLOCK, n - kb);
    __syncthreads();  // the previous block's reads are done
    for (int i = lane; i < ATT_BLOCK * (ATT_D / 4); i += ATT_BLOCK) {
      const int row = i >> 4, c4 = (i & 15) * 4;
      float4 kv = f4(0.f), vv = f4(0.f);
      if (row < nk) {
        const long long g = (long long)(base + kb + row) * ld + c4;
        kv = *reinterpret_cast<const float4*>(kbase + g);
        vv = *reinterpret_cast<const float4*>(vbase + g);
      }
      *reinterpret_cast<float4*>(Ks + row * ATT_D + c4) = kv;
      *reinterpret_cast<float4*>(Vs + row * ATT_D + c4) = vv;
    }
    __syncthreads();
    for (int j0 = 0; j0 < nk; j0 += 8) {
      float s[8];
      float cmax = -INFINITY;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float* kr = Ks + (j0 + u) * ATT_D;  // rows past nk are zero-filled, inside the block
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int c = 0; c < ATT_D; c += 8) {
          const float4 a = *reinterpret_cast<const float4*>(kr + c);
          const float4 b = *reinterpret_cast<const float4*>(kr + c + 4);
          d0 = fmaf(q[c], a.x, d0), d0 = fmaf(q[c + 1], a.y, d0), d0 = fmaf(q[c + 2], a.z, d0),
          d0 = fmaf(q[c + 3], a.w, d0);
          d1 = fmaf(q[c + 4], b.x, d1), d1 = fmaf(q[c + 5], b.y, d1), d1 = fmaf(q[c + 6], b.z, d1),
          d1 = fmaf(q[c + 7], b.w, d1);
        }
        s[u] = (j0 + u < nk) ? d0 + d1 : -INFINITY;
        cmax = fmaxf(cmax, s[u]);
      }
      const float mn = fmaxf(m, cmax);  // finite: key j0 < nk is valid
      const float corr = expf(m - mn);  // m = -inf on the first chunk: 0
      m = mn;
      l *= corr;
#pragma unroll
      for (int c = 0; c < ATT_D; ++c) acc[c] *= corr;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float p = expf(s[u] - mn);  // masked keys: exp(-inf) = 0
        l += p;
        const float* vr = Vs + (j0 + u) * ATT_D;
#pragma unroll
        for (int c = 0; c < ATT_D; c += 4) {
          const float4 v = *reinterpret_cast<const float4*>(vr + c);
          acc[c] = fmaf(p, v.x, acc[c]), acc[c + 1] = fmaf(p, v.y, acc[c + 1]);
          acc[c + 2] = fmaf(p, v.z, acc[c + 2]), acc[c + 3] = fmaf(p, v.w, acc[c + 3]);
        }
      }
    }
  }
  if (active) {
    const float inv = 1.0f / l;
    float* op = out + (long long)(base + qi) * ld_out + head * ATT_D;
#pragma unroll
    for (int c = 0; c < ATT_D; c += 4)
      *reinterpret_cast<float4*>(op + c) = make_float4(acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv);
  }
}

__global__ __launch_bounds__(256) void segment_sum_rows_kernel(const float* __restrict__ x,
                                                               const int* __restrict__ seg, int H, int total_rows,
                                                               float* __restrict__ out) {
  const long long s = blockIdx.x;
  int lo = seg[s], hi = seg[s + 1];
  lo = min(max(lo, 0), total_rows);
  hi = min(max(hi, lo), total_rows);
  for (int c = threadIdx.x * 4; c < H; c += 256 * 4) {
    float4 a = f4(0.f);
    for (int r = lo; r < hi; ++r) a = a + *reinterpret_cast<const float4*>(x + (long long)r * H + c);
    *reinterpret_cast<float4*>(out + s * H + c) = a;
  }
}

}  // namespace

extern "C" {

int capmi_bert_embed_ln(const float* word_emb, const float* pos_emb, const float* type_emb, const int* ids,
                        const int* pos, int rows, int hidden, int vocab, int npos, const float* gamma,
                        const float* beta, float eps, float* out, void* stream) {
  CAPMI_REQUIRE(word_emb && pos_emb && type_emb && ids && pos && gamma && beta && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(rows > 0 && vocab > 0 && npos > 0 && eps >= 0.f && hidden > 0 && hidden % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(hidden <= BERT_MAX_HIDDEN, CAPMI_ERANGE);
  CAPMI_REQUIRE(aligned16(word_emb) && aligned16(pos_emb) && aligned16(type_emb) && aligned16(gamma) &&
                    aligned16(beta) && aligned16(out), CAPMI_EALIGN);
  const size_t sh = (size_t)(hidden + 16) * sizeof(float);
  hipLaunchKernelGGL(bert_embed_ln_kernel, dim3(rows), dim3(LN_THREADS), sh, as_stream(stream), word_emb, pos_emb,
                type_emb, ids, pos, hidden, vocab, npos, gamma, beta, eps, out);
  CAPMI_LAUNCH_CHECK();
  return CAPMI_OK;
}

int capmi_add_ln(const float* x, const float* bias, const float* residual, int rows, int hidden,
                 const float* gamma, const float* beta, float eps, float* out, void* stream) {
  CAPMI_REQUIRE(x && residual && gamma && beta && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(rows > 0 && eps >= 0.f && hidden > 0 && hidden % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(hidden <= BERT_MAX_HIDDEN, CAPMI_ERANGE);
  CAPMI_REQUIRE(aligned16(x) && aligned16(residual) && aligned16(gamma) && aligned16(beta) && aligned16(out) &&
                    (bias == nullptr || aligned16(bias)), CAPMI_EALIGN);
  const size_t sh = (size_t)(hidden + 16) * sizeof(float);
  hipLaunchKernelGGL(add_ln_kernel, dim3(rows), dim3(LN_THREADS), sh, as_stream(stream), x, bias, residual, hidden,
                gamma, beta, eps, out);
  CAPMI_LAUNCH_CHECK();
  return CAPMI_OK;
}

int capmi_bias_gelu(float* x, const float* bias, long long rows, int cols, long long ld, void* stream) {
  CAPMI_REQUIRE(x, CAPMI_EINVAL);
  CAPMI_REQUIRE(rows > 0 && cols > 0 && cols % 4 == 0 && ld >= cols && ld % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(aligned16(x) && (bias == nullptr || aligned16(bias)), CAPMI_EALIGN);
  const long long n = rows * (cols / 4);
  const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 256LL * 16);
  hipLaunchKernelGGL(bias_gelu_kernel, dim3(grid), dim3(256), 0, as_stream(stream), x, bias, rows, cols / 4, ld);
  CAPMI_LAUNCH_CHECK();
  return CAPMI_OK;
}

int capmi_bert_attention(const float* qkv, const int* seq_off, int nseq, int total_rows, int max_len, int heads,
                         int head_dim, float* out, long long ld_out, void* stream) {
  CAPMI_REQUIRE(qkv && seq_off && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(nseq > 0 && total_rows > 0 && heads > 0 && head_dim > 0 && max_len > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(head_dim == ATT_D && max_len <= ATT_MAX_SEQ && nseq <= 65535 && heads <= 65535, CAPMI_ERANGE);
  const int hidden = heads * head_dim;
  CAPMI_REQUIRE(ld_out >= hidden && ld_out % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(aligned16(qkv) && aligned16(out), CAPMI_EALIGN);
  const dim3 grid(cdiv(max_len, ATT_BLOCK), heads, nseq);
  hipLaunchKernelGGL(bert_attention_kernel, grid, dim3(ATT_BLOCK), 0, as_stream(stream), qkv, seq_off, hidden,
                total_rows, 1.0f / sqrtf((float)head_dim), out, ld_out);
  CAPMI_LAUNCH_CHECK();
  return CAPMI_OK;
}

int capmi_segment_sum_rows(const float* x, const int* seg, int nseg, int total_rows, int hidden, float* out,
                           void* stream) {
  CAPMI_REQUIRE(x && seg && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(nseg > 0 && total_rows > 0 && hidden > 0 && hidden % 4 == 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(aligned16(x) && aligned16(out), CAPMI_EALIGN);
  hipLaunchKernelGGL(segment_sum_rows_kernel, dim3(nseg), dim3(256), 0, as_stream(stream), x, seg, hidden, total_rows,
                out);
  CAPMI_LAUNCH_CHECK();
  return CAPMI_OK;
}

}  // extern "C"
