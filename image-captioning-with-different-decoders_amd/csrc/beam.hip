// Batched beam search (gen_captions.py:16-131 for B images at once): attention over beam groups that
// share one image's features, per-image top-s selection, and the per-step beam bookkeeping.
//
// Row layout of all three entry points: image i owns rows i*k .. i*k+k-1; its live[i] (0..k) surviving
// beams are compacted into the first live[i] of them, in selection order (the order the reference's
// seqs[inc] keeps). Rows at or past live[i] are dead: never read as candidates, never written.
//
//   capmi_beam_att_fwd : the arithmetic of att_score_fwd + att_softmax_ctx_fwd per live row, but one
//                        workgroup serves all rows of an image, so every att_enc / enc element it needs is
//                        loaded once and used for up to k rows (no k-fold expanded copy of either tensor)
//   capmi_beam_select  : log_softmax + carried beam score, top-s of each live row (s rounds of block
//                        arg-max), then the per-image merge of those <= k*s candidates by rank counting
//   capmi_beam_advance : one launch: finished beams recorded, survivors compacted, h/c gathered from
//                        their parents, next words / scores / back-pointers / live counts written
//   capmi_beam_backtrack : after the loop, one launch: per image the best finished beam walked back through
//                        the back-pointers into the sampler's (T, B) token table, so the scorer reads it in place
#include <limits.h>

#include "common.h"

constexpr int BEAM_KMAX = 16;

// --------------------------------------------------------------------------------------
// score: e[row][p] = relu(att_enc[i][p][:] + ad[row][:]) . wf + bf for the live rows of image i
// grid (cdiv(P, BEAM_PCH), B); a wave owns slots p0+wid, p0+wid+4, ...: each att_enc row is loaded once
// per wave and dotted against the ad of every live row (KM accumulators per lane). The per-row sum is one
// wave's in the lane order of att_score_fwd_kernel.
// --------------------------------------------------------------------------------------
constexpr int BEAM_PCH = 13;

template <int KM>
__global__ void __launch_bounds__(256) beam_score_kernel(
    const float* __restrict__ att_enc, const float* __restrict__ dec_part, int S, long long dec_slab,
    const float* __restrict__ bias_da, const float* __restrict__ wf, const float* __restrict__ bf,
    const int* __restrict__ live, int k, int P, int A, float* __restrict__ e) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // ad [s][A]
  const int i = blockIdx.y, p0 = blockIdx.x * BEAM_PCH;
  const int s = min(live[i], k);
  if (s <= 0) return;
  const long long row0 = (long long)i * k;
  for (int t = threadIdx.x; t < s * A; t += 256) {
    const int j = t / A, a = t - j * A;
    smem[t] = slab_sum(dec_part + (row0 + j) * A + a, S, dec_slab, bias_da ? bias_da[a] : 0.f);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const float b0 = bf ? bf[0] : 0.f;
  const int pend = min(P, p0 + BEAM_PCH);
  // the wave's R slots together: their loads are issued before any reduction, and the R*s wave sums run
  // interleaved (as att_score_fwd_kernel); each (slot, row) sum keeps its own order over a
  constexpr int R = (BEAM_PCH + 3) / 4;
  const float* base = att_enc + ((long long)i * P + p0 + wid) * A;
  float acc[R][KM];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int j = 0; j < KM; ++j) acc[r][j] = 0.f;
  for (int a = lane * 4; a < A; a += 256) {
    const float4 w = *reinterpret_cast<const float4*>(wf + a);
    float4 x[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      x[r] = p0 + wid + 4 * r < pend ? *reinterpret_cast<const float4*>(base + (long long)4 * r * A + a) : f4(0.f);
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < s) {
        const float4 d = *reinterpret_cast<const float4*>(smem + j * A + a);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r][j] += dot4(relu4(x[r] + d), w);
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = p0 + wid + 4 * r;
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < s && p < pend) {
        const float v = wave_sum(acc[r][j]);
        if (lane == 0) e[(row0 + j) * P + p] = v + b0;
      }
  }
}

// --------------------------------------------------------------------------------------
// softmax over P + context + gate for the live rows of image i: grid (cdiv(E, 256), B), 256 threads =
// 64 float4 columns x 4 slot groups. Softmax: one wave per row (rows wid, wid+4, ...), so a row's alpha
// does not depend on its position. Context: each enc float4 is loaded once and accumulated into every
// live row. The four slot groups are summed in the order of att_softmax_ctx_fwd_kernel.
// --------------------------------------------------------------------------------------
constexpr int BEAM_ECH = 256;

template <int KM>
__global__ void __launch_bounds__(256) beam_ctx_kernel(
    const float* __restrict__ e, const float* __restrict__ enc, const int* __restrict__ live, int k, int P,
    int E, float* __restrict__ alpha_out, float* __restrict__ awe_out, const float* __restrict__ gate_part,
    int S, long long gate_slab, const float* __restrict__ bias_fb, float* __restrict__ gate_out,
    float* __restrict__ x_out, long long ld_x) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int P4 = (P + 3) & ~3;
  float* alpha = smem;                                        // [KM][P4]
  float4* part = reinterpret_cast<float4*>(smem + KM * P4);   // [3][KM][64]
  const int i = blockIdx.y, tid = threadIdx.x;
  const int s = min(live[i], k);
  if (s <= 0) return;
  const long long row0 = (long long)i * k;
  const int lane = tid & 63, wid = tid >> 6;
  // the first U enc rows of this thread's slot group are requested before the softmax: they do not depend on it
  constexpr int U = KM <= 8 ? 8 : 4;
  const int c4 = tid & 63, pg = tid >> 6;
  const int c = blockIdx.x * BEAM_ECH + c4 * 4;
  const float* base = enc + (long long)i * P * E + c;
  float4 xb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int p = pg + 4 * u;
    xb[u] = (c < E && p < P) ? *reinterpret_cast<const float4*>(base + (long long)p * E) : f4(0.f);
  }
  for (int j = wid; j < s; j += 4) {
    const float* er = e + (row0 + j) * P;
    float* al = alpha + j * P4;
    float m = -INFINITY;
    for (int p = lane; p < P; p += 64) {
      const float v = er[p];
      al[p] = v;
      m = fmaxf(m, v);
    }
    m = wave_max(m);
    float sum = 0.f;
    for (int p = lane; p < P; p += 64) {
      const float v = expf(al[p] - m);
      al[p] = v;
      sum += v;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int p = lane; p < P; p += 64) {
      const float a = al[p] * inv;
      al[p] = a;
      if (alpha_out && blockIdx.x == 0) alpha_out[(row0 + j) * P + p] = a;
    }
  }
  __syncthreads();
  float4 acc[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) acc[j] = f4(0.f);
  // slots pg, pg+4, ... in blocks of U: the next block's loads are in flight while this one is accumulated
  for (int pb = pg; pb < P; pb += 4 * U) {
    float4 xn[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = pb + 4 * (U + u);
      xn[u] = (c < E && p < P) ? *reinterpret_cast<const float4*>(base + (long long)p * E) : f4(0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = pb + 4 * u;
      if (p < P) {
#pragma unroll
        for (int j = 0; j < KM; ++j)
          if (j < s) acc[j] = fma4(f4(alpha[j * P4 + p]), xb[u], acc[j]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) xb[u] = xn[u];
  }
  if (pg > 0) {
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < s) part[((pg - 1) * KM + j) * 64 + c4] = acc[j];
  }
  __syncthreads();
  if (pg == 0 && c < E) {
#pragma unroll
    for (int j = 0; j < KM; ++j)
      if (j < s) {
        float4 awe = acc[j];
        awe = awe + part[(0 * KM + j) * 64 + c4];
        awe = awe + part[(1 * KM + j) * 64 + c4];
        awe = awe + part[(2 * KM + j) * 64 + c4];
        const long long o = (row0 + j) * E + c;
        if (awe_out) *reinterpret_cast<float4*>(awe_out + o) = awe;
        float4 xg = awe;
        if (gate_part) {
          float4 g = slab_sum(reinterpret_cast<const float4*>(gate_part + o), S, gate_slab / 4,
                              *reinterpret_cast<const float4*>(bias_fb + c));
          g = make_float4(sigmoidf_(g.x), sigmoidf_(g.y), sigmoidf_(g.z), sigmoidf_(g.w));
          if (gate_out) *reinterpret_cast<float4*>(gate_out + o) = g;
          xg = g * awe;
        }
        if (x_out) *reinterpret_cast<float4*>(x_out + (row0 + j) * ld_x + c) = xg;
      }
  }
}

template <int KM>
static int beam_att_launch(const float* enc, const float* att_enc, const float* dec_part, int S_a,
                           long long slab_a, const float* bias_da, const float* wf, const float* bf,
                           const float* gate_part, int S_g, long long slab_g, const float* bias_fb,
                           const int* live, int B, int k, int P, int A, int E, float* e_ws, float* alpha_out,
                           float* awe_out, float* gate_out, float* x_out, long long ld_x, hipStream_t st) {
  const size_t sh_s = (size_t)k * A * sizeof(float);
  const size_t sh_c = ((size_t)KM * ((P + 3) & ~3) + 3 * KM * 64 * 4) * sizeof(float);
  CAPMI_REQUIRE(sh_s <= 65536 && sh_c <= 65536, CAPMI_ERANGE);
  hipLaunchKernelGGL(beam_score_kernel<KM>, dim3(cdiv(P, BEAM_PCH), B), dim3(256), sh_s, st, att_enc, dec_part,
                     S_a, slab_a, bias_da, wf, bf, live, k, P, A, e_ws);
  CAPMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_ctx_kernel<KM>, dim3(cdiv(E, BEAM_ECH), B), dim3(256), sh_c, st, e_ws, enc, live, k, P,
                     E, alpha_out, awe_out, gate_part, S_g, slab_g, bias_fb, gate_out, x_out, ld_x);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_beam_att_fwd(const float* enc, const float* att_enc, const float* dec_part, int S_a,
                                  long long slab_a, const float* bias_da, const float* wf, const float* bf,
                                  const float* gate_part, int S_g, long long slab_g, const float* bias_fb,
                                  const int* live, int B, int k, int P, int A, int E, float* e_ws,
                                  float* alpha_out, float* awe_out, float* gate_out, float* x_out,
                                  long long ld_x, void* stream) {
  CAPMI_REQUIRE(enc && att_enc && dec_part && wf && live && e_ws, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && P > 0 && A > 0 && E > 0 && S_a >= 1 && k >= 1 && k <= BEAM_KMAX, CAPMI_EINVAL);
  CAPMI_REQUIRE(!gate_part || (bias_fb && S_g >= 1 && slab_g % 4 == 0), CAPMI_EINVAL);
  CAPMI_REQUIRE(A % 4 == 0 && E % 4 == 0 && B <= 65535, CAPMI_ERANGE);
  CAPMI_REQUIRE(aligned16(enc) && aligned16(att_enc) && aligned16(wf) && (!awe_out || aligned16(awe_out)) &&
                    (!gate_out || aligned16(gate_out)) && (!gate_part || (aligned16(gate_part) && aligned16(bias_fb))),
                CAPMI_EALIGN);
  CAPMI_REQUIRE(!x_out || (aligned16(x_out) && ld_x % 4 == 0 && ld_x >= E), CAPMI_EALIGN);
  const hipStream_t st = as_stream(stream);
#define BEAM_ATT(KM)                                                                                           \
  return beam_att_launch<KM>(enc, att_enc, dec_part, S_a, slab_a, bias_da, wf, bf, gate_part, S_g, slab_g,     \
                             bias_fb, live, B, k, P, A, E, e_ws, alpha_out, awe_out, gate_out, x_out, ld_x, st)
  if (k <= 4) BEAM_ATT(4);
  if (k <= 8) BEAM_ATT(8);
  BEAM_ATT(16);
#undef BEAM_ATT
}

// --------------------------------------------------------------------------------------
// selection. A candidate is (value, flat index j*V + w); candidate x precedes y when its value is larger,
// or equal with the lower flat index.
// beam_row_topk_kernel, one workgroup per live row: max and sum-exp of the row (fixed thread -> column
// assignment and reduction tree, so bit-identical rows give bit-identical values wherever they sit), then s
// rounds of block arg-max over value = score + ((x - max) - log(sum)); round r takes the best candidate
// that comes strictly after round r-1's pick, so nothing has to be marked. The row stays L2-resident.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ bool cand_before(float v, int w, float ov, int ow) {
  return v > ov || (v == ov && w < ow);
}

constexpr int BEAM_TOPK_T = 1024;  // threads per row: V = 8100 is 8 columns per thread and pass

__global__ void __launch_bounds__(BEAM_TOPK_T) beam_row_topk_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ scores,
                                                            const int* __restrict__ live, int first_step, int k,
                                                            int V, float* __restrict__ cand_v,
                                                            int* __restrict__ cand_w) {
  __shared__ float red[16];
  __shared__ float rv[BEAM_TOPK_T / 64];
  __shared__ int rw[BEAM_TOPK_T / 64];
  const int i = blockIdx.x / k, j = blockIdx.x - i * k;
  const int s = min(live[i], k);
  if (j >= (first_step ? min(s, 1) : s)) return;
  const long long row = blockIdx.x;
  const float* x = logits + row * V;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float m = -INFINITY;
  for (int w = tid; w < V; w += BEAM_TOPK_T) m = fmaxf(m, x[w]);
  m = block_max(m, red);
  float sum = 0.f;
  for (int w = tid; w < V; w += BEAM_TOPK_T) sum += expf(x[w] - m);
  sum = block_sum(sum, red);
  const float lg = logf(sum), sc = scores[row];
  float lastv = INFINITY;
  int lastw = -1;
  for (int r = 0; r < s; ++r) {
    float bv = -INFINITY;
    int bw = INT_MAX;
    for (int w = tid; w < V; w += BEAM_TOPK_T) {
      const float v = sc + ((x[w] - m) - lg);
      if (cand_before(lastv, lastw, v, w) && cand_before(v, w, bv, bw)) {
        bv = v;
        bw = w;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int ow = __shfl_xor(bw, o, 64);
      if (cand_before(ov, ow, bv, bw)) {
        bv = ov;
        bw = ow;
      }
    }
    __syncthreads();
    if (lane == 0) {
      rv[wid] = bv;
      rw[wid] = bw;
    }
    __syncthreads();
    bv = rv[0];
    bw = rw[0];
#pragma unroll
    for (int q = 1; q < BEAM_TOPK_T / 64; ++q)
      if (cand_before(rv[q], rw[q], bv, bw)) {
        bv = rv[q];
        bw = rw[q];
      }
    if (tid == 0) {
      cand_v[row * k + r] = bv;
      cand_w[row * k + r] = bw < V ? bw : 0;  // no candidate left (NaN logits): keep the word a valid index
    }
    lastv = bv;
    lastw = bw;
  }
}

// per image: the n = rows*s row candidates (n <= 256) are ranked by counting the candidates that precede
// each one; ranks 0..s-1 are the selection, in descending order
__global__ void __launch_bounds__(256) beam_merge_kernel(const float* __restrict__ cand_v,
                                                         const int* __restrict__ cand_w,
                                                         const int* __restrict__ live, int first_step, int k,
                                                         int V, int* __restrict__ parent, int* __restrict__ word,
                                                         float* __restrict__ top) {
  __shared__ float cv[BEAM_KMAX * BEAM_KMAX];
  __shared__ long long cf[BEAM_KMAX * BEAM_KMAX];
  const int i = blockIdx.x, t = threadIdx.x;
  const int s = min(live[i], k);
  if (s <= 0) return;
  const int rows = first_step ? 1 : s, n = rows * s;
  float v = 0.f;
  long long f = 0;
  int j = 0, w = 0;
  if (t < n) {
    j = t / s;
    const long long o = ((long long)i * k + j) * k + (t - j * s);
    v = cand_v[o];
    w = cand_w[o];
    f = (long long)j * V + w;
    cv[t] = v;
    cf[t] = f;
  }
  __syncthreads();
  if (t < n) {
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += (cv[q] > v || (cv[q] == v && cf[q] < f)) ? 1 : 0;
    if (rank < s) {
      const long long o = (long long)i * k + rank;
      parent[o] = j;
      word[o] = w;
      top[o] = v;
    }
  }
}

extern "C" int capmi_beam_select(const float* logits, const float* scores, const int* live, int first_step,
                                 int B, int k, int V, float* cand_v, int* cand_w, int* parent, int* word,
                                 float* top, void* stream) {
  CAPMI_REQUIRE(logits && scores && live && cand_v && cand_w && parent && word && top, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && k >= 1 && k <= BEAM_KMAX && V >= k && (long long)B * k <= INT_MAX, CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)k * V <= INT_MAX, CAPMI_ERANGE);
  const hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(beam_row_topk_kernel, dim3(B * k), dim3(BEAM_TOPK_T), 0, st, logits, scores, live, first_step, k, V,
                     cand_v, cand_w);
  CAPMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(256), 0, st, cand_v, cand_w, live, first_step, k, V, parent,
                     word, top);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

// --------------------------------------------------------------------------------------
// bookkeeping of one step, one workgroup per image. Selection slot r (< s = live[i]) either ends (word ==
// end_idx: appended to the image's finished list as (step, r, score)) or survives into row n = number of
// survivors before it. bp_parent / bp_word are indexed by slot, bp_src by the new row (the slot it came
// from), so a sequence is walked back as slot -> parent row -> (previous step) slot of that row.
// --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) beam_advance_kernel(
    const int* __restrict__ parent, const int* __restrict__ word, const float* __restrict__ top,
    int* __restrict__ live, int k, int D, int end_idx, int step, const float* __restrict__ h_src,
    const float* __restrict__ c_src, float* __restrict__ h_dst, float* __restrict__ c_dst,
    long long* __restrict__ prev, float* __restrict__ scores, int* __restrict__ bp_parent,
    int* __restrict__ bp_word, int* __restrict__ bp_src, int* __restrict__ fin_count,
    int* __restrict__ fin_step, int* __restrict__ fin_slot, float* __restrict__ fin_score,
    int* __restrict__ images_live) {
  __shared__ int src_row[BEAM_KMAX];
  __shared__ int n_sh;
  const int i = blockIdx.x;
  const int s = min(live[i], k);
  if (s <= 0) return;
  const long long row0 = (long long)i * k;
  if (threadIdx.x == 0) {
    int n = 0, nf = fin_count[i];
    for (int r = 0; r < s; ++r) {
      const int par = parent[row0 + r], w = word[row0 + r];
      const float v = top[row0 + r];
      bp_parent[row0 + r] = par;
      bp_word[row0 + r] = w;
      if (w == end_idx) {
        if (nf < k) {
          fin_step[row0 + nf] = step;
          fin_slot[row0 + nf] = r;
          fin_score[row0 + nf] = v;
          ++nf;
        }
      } else {
        src_row[n] = par;
        bp_src[row0 + n] = r;
        prev[row0 + n] = w;
        scores[row0 + n] = v;
        ++n;
      }
    }
    fin_count[i] = nf;
    live[i] = n;
    n_sh = n;
    if (n == 0) atomicSub(images_live, 1);
  }
  __syncthreads();
  const int n = n_sh;
  for (int t = threadIdx.x; t < n * D; t += 256) {
    const int r = t / D, d = t - r * D;
    const long long src = (row0 + src_row[r]) * D + d, dst = (row0 + r) * D + d;
    h_dst[dst] = h_src[src];
    c_dst[dst] = c_src[src];
  }
}

extern "C" int capmi_beam_advance(const int* parent, const int* word, const float* top, int* live, int B, int k,
                                  int D, int end_idx, int step, const float* h_src, const float* c_src,
                                  float* h_dst, float* c_dst, long long* prev, float* scores, int* bp_parent,
                                  int* bp_word, int* bp_src, int* fin_count, int* fin_step, int* fin_slot,
                                  float* fin_score, int* images_live, void* stream) {
  CAPMI_REQUIRE(parent && word && top && live && h_src && c_src && h_dst && c_dst && prev && scores, CAPMI_EINVAL);
  CAPMI_REQUIRE(bp_parent && bp_word && bp_src && fin_count && fin_step && fin_slot && fin_score && images_live,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(h_src != h_dst && c_src != c_dst, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && k >= 1 && k <= BEAM_KMAX && D > 0 && step >= 0, CAPMI_EINVAL);
  hipLaunchKernelGGL(beam_advance_kernel, dim3(B), dim3(256), 0, as_stream(stream), parent, word, top, live, k, D,
                     end_idx, step, h_src, c_src, h_dst, c_dst, prev, scores, bp_parent, bp_word, bp_src, fin_count,
                     fin_step, fin_slot, fin_score, images_live);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

// --------------------------------------------------------------------------------------
// back-trace after the loop, one thread per image: the finished beam with the largest key (or, with
// fallback_live, live row 0 at the last step) is walked back through the back-pointers twice, once to count
// the words it keeps and once to write them from position 0 of column i of the (T, B) token table. Every
// index read from the state (finished count, step, slot, parent row) is checked against its range during
// the first walk; a path that leaves it gives length 0, so the second walk reads only what the first saw.
// --------------------------------------------------------------------------------------
constexpr int BEAM_BT_T = 64;

__global__ void __launch_bounds__(BEAM_BT_T) beam_backtrack_kernel(
    const int* __restrict__ bp, const int* __restrict__ fin_count, const int* __restrict__ fin_step,
    const int* __restrict__ fin_slot, const float* __restrict__ fin_score, const int* __restrict__ live,
    const float* __restrict__ scores, int steps, int B, int k, int T, int end_idx, int drop_a, int drop_b,
    int emit_end, int fallback_live, double length_alpha, int* __restrict__ tokens, int* __restrict__ lens,
    int* __restrict__ finished, float* __restrict__ score, int* __restrict__ alpha_rows) {
  const int i = blockIdx.x * BEAM_BT_T + threadIdx.x;
  if (i >= B) return;
  const long long R = (long long)B * k, row0 = (long long)i * k;
  const int* bp_i = bp + row0;  // bp[t][c][i*k + s] = bp_i[(t*3 + c)*R + s]
  int t0 = -1, s0 = 0, fin = 0;
  float sc = 0.f;
  const int nf = min(fin_count[i], k);
  if (nf > 0) {
    int best = 0;
    if (length_alpha == 0.0) {
      float bv = fin_score[row0];
      for (int q = 1; q < nf; ++q) {
        const float v = fin_score[row0 + q];
        if (v > bv) {
          bv = v;
          best = q;
        }
      }
    } else {
      double bv = (double)fin_score[row0] / pow((double)fin_step[row0] + 1.0, length_alpha);
      for (int q = 1; q < nf; ++q) {
        const double v = (double)fin_score[row0 + q] / pow((double)fin_step[row0 + q] + 1.0, length_alpha);
        if (v > bv) {
          bv = v;
          best = q;
        }
      }
    }
    t0 = fin_step[row0 + best];
    s0 = fin_slot[row0 + best];
    sc = fin_score[row0 + best];
    fin = 1;
  } else if (fallback_live && live[i] > 0 && steps > 0) {
    t0 = steps - 1;
    s0 = bp_i[((long long)t0 * 3 + 2) * R];
    sc = scores[row0];
  }
  bool ok = t0 >= 0 && t0 < steps && s0 >= 0 && s0 < k;
  const int t_end = t0;  // the step whose END is the sequence's last word
  const auto kept = [&](int t, int w) {
    return w != drop_a && w != drop_b && !(t == t_end && w == end_idx && !emit_end);
  };
  int n = 0;
  if (ok) {
    int t = t0, s = s0;
    while (true) {
      const int row = bp_i[((long long)t * 3 + 0) * R + s], w = bp_i[((long long)t * 3 + 1) * R + s];
      if (row < 0 || row >= k) {
        ok = false;
        break;
      }
      n += kept(t, w) ? 1 : 0;
      if (t == 0) break;
      --t;
      s = bp_i[((long long)t * 3 + 2) * R + row];
      if (s < 0 || s >= k) {
        ok = false;
        break;
      }
    }
  }
  if (!ok) {
    n = 0;
    t0 = -1;
    fin = 0;
    sc = 0.f;
  }
  lens[i] = n;
  finished[i] = fin;
  score[i] = sc;
  for (int t = n; t < T; ++t) tokens[(long long)t * B + i] = -1;
  if (alpha_rows)
    for (int t = t0 + 1; t < T; ++t) alpha_rows[(long long)t * B + i] = -1;
  if (!ok) return;
  int t = t0, s = s0, pos = n;
  while (true) {
    const int row = bp_i[((long long)t * 3 + 0) * R + s], w = bp_i[((long long)t * 3 + 1) * R + s];
    if (kept(t, w)) tokens[(long long)(--pos) * B + i] = w;
    if (alpha_rows) alpha_rows[(long long)t * B + i] = (int)((long long)t * R + row0 + row);
    if (t == 0) break;
    --t;
    s = bp_i[((long long)t * 3 + 2) * R + row];
  }
}

extern "C" int capmi_beam_backtrack(const int* bp, const int* fin_count, const int* fin_step, const int* fin_slot,
                                    const float* fin_score, const int* live, const float* scores, int steps, int B,
                                    int k, int T, int end_idx, int drop_a, int drop_b, int emit_end,
                                    int fallback_live, double length_alpha, int* tokens, int* lens, int* finished,
                                    float* score, int* alpha_rows, void* stream) {
  CAPMI_REQUIRE(bp && fin_count && fin_step && fin_slot && fin_score && live && scores, CAPMI_EINVAL);
  CAPMI_REQUIRE(tokens && lens && finished && score, CAPMI_EINVAL);
  CAPMI_REQUIRE(B >= 1 && k >= 1 && k <= BEAM_KMAX && T >= 1 && steps >= 0 && steps <= T && end_idx >= 0,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(length_alpha >= 0.0, CAPMI_EINVAL);  // a NaN fails the comparison too
  // T * R * 3 < 2^31 (the first test keeps the product inside 64 bits)
  CAPMI_REQUIRE((long long)B * k * 3 < (1LL << 31) && (long long)T * B * k * 3 < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(beam_backtrack_kernel, dim3(cdiv(B, BEAM_BT_T)), dim3(BEAM_BT_T), 0, as_stream(stream), bp,
                     fin_count, fin_step, fin_slot, fin_score, live, scores, steps, B, k, T, end_idx, drop_a, drop_b,
                     emit_end, fallback_live, length_alpha, tokens, lens, finished, score, alpha_rows);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
