// Sampled decoding: one launch per decode step draws the next token of every row from its logits
// (temperature / top-k sampling or greedy) and records the token's log-probability.
//
//   capmi_sample_step : one workgroup per row. The row is read from HBM once into LDS (V <= SAMPLE_LDS_V;
//                       longer rows are re-read through L2 by the same code). Steps, all fp32:
//     1. block max with the lowest index attaining it (the greedy token, and the softmax shift)
//     2. top-k: exact radix select of the k-th largest value on the order-preserving bit pattern of the raw
//        logits, four 8-bit digits, integer histogram in LDS; ties at the threshold are ranked by
//        vocabulary index with an integer block scan, so the kept set is exact and deterministic
//     3. thread t owns the contiguous chunk [t*chunk, t*chunk + chunk): it sums its weights
//        w_v = exp((l_v - max) / temperature) in index order, a block scan gives every thread the sum of the
//        chunks before it (excl) and S, the first thread whose inclusive sum exceeds u*S walks its chunk and
//        takes the first v with excl + (w_first + ... + w_v) > u*S
//     4. logp = (l_tok - max) / temperature - log S; thread 0 or the owner writes the row's outputs
//   The thread count is a constant and every sum has one fixed order, so a row's result depends on its
//   logits and u alone, not on its position or on R. No float atomics; the integer LDS atomics only count.
#include <limits.h>

#include "common.h"

constexpr int SAMPLE_T = 1024;        // threads per row: V = 8100 is a chunk of 9 per thread
constexpr int SAMPLE_W = SAMPLE_T / 64;
constexpr int SAMPLE_LDS_V = 14336;   // rows up to 56 KB stay in LDS (64 KB with the scratch below)

// bit pattern whose unsigned order is the float order (-0 counted as +0)
__device__ __forceinline__ unsigned sample_key(float x) {
  const unsigned b = __float_as_uint(x + 0.f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// exclusive scan over the block's threads in thread order; incl = excl of the next thread (bit for bit),
// the last thread's incl is the total. wt = LDS[SAMPLE_W].
template <typename Tp>
__device__ __forceinline__ Tp sample_scan(Tp v, Tp* wt, Tp* incl_out, Tp* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  Tp inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Tp n = __shfl_up(inc, o, 64);
    if (lane >= o) inc += n;
  }
  const Tp before = __shfl_up(inc, 1, 64);
  __syncthreads();
  if (lane == 63) wt[wid] = inc;
  __syncthreads();
  Tp off = 0, all = 0;
  for (int i = 0; i < SAMPLE_W; ++i) {
    if (i == wid) off = all;
    all += wt[i];
  }
  *incl_out = off + inc;
  *total = all;
  return lane == 0 ? off : off + before;
}

template <bool IN_LDS>
__global__ void __launch_bounds__(SAMPLE_T) sample_step_kernel(
    const float* __restrict__ logits, long long ld, int V, const float* __restrict__ u, float temperature,
    int top_k, int end_idx, int* __restrict__ alive, long long* __restrict__ prev, int* __restrict__ tokens,
    float* __restrict__ logp, int* __restrict__ rows_live) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ float redv[SAMPLE_W];
  __shared__ int redi[SAMPLE_W];
  __shared__ int hist[4 * 256];
  __shared__ float wt_f[SAMPLE_W];
  __shared__ int wt_i[SAMPLE_W];
  __shared__ int sel_digit, sel_need, pick_t, last_pos;
  const long long row = blockIdx.x;
  if (alive[row] == 0) return;  // the whole workgroup: a dead row writes nothing
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* __restrict__ g = logits + row * ld;
  auto at = [&](int v) -> float {
    if constexpr (IN_LDS) return srow[v];
    else return g[v];
  };

  // 1. the row into LDS, max and the lowest index attaining it
  float bm = -INFINITY;
  int bi = INT_MAX;
  // eight loads in flight per thread (V = 8100: the whole row in one round), taken in index order
  for (int vb = tid; vb < V; vb += 8 * SAMPLE_T) {
    float a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = vb + j * SAMPLE_T;
      a[j] = v < V ? g[v] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = vb + j * SAMPLE_T;
      if (v < V) {
        if constexpr (IN_LDS) srow[v] = a[j];
        if (a[j] > bm) {
          bm = a[j];
          bi = v;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bm, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bm || (ov == bm && oi < bi)) {
      bm = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    redv[wid] = bm;
    redi[wid] = bi;
  }
  if (tid == 0) {
    pick_t = INT_MAX;
    last_pos = -1;
    sel_digit = 0;
    sel_need = 1;
  }
  __syncthreads();
  bm = redv[0];
  bi = redi[0];
#pragma unroll
  for (int q = 1; q < SAMPLE_W; ++q)
    if (redv[q] > bm || (redv[q] == bm && redi[q] < bi)) {
      bm = redv[q];
      bi = redi[q];
    }
  const float m = bm;
  const int am = bi < V ? bi : 0;  // no finite logit (all -inf / NaN): keep the token a valid index

  const bool greedy = temperature == 0.f;
  const float tdiv = greedy ? 1.f : temperature;
  const bool select = !greedy && top_k > 0 && top_k < V;

  // 2. thr = key of the top_k-th largest logit, need = how many entries equal to it are kept
  unsigned thr = 0;
  int need = INT_MAX;
  if (select) {
    unsigned prefix = 0, mask = 0;
    int rem = top_k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[tid] = 0;  // SAMPLE_T == 4 * 256
      __syncthreads();
      for (int v = tid; v < V; v += SAMPLE_T) {
        const unsigned key = sample_key(at(v));
        // four copies of the histogram by lane: a quarter of the same-address serialisation
        if ((key & mask) == prefix) atomicAdd(&hist[(lane & 3) * 256 + ((key >> shift) & 255u)], 1);
      }
      __syncthreads();
      if (wid == 0) {  // lane l owns digits 4l .. 4l+3; counted from the top digit down
        int h[4], s = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int d = 4 * lane + j;
          h[j] = hist[d] + hist[256 + d] + hist[512 + d] + hist[768 + d];
          s += h[j];
        }
        int suf = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int n = __shfl_down(suf, o, 64);
          if (lane + o < 64) suf += n;
        }
        int above = suf - s;
        if (above < rem && rem <= above + s) {  // exactly one lane: the prefix set holds >= rem entries
          int j = 3;
          while (j > 0 && above + h[j] < rem) {
            above += h[j];
            --j;
          }
          sel_digit = 4 * lane + j;
          sel_need = rem - above;
        }
      }
      __syncthreads();
      prefix |= (unsigned)sel_digit << shift;
      mask |= 255u << shift;
      rem = sel_need;
    }
    thr = prefix;
    need = rem;
  }

  // thread t owns [v0, v1); an odd chunk keeps the LDS reads of a wave on distinct banks
  const int chunk = ((V - 1) / SAMPLE_T + 1) | 1;
  const long long lo = (long long)tid * chunk;
  const int v0 = (int)(lo < V ? lo : V), v1 = (int)(lo + chunk < V ? lo + chunk : V);

  // entries equal to the threshold are kept in index order: eq0 = how many sit before this chunk
  int eq0 = 0;
  if (select) {
    int c = 0, inc_, tot_;
    for (int v = v0; v < v1; ++v) c += sample_key(at(v)) == thr ? 1 : 0;
    eq0 = sample_scan<int>(c, wt_i, &inc_, &tot_);
  }
  auto weight = [&](int v, int& eq) -> float {
    const float a = at(v);
    if (select) {
      const unsigned key = sample_key(a);
      if (key < thr) return 0.f;
      if (key == thr && eq++ >= need) return 0.f;
    }
    return expf((a - m) / tdiv);
  };

  // 3. chunk sums in index order, block scan
  float sum = 0.f;
  int lastp = -1, eq = eq0;
  for (int v = v0; v < v1; ++v) {
    const float w = weight(v, eq);
    sum += w;
    if (w > 0.f) lastp = v;
  }
  float incl, S;
  const float excl = sample_scan<float>(sum, wt_f, &incl, &S);
  const float target = greedy ? 0.f : u[row] * S;
  if (lastp >= 0) atomicMax(&last_pos, lastp);
  if (!greedy && incl > target) atomicMin(&pick_t, tid);
  __syncthreads();
  const int owner = pick_t == INT_MAX ? 0 : pick_t;
  if (tid != owner) return;

  // 4. the owner finds the token inside its chunk and writes the row's outputs
  int tok = -1;
  if (greedy) {
    tok = am;
  } else {
    if (pick_t != INT_MAX) {
      float local = 0.f;
      int lastc = -1;
      eq = eq0;
      for (int v = v0; v < v1; ++v) {
        const float w = weight(v, eq);
        local += w;
        if (w > 0.f) {
          lastc = v;
          if (excl + local > target) {
            tok = v;
            break;
          }
        }
      }
      if (tok < 0) tok = lastc;  // the scan's rounding against this loop's: the chunk's last weighted entry
    }
    if (tok < 0) tok = last_pos;  // u * S rounded up to S: the last kept entry with weight
    if (tok < 0) tok = am;        // no weight anywhere (NaN row)
  }
  tokens[row] = tok;
  logp[row] = (g[tok] - m) / tdiv - logf(S);
  prev[row] = tok;
  if (tok == end_idx) {
    alive[row] = 0;
    atomicSub(rows_live, 1);
  }
}

extern "C" int capmi_sample_step(const float* logits, int ld, int R, int V, const float* u, float temperature,
                                 int top_k, int end_idx, int step, int* alive, long long* prev, int* tokens,
                                 float* logp, int* rows_live, void* stream) {
  CAPMI_REQUIRE(logits && u && alive && prev && tokens && logp && rows_live, CAPMI_EINVAL);
  CAPMI_REQUIRE(R >= 1 && V >= 1 && ld >= V && step >= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(temperature >= 0.f && top_k >= 0, CAPMI_EINVAL);  // a NaN temperature fails the comparison
  CAPMI_REQUIRE(V <= (1 << 30), CAPMI_ERANGE);  // index arithmetic in int with room for a round of loads
  const hipStream_t st = as_stream(stream);
  if (V <= SAMPLE_LDS_V)
    CAPMI_KLAUNCH(sample_step_kernel<true>, dim3(R), dim3(SAMPLE_T), (size_t)V * sizeof(float), st, logits,
                  (long long)ld, V, u, temperature, top_k, end_idx, alive, prev, tokens, logp, rows_live);
  else
    CAPMI_KLAUNCH(sample_step_kernel<false>, dim3(R), dim3(SAMPLE_T), 0, st, logits, (long long)ld, V, u,
                  temperature, top_k, end_idx, alive, prev, tokens, logp, rows_live);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
