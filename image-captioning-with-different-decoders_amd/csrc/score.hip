// Caption metrics on the sampler's token table: the BLEU-1..4 and ROUGE-L statistics of every hypothesis row against
// its image's references, and the weighted mix of CIDEr-D, BLEU-4 and ROUGE-L a self-critical step trains on.
// Nothing here copies to the host.
//
//   capmi_caption_stats   one workgroup of four waves per hypothesis row, tokens / lens / img_key / score_end read as
//                         capmi_cider_reward reads them (scst.hip) and the same uint64 n-gram keys.
//                         BLEU: wave w owns the (w + 1)-grams, lane l the one starting at word l; tf from the
//                         all-pairs compare in LDS; the lowest lane of every distinct key does one binary search in
//                         the image's (key, max count over its references) table and keeps min(tf, max count); one
//                         integer wave sum per order.
//                         ROUGE-L: the bit-vector LCS (Allison & Dix 1986; Hyyro 2004). Lane j holds hypothesis word j,
//                         the match mask of a reference word is the wave's ballot, V = (V + (V & M)) | (V & ~M) from
//                         all ones, LCS = the zero bits among the low len bits of V. The four waves take the image's
//                         distinct references round-robin and meet once in LDS; the same loop finds the reference
//                         length closest to the hypothesis's for the brevity penalty.
//                         Thread 0 finishes the row's sentence-level BLEU-1..4 and ROUGE-L in fp64 and rounds once.
//   capmi_reward_mix      reward = w_c cider + w_b bleu4 + w_r rouge in fp64, rounded once. One launch.
//
// Integer sums only, no atomics: a row's outputs depend on that row and the tables alone.
#include "common.h"

namespace {

constexpr int SCORE_TMAX = 64;  // words of a hypothesis or a reference: one lane, one bit of V each
constexpr int NS = CAPMI_SCORE_STATS;
constexpr double BLEU_TINY = 1e-15, BLEU_SMALL = 1e-9;  // capmi/scoring.py
constexpr double ROUGE_BETA2 = 1.2 * 1.2;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// (lcs, len) is the better recall: the larger lcs / len, the shorter reference on equal ratios
__device__ __forceinline__ bool better_recall(int lcs, int len, int best_lcs, int best_len) {
  const int a = lcs * best_len, b = best_lcs * len;  // <= 64 * 64
  return a > b || (a == b && len < best_len);
}

// (d, len) is the closer reference length: the smaller |len - hyp|, the shorter on a tie
__device__ __forceinline__ bool closer_len(int d, int len, int best_d, int best_len) {
  return d < best_d || (d == best_d && len < best_len);
}

__global__ void __launch_bounds__(256) caption_stats_kernel(
    const int* __restrict__ tokens, int T, int R, int n, const int* __restrict__ lens,
    const int* __restrict__ img_key, int n_images, int end_idx, int score_end,
    const unsigned long long* __restrict__ bleu_keys, const int* __restrict__ bleu_cnt,
    const int* __restrict__ bleu_off, const int* __restrict__ ref_tok, const int* __restrict__ ref_off,
    const int* __restrict__ ref_len, const int* __restrict__ rimg_off, int* __restrict__ stats,
    float* __restrict__ bleu, float* __restrict__ rouge) {
  __shared__ int tok[SCORE_TMAX];
  __shared__ unsigned long long keys[4][SCORE_TMAX];
  __shared__ int match[4];
  __shared__ int part[4][5];  // per wave: lcs_p, lcs_r, len_r, |closest - len|, closest
  const int r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the reference loop runs on scalars
  int len = lens[r];
  len = len < 0 ? 0 : (len > T ? T : len);
  if (tid < SCORE_TMAX) tok[tid] = tid < len ? tokens[(long long)tid * R + r] : -1;
  __syncthreads();
  if (!score_end && len > 0 && tok[len - 1] == end_idx) --len;
  const int image = img_key[r / n];
  if (image < 0 || image >= n_images) {  // the whole workgroup: no table row to score against
    if (tid < NS) stats[(long long)r * NS + tid] = -1;
    if (tid < 4) bleu[(long long)r * 4 + tid] = NAN;
    if (tid == 0) rouge[r] = NAN;
    return;
  }
  // BLEU: the wave's n-grams, one per lane
  const int order = w + 1, cnt = len - order + 1;
  const bool valid = lane < cnt;
  unsigned long long key = 0;
  if (valid) {
    for (int j = 0; j < order; ++j) key |= (unsigned long long)((tok[lane + j] + 1) & 0xffff) << (48 - 16 * j);
  }
  keys[w][lane] = key;
  __syncthreads();
  int tf = 0;
  bool first = true;
  if (valid) {
    for (int j = 0; j < cnt; ++j) {  // every lane reads the same address: a broadcast
      const bool eq = keys[w][j] == key;
      tf += eq;
      first = first && !(eq && j < lane);
    }
  }
  int clipped = 0;
  if (valid && first) {  // one lane per distinct n-gram
    const int e1 = bleu_off[image + 1];
    const int i = key_lower_bound(bleu_keys, bleu_off[image], e1, key);
    if (i < e1 && bleu_keys[i] == key) clipped = min(tf, bleu_cnt[i]);
  }
  clipped = wave_sum_int(clipped);
  if (lane == 0) match[w] = clipped;
  // ROUGE-L and the closest reference length: the image's distinct references, round-robin over the waves
  const int word = tok[lane];
  const bool live = lane < len;  // a dropped END stays in tok[len]
  const unsigned long long low = len >= 64 ? ~0ull : (1ull << len) - 1ull;
  int lcs_p = 0, lcs_r = -1, len_r = 1, d_best = 1 << 30, l_best = 0;
  const int r1 = rimg_off[image + 1];
  for (int ref = rimg_off[image] + w; ref < r1; ref += 4) {
    int rl = __builtin_amdgcn_readfirstlane(ref_len[ref]);
    rl = rl < 0 ? 0 : (rl > SCORE_TMAX ? SCORE_TMAX : rl);
    const int x = lane < rl ? ref_tok[ref_off[ref] + lane] : -1;  // reference word l in lane l
    unsigned long long V = ~0ull;
    for (int i = 0; i < rl; ++i) {
      const unsigned long long M = __ballot(live && word == __builtin_amdgcn_readlane(x, i));
      V = (V + (V & M)) | (V & ~M);  // the carry out of bit 63 drops
    }
    int lcs = __popcll(~V & low);
    // an empty sentence counts as one empty token, which matches only another empty sentence (capmi/scoring.py)
    if (len == 0 && rl == 0) lcs = 1;
    const int rlen = rl > 0 ? rl : 1;
    lcs_p = max(lcs_p, lcs);
    if (better_recall(lcs, rlen, lcs_r, len_r)) {
      lcs_r = lcs;
      len_r = rlen;
    }
    const int d = abs(rl - len);
    if (closer_len(d, rl, d_best, l_best)) {
      d_best = d;
      l_best = rl;
    }
  }
  if (lane == 0) {
    part[w][0] = lcs_p;
    part[w][1] = lcs_r;
    part[w][2] = len_r;
    part[w][3] = d_best;
    part[w][4] = l_best;
  }
  __syncthreads();
  if (tid == 0) {
#pragma clang fp contract(off)
    for (int k = 1; k < 4; ++k) {  // a wave without a reference keeps its start values, which lose
      lcs_p = max(lcs_p, part[k][0]);
      if (better_recall(part[k][1], part[k][2], lcs_r, len_r)) {
        lcs_r = part[k][1];
        len_r = part[k][2];
      }
      if (closer_len(part[k][3], part[k][4], d_best, l_best)) {
        d_best = part[k][3];
        l_best = part[k][4];
      }
    }
    if (lcs_r < 0) lcs_r = 0;  // an image without a reference: the tables never hold one
    const int len_h = len > 0 ? len : 1;
    int* __restrict__ s = stats + (long long)r * NS;
    // sentence-level BLEU-1..4 (capmi.scoring.bleu on this one hypothesis)
    const double ratio = ((double)len + BLEU_TINY) / ((double)l_best + BLEU_SMALL);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double prod = 1.0;
    for (int k = 0; k < 4; ++k) {
      const int guess = len > k ? len - k : 0;
      s[k] = match[k];
      s[4 + k] = guess;
      prod *= ((double)match[k] + BLEU_TINY) / ((double)guess + BLEU_SMALL);
      const double root = k == 0 ? prod : (k == 1 ? sqrt(prod) : (k == 2 ? cbrt(prod) : sqrt(sqrt(prod))));
      bleu[(long long)r * 4 + k] = (float)(ratio < 1.0 ? root * bp : root);
    }
    s[8] = len;
    s[9] = l_best;
    s[10] = lcs_p;
    s[11] = lcs_r;
    s[12] = len_r;
    s[13] = len_h;
    // ROUGE-L (capmi.scoring.rouge_l on this one hypothesis)
    const double prec = (double)lcs_p / (double)len_h, rec = (double)lcs_r / (double)len_r;
    double f = 0.0;
    if (prec != 0.0 && rec != 0.0) f = ((1.0 + ROUGE_BETA2) * prec * rec) / (rec + ROUGE_BETA2 * prec);
    rouge[r] = (float)f;
  }
}

__global__ void __launch_bounds__(256) reward_mix_kernel(const float* __restrict__ cider,
                                                         const float* __restrict__ bleu4, long long bleu_stride,
                                                         const float* __restrict__ rouge, int R, double w_c,
                                                         double w_b, double w_r, float* __restrict__ reward) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < R) reward[i] = (float)((w_c * (double)cider[i] + w_b * (double)bleu4[i * bleu_stride]) + w_r * (double)rouge[i]);
}

}  // namespace

extern "C" int capmi_caption_stats(const int* tokens, int T, int R, int n, const int* lens, const int* img_key,
                                   int n_images, int V, int end_idx, int score_end,
                                   const unsigned long long* bleu_keys, const int* bleu_cnt, int n_keys,
                                   const int* bleu_off, const int* ref_tok, int n_tok, const int* ref_off,
                                   const int* ref_len, const int* rimg_off, int* stats, float* bleu, float* rouge,
                                   void* stream) {
  CAPMI_REQUIRE(tokens && lens && img_key && bleu_off && ref_off && ref_len && rimg_off && stats && bleu && rouge,
                CAPMI_EINVAL);
  // references that are all empty have neither an n-gram nor a word: those tables may then be missing
  CAPMI_REQUIRE(n_keys >= 0 && (n_keys == 0 || (bleu_keys && bleu_cnt)), CAPMI_EINVAL);
  CAPMI_REQUIRE(n_tok >= 0 && (n_tok == 0 || ref_tok), CAPMI_EINVAL);
  CAPMI_REQUIRE(T > 0 && T <= SCORE_TMAX && R > 0 && n > 0 && R % n == 0 && n_images > 0 && V > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(end_idx >= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(V <= 65534, CAPMI_ERANGE);  // token + 1 in 16 bits, 0 kept for 'no word'
  CAPMI_REQUIRE((long long)R * NS < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(caption_stats_kernel, dim3(R), dim3(256), 0, as_stream(stream), tokens, T, R, n, lens, img_key,
                     n_images, end_idx, score_end, bleu_keys, bleu_cnt, bleu_off, ref_tok, ref_off, ref_len, rimg_off,
                     stats, bleu, rouge);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_reward_mix(const float* cider, const float* bleu4, long long bleu_stride, const float* rouge,
                                int R, double w_cider, double w_bleu4, double w_rouge, float* reward, void* stream) {
  CAPMI_REQUIRE(cider && bleu4 && rouge && reward && R > 0 && bleu_stride >= 1, CAPMI_EINVAL);
  CAPMI_REQUIRE(w_cider == w_cider && w_bleu4 == w_bleu4 && w_rouge == w_rouge, CAPMI_EINVAL);
  CAPMI_REQUIRE(bleu_stride * (long long)R < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(reward_mix_kernel, dim3(cdiv(R, 256)), dim3(256), 0, as_stream(stream), cider, bleu4, bleu_stride,
                     rouge, R, w_cider, w_bleu4, w_rouge, reward);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
