// Self-critical sequence training (SCST) on the sampler's token table: pack the rollouts into teacher-forcing
// captions, score every hypothesis with CIDEr-D against its image's references and turn the rewards into
// advantages. capmi_pg_ce_fwd_bwd (loss.hip) weights the cross-entropy rows by them. Nothing here copies to the host.
//
//   capmi_rollout_pack    tokens (T, R) int32 as capmi_sample_step leaves them (-1: the row had finished or the loop
//                         had stopped) -> lens[r], caps (R, T + 1) int64 = [start, tok_0 .. tok_{len-1}, pad ..],
//                         count = sum lens, inv_count = 1 / count. One workgroup, one launch.
//   capmi_cider_reward    one workgroup of four waves per hypothesis row; wave w owns the (w + 1)-grams, lane l the
//                         one starting at word l (T <= 64: at most 64 n-grams of each order). An n-gram is a uint64
//                         key of four 16-bit fields token + 1, first word in the top field, shorter ones zero-filled,
//                         so a key carries its own order. tf: an all-pairs compare of the wave's keys in LDS, the
//                         lowest lane of every distinct key keeps the count. idf: binary search in the corpus table
//                         (sorted keys, fp32 idf; an absent key has df 0 and idf = log_images). Per listed reference
//                         the lane's key is searched in the reference's own sorted (key, weight) entries. Every sum
//                         (two norms' worth per order, the clipped products) is one wave butterfly: a fixed order and
//                         no barrier inside the reference loop; the four orders meet once at the end.
//   capmi_scst_advantage  reward minus the mean of the image's other samples, or minus the greedy rollout's reward;
//                         the batch means go to a two-float stats buffer. One workgroup, one launch.
//
// All reductions are fp32 in one fixed order, no float atomics: a row's result depends on that row's inputs alone.
#include "common.h"

namespace {

constexpr int SCST_TMAX = 64;      // words of a hypothesis: one lane per starting word
constexpr float CIDER_2SIGMA2 = 72.f;  // 2 sigma^2, sigma = 6

__global__ void __launch_bounds__(1024) rollout_pack_kernel(const int* __restrict__ tokens, int T, int R,
                                                            long long start_idx, int end_idx, long long pad_idx,
                                                            int* __restrict__ lens, long long* __restrict__ caps,
                                                            int* __restrict__ count, float* __restrict__ inv_count) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int n = 0;
  for (int r = threadIdx.x; r < R; r += 1024) {
    long long* __restrict__ c = caps + (long long)r * (T + 1);
    c[0] = start_idx;
    int len = 0;
    bool open = true;
    for (int t = 0; t < T; ++t) {
      const int v = tokens[(long long)t * R + r];
      open = open && v >= 0;
      c[1 + t] = open ? (long long)v : pad_idx;
      len += open;
      open = open && v != end_idx;
    }
    lens[r] = len;
    n += len;
  }
  if (n) atomicAdd(&total, n);  // integers: the sum does not depend on the order
  __syncthreads();
  if (threadIdx.x == 0) {
    if (count) count[0] = total;
    inv_count[0] = 1.f / (float)total;
  }
}

__global__ void __launch_bounds__(256) cider_reward_kernel(
    const int* __restrict__ tokens, int T, int R, int n, const int* __restrict__ lens,
    const int* __restrict__ img_key, int n_images, int end_idx, int score_end,
    const unsigned long long* __restrict__ idf_keys, const float* __restrict__ idf_vals, int n_keys, float log_images,
    const unsigned long long* __restrict__ ref_keys, const float* __restrict__ ref_w,
    const int* __restrict__ ref_off, const float* __restrict__ ref_norm, const int* __restrict__ ref_bigrams,
    const int* __restrict__ img_off, float* __restrict__ reward) {
  __shared__ int tok[SCST_TMAX];
  __shared__ unsigned long long keys[4][SCST_TMAX];
  __shared__ float part[4];
  const int r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int len = lens[r];
  len = len < 0 ? 0 : (len > T ? T : len);
  if (tid < SCST_TMAX) tok[tid] = tid < len ? tokens[(long long)tid * R + r] : -1;
  __syncthreads();
  if (!score_end && len > 0 && tok[len - 1] == end_idx) --len;
  const int image = img_key[r / n];
  if (image < 0 || image >= n_images) {  // the whole workgroup: no table row to score against
    if (tid == 0) reward[r] = NAN;
    return;
  }
  // the wave's n-grams, one per lane
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
  const bool rep = valid && first;  // one lane per distinct n-gram carries its weight
  float wh = 0.f;
  if (rep) {
    const int i = key_lower_bound(idf_keys, 0, n_keys, key);
    const float idf = (i < n_keys && idf_keys[i] == key) ? idf_vals[i] : log_images;
    wh = (float)tf * idf;
  }
  const float hn = sqrtf(wave_sum(wh * wh));
  const int hl = len > 1 ? len - 1 : 0;  // the hypothesis's bigrams
  const int r0 = img_off[image], r1 = img_off[image + 1];
  float acc = 0.f;
  for (int ref = r0; ref < r1; ++ref) {
    float term = 0.f;
    if (rep) {
      const int e1 = ref_off[ref + 1];
      const int i = key_lower_bound(ref_keys, ref_off[ref], e1, key);
      if (i < e1 && ref_keys[i] == key) {
        const float wr = ref_w[i];
        term = fminf(wh, wr) * wr;
      }
    }
    float val = wave_sum(term);
    const float rn = ref_norm[(long long)ref * 4 + w];
    if (hn != 0.f && rn != 0.f) val /= hn * rn;
    const float d = (float)(hl - ref_bigrams[ref]);
    acc += val * expf(-(d * d) / CIDER_2SIGMA2);
  }
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (tid == 0) {
    const float s = ((part[0] + part[1]) + part[2]) + part[3];
    reward[r] = r1 > r0 ? s / 4.f / (float)(r1 - r0) * 10.f : 0.f;
  }
}

__global__ void __launch_bounds__(1024) scst_advantage_kernel(const float* __restrict__ reward,
                                                              const float* __restrict__ greedy, int B, int n,
                                                              int mode, float* __restrict__ adv,
                                                              float* __restrict__ stats) {
  __shared__ float red[16];
  float sr = 0.f, sg = 0.f;
  for (int b = threadIdx.x; b < B; b += 1024) {
    const float* __restrict__ x = reward + (long long)b * n;
    for (int j = 0; j < n; ++j) {
      float base;
      if (mode == CAPMI_SCST_GREEDY) {
        base = greedy[b];
      } else {
        float s = 0.f;
        for (int k = 0; k < n; ++k)
          if (k != j) s += x[k];
        base = s / (float)(n - 1);
      }
      adv[(long long)b * n + j] = x[j] - base;
      sr += x[j];
    }
    if (greedy) sg += greedy[b];
  }
  sr = block_sum(sr, red);
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    stats[0] = sr / ((float)B * (float)n);
    stats[1] = greedy ? sg / (float)B : 0.f;
  }
}

}  // namespace

extern "C" int capmi_rollout_pack(const int* tokens, int T, int R, long long start_idx, int end_idx,
                                  long long pad_idx, int* lens, long long* caps, int* count, float* inv_count,
                                  void* stream) {
  CAPMI_REQUIRE(tokens && lens && caps && inv_count && T > 0 && R > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(start_idx >= 0 && end_idx >= 0 && pad_idx >= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)R * (T + 1LL) < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(rollout_pack_kernel, dim3(1), dim3(1024), 0, as_stream(stream), tokens, T, R, start_idx, end_idx,
                     pad_idx, lens, caps, count, inv_count);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_cider_reward(const int* tokens, int T, int R, int n, const int* lens, const int* img_key,
                                  int n_images, int V, int end_idx, int score_end,
                                  const unsigned long long* idf_keys, const float* idf_vals, int n_keys,
                                  float log_images, const unsigned long long* ref_keys, const float* ref_w,
                                  const int* ref_off, const float* ref_norm, const int* ref_bigrams,
                                  const int* img_off, float* reward, void* stream) {
  CAPMI_REQUIRE(tokens && lens && img_key && ref_off && ref_norm && ref_bigrams && img_off && reward, CAPMI_EINVAL);
  // a corpus of empty references has no n-gram: the two entry tables may then be missing
  CAPMI_REQUIRE(n_keys >= 0 && (n_keys == 0 || (idf_keys && idf_vals && ref_keys && ref_w)), CAPMI_EINVAL);
  CAPMI_REQUIRE(T > 0 && T <= SCST_TMAX && R > 0 && n > 0 && R % n == 0 && n_images > 0 && V > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(end_idx >= 0 && log_images == log_images, CAPMI_EINVAL);
  CAPMI_REQUIRE(V <= 65534, CAPMI_ERANGE);  // token + 1 in 16 bits, 0 kept for 'no word'
  hipLaunchKernelGGL(cider_reward_kernel, dim3(R), dim3(256), 0, as_stream(stream), tokens, T, R, n, lens, img_key,
                     n_images, end_idx, score_end, idf_keys, idf_vals, n_keys, log_images, ref_keys, ref_w, ref_off,
                     ref_norm, ref_bigrams, img_off, reward);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_scst_advantage(const float* reward, const float* greedy_reward, int B, int n, int mode,
                                    float* adv, float* stats, void* stream) {
  CAPMI_REQUIRE(reward && adv && stats && B > 0 && n > 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(mode == CAPMI_SCST_MEAN || mode == CAPMI_SCST_GREEDY, CAPMI_EINVAL);
  CAPMI_REQUIRE(mode != CAPMI_SCST_MEAN || n >= 2, CAPMI_EINVAL);  // the mean of the other samples
  CAPMI_REQUIRE(mode != CAPMI_SCST_GREEDY || greedy_reward, CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * n < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(scst_advantage_kernel, dim3(1), dim3(1024), 0, as_stream(stream), reward, greedy_reward, B, n,
                     mode, adv, stats);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
