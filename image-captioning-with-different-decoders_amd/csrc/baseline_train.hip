// The baseline captioner's training loss (reference models/baseline.py:114-264): nn.CrossEntropyLoss with
// ignore_index over the (B, T, V) logits, target of row r = b T + t at caps[b L + t + tgt_off] (the baseline
// scores step t against caps[t]: offset 0). The number of live targets and its reciprocal live on the device,
// so a captured step replays with any batch: nothing about the count is on the host.
//
//   capmi_count_targets      count = #{targets != ignore_index}, inv_count = 1 / count
//   capmi_ce_ignore_fwd_bwd  ce_fwd_bwd_kernel's per-row arithmetic (decoder.hip); an ignored row gives
//                            loss_rows = 0 and a zero gradient row, a live one (softmax - onehot) * inv_count
//   capmi_loss_finalize_dev  loss = sum(loss_rows) * inv_count, one workgroup, fixed order
//
// A batch with no live target: count = 0, inv_count = +inf, loss = 0 * inf = NaN, as torch gives.
#include "common.h"

namespace {

__global__ void __launch_bounds__(1024) count_targets_kernel(const long long* __restrict__ caps, int B, int T, int L,
                                                             int tgt_off, long long ignore_index,
                                                             int* __restrict__ count, float* __restrict__ inv_count) {
  __shared__ int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  int n = 0;
  for (int r = threadIdx.x; r < B * T; r += 1024) {
    const int b = r / T, t = r - b * T;
    n += caps[(long long)b * L + t + tgt_off] != ignore_index;
  }
  if (n) atomicAdd(&total, n);  // integers: the sum does not depend on the order
  __syncthreads();
  if (threadIdx.x == 0) {
    if (count) count[0] = total;
    inv_count[0] = 1.f / (float)total;
  }
}

__global__ void __launch_bounds__(256) ce_ignore_fwd_bwd_kernel(const float* __restrict__ logits,
                                                                const long long* __restrict__ caps, int B, int T,
                                                                int L, int V, int tgt_off, long long ignore_index,
                                                                const float* __restrict__ inv_count,
                                                                float* __restrict__ loss_rows,
                                                                float* __restrict__ dlogits, int tm) {
  __shared__ float red[16];
  const int r = blockIdx.x;  // r = b*T + t
  const int b = r / T, t = r - b * T;
  const long long tgt = caps[(long long)b * L + t + tgt_off];
  const long long drow = tm ? ((long long)t * B + b) : r;
  // a target outside [0, V) other than ignore_index is an error in torch; here it is never followed: ignored
  if (tgt == ignore_index || tgt < 0 || tgt >= V) {
    if (threadIdx.x == 0) loss_rows[r] = 0.f;
    if (dlogits)
      for (int v = threadIdx.x; v < V; v += 256) dlogits[drow * V + v] = 0.f;
    return;
  }
  const float* x = logits + (long long)r * V;
  float m = -INFINITY, s = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float xv = x[v];
    if (xv > m) {
      s = s * expf(m - xv) + 1.f;
      m = xv;
    } else {
      s += expf(xv - m);
    }
  }
  const float gm = block_max(m, red);
  s = (m == -INFINITY) ? 0.f : s * expf(m - gm);
  s = block_sum(s, red);
  const float lse = gm + logf(s);
  if (threadIdx.x == 0) loss_rows[r] = lse - x[tgt];
  if (dlogits) {
    const float g = *inv_count;
    for (int v = threadIdx.x; v < V; v += 256) {
      const float pv = expf(x[v] - lse);
      dlogits[drow * V + v] = (pv - (v == tgt ? 1.f : 0.f)) * g;
    }
  }
}

__global__ void __launch_bounds__(1024) loss_finalize_dev_kernel(const float* __restrict__ rows, int n,
                                                                 const float* __restrict__ inv_count,
                                                                 float* __restrict__ out) {
  __shared__ float red[16];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += rows[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s * inv_count[0];
}

}  // namespace

extern "C" int capmi_count_targets(const long long* caps, int B, int T, int L, int tgt_off, long long ignore_index,
                                   int* count, float* inv_count, void* stream) {
  CAPMI_REQUIRE(caps && inv_count && B > 0 && T > 0 && tgt_off >= 0 && L >= T + tgt_off, CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * T < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(count_targets_kernel, dim3(1), dim3(1024), 0, as_stream(stream), caps, B, T, L, tgt_off,
                     ignore_index, count, inv_count);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_ce_ignore_fwd_bwd(const float* logits, const long long* caps, int B, int T, int L, int V,
                                       int tgt_off, long long ignore_index, const float* inv_count, float* loss_rows,
                                       float* dlogits, int dl_time_major, void* stream) {
  CAPMI_REQUIRE(logits && caps && loss_rows && B > 0 && T > 0 && V > 0 && tgt_off >= 0 && L >= T + tgt_off,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(!dlogits || (inv_count && dlogits != logits), CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * T < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(ce_ignore_fwd_bwd_kernel, dim3(B * T), dim3(256), 0, as_stream(stream), logits, caps, B, T, L,
                     V, tgt_off, ignore_index, inv_count, loss_rows, dlogits, dl_time_major);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_loss_finalize_dev(const float* loss_rows, int n, const float* inv_count, float* out,
                                       void* stream) {
  CAPMI_REQUIRE(loss_rows && inv_count && out && n > 0, CAPMI_EINVAL);
  hipLaunchKernelGGL(loss_finalize_dev_kernel, dim3(1), dim3(1024), 0, as_stream(stream), loss_rows, n, inv_count,
                     out);
  CAPMI_LAUNCH_CHECK();
  return 0;
}
