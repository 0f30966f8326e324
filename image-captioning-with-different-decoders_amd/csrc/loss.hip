// The captioners' training loss: cross entropy over the (B, T, V) logits, one workgroup per row r = b T + t, and
// the reductions that finish it. The row arithmetic is written once (ce_rows_kernel); the three entry points
// differ only in their form: which rows are live, what a row writes besides its gradient, and the gradient's scale.
//
//   capmi_ce_fwd_bwd         BtForm, the attention captioner: row (b, t) live iff b < bt[t] (bt NULL: every row),
//                            target caps[b L + t + 1]; loss_rows, optional lse; g = gscale / nrows
//   capmi_ce_ignore_fwd_bwd  IgnoreForm, the baseline captioner (reference models/baseline.py:114-264,
//                            nn.CrossEntropyLoss with ignore_index): live iff target != ignore_index, target
//                            caps[b L + t + tgt_off]; loss_rows; g = inv_count[0]
//   capmi_pg_ce_fwd_bwd      PgForm, both self-critical steps: live iff t_first <= t < t_first + lens[b]; logp_rows,
//                            loss_rows = -adv[b] logp; g = adv[b] inv_count[0]
//   capmi_count_targets      count = #{targets != ignore_index}, inv_count = 1 / count, both on the device: a
//                            captured step replays with any batch
//   capmi_loss_finalize      loss = sum(loss_rows) / nrows + sum(reg_part)
//   capmi_loss_finalize_dev  loss = sum(loss_rows) * inv_count[0]
//
// In every form a row that is not live, or whose target lies outside [0, V) (an error in torch; here it is never
// followed), is written, not skipped: zero row outputs and a zero gradient row. A batch with no live target:
// count = 0, inv_count = +inf, loss = 0 * inf = NaN, as torch gives. All sums are fp32 in one fixed order.
#include "common.h"

namespace {

struct BtForm {
  const int* bt;
  float inv_n;
  const float* gscale;
  float* loss_rows;
  float* lse_out;
  __device__ bool live(int b, int t, long long) const { return bt == nullptr || b < bt[t]; }
  __device__ void write_row(int r, int, float lse, float xt) const {
    loss_rows[r] = lse - xt;
    if (lse_out) lse_out[r] = lse;
  }
  __device__ void zero_row(int r) const {
    loss_rows[r] = 0.f;
    if (lse_out) lse_out[r] = 0.f;
  }
  __device__ float grad_scale(int) const { return (gscale ? *gscale : 1.f) * inv_n; }
};

struct IgnoreForm {
  long long ignore_index;
  const float* inv_count;
  float* loss_rows;
  __device__ bool live(int, int, long long tgt) const { return tgt != ignore_index; }
  __device__ void write_row(int r, int, float lse, float xt) const { loss_rows[r] = lse - xt; }
  __device__ void zero_row(int r) const { loss_rows[r] = 0.f; }
  __device__ float grad_scale(int) const { return *inv_count; }
};

struct PgForm {
  const int* lens;
  int t_first;
  const float* adv;
  const float* inv_count;
  float* logp_rows;
  float* loss_rows;
  __device__ bool live(int b, int t, long long) const { return t >= t_first && t - t_first < lens[b]; }
  __device__ void write_row(int r, int b, float lse, float xt) const {
    const float lp = xt - lse;
    logp_rows[r] = lp;
    loss_rows[r] = -adv[b] * lp;
  }
  __device__ void zero_row(int r) const {
    logp_rows[r] = 0.f;
    loss_rows[r] = 0.f;
  }
  __device__ float grad_scale(int b) const { return adv[b] * *inv_count; }
};

// Online max/sum over the row, lse, the form's row outputs, then the gradient (softmax - onehot) * g in the same
// launch (the row is L2-hot). dlogits row: r, or t B + b where the caller wants it time-major.
template <class Form>
__global__ void __launch_bounds__(256) ce_rows_kernel(const float* __restrict__ logits,
                                                      const long long* __restrict__ caps, int B, int T, int L, int V,
                                                      int tgt_off, float* __restrict__ dlogits, int tm, const Form f) {
  __shared__ float red[16];
  const int r = blockIdx.x;  // r = b*T + t
  const int b = r / T, t = r - b * T;
  const long long tgt = caps[(long long)b * L + t + tgt_off];
  const long long drow = tm ? ((long long)t * B + b) : r;
  // read ahead of every store: the form's pointers carry no restrict, and past a store that may alias it this
  // load would be a vector load and g a VGPR pair
  const float g = dlogits ? f.grad_scale(b) : 0.f;
  if (!f.live(b, t, tgt) || tgt < 0 || tgt >= V) {
    if (threadIdx.x == 0) f.zero_row(r);
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
  if (threadIdx.x == 0) f.write_row(r, b, lse, x[tgt]);
  if (dlogits)
    for (int v = threadIdx.x; v < V; v += 256) {
      const float pv = expf(x[v] - lse);
      dlogits[drow * V + v] = (pv - (v == tgt ? 1.f : 0.f)) * g;
    }
}

template <class Form>
int launch_ce_rows(const float* logits, const long long* caps, int B, int T, int L, int V, int tgt_off,
                   float* dlogits, int dl_time_major, const Form& f, void* stream) {
  hipLaunchKernelGGL(ce_rows_kernel<Form>, dim3(B * T), dim3(256), 0, as_stream(stream), logits, caps, B, T, L, V,
                     tgt_off, dlogits, dl_time_major, f);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

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

// sum of rows[0 .. n) over one workgroup, in one fixed order
__device__ __forceinline__ float sum_rows(const float* __restrict__ rows, int n, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += rows[i];
  return block_sum(s, red);
}

__global__ void __launch_bounds__(1024) loss_finalize_kernel(const float* __restrict__ rows, int n, float inv_n,
                                                             const float* __restrict__ reg, int nreg,
                                                             float* __restrict__ out) {
  __shared__ float red[16];
  const float s = sum_rows(rows, n, red);
  const float r = sum_rows(reg, nreg, red);
  if (threadIdx.x == 0) out[0] = s * inv_n + r;
}

__global__ void __launch_bounds__(1024) loss_finalize_dev_kernel(const float* __restrict__ rows, int n,
                                                                 const float* __restrict__ inv_count,
                                                                 float* __restrict__ out) {
  __shared__ float red[16];
  const float s = sum_rows(rows, n, red);
  if (threadIdx.x == 0) out[0] = s * inv_count[0];
}

}  // namespace

extern "C" int capmi_ce_fwd_bwd(const float* logits, const long long* caps, int B, int T, int L, int V, const int* bt,
                                int nrows, float* loss_rows, float* lse, float* dlogits, int dl_time_major,
                                const float* gscale, void* stream) {
  CAPMI_REQUIRE(logits && caps && loss_rows && B > 0 && T > 0 && V > 0 && L > T && nrows > 0, CAPMI_EINVAL);
  return launch_ce_rows(logits, caps, B, T, L, V, 1, dlogits, dl_time_major,
                        BtForm{bt, 1.f / (float)nrows, gscale, loss_rows, lse}, stream);
}

extern "C" int capmi_ce_ignore_fwd_bwd(const float* logits, const long long* caps, int B, int T, int L, int V,
                                       int tgt_off, long long ignore_index, const float* inv_count, float* loss_rows,
                                       float* dlogits, int dl_time_major, void* stream) {
  CAPMI_REQUIRE(logits && caps && loss_rows && B > 0 && T > 0 && V > 0 && tgt_off >= 0 && L >= T + tgt_off,
                CAPMI_EINVAL);
  CAPMI_REQUIRE(!dlogits || (inv_count && dlogits != logits), CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * T < (1LL << 31), CAPMI_ERANGE);
  return launch_ce_rows(logits, caps, B, T, L, V, tgt_off, dlogits, dl_time_major,
                        IgnoreForm{ignore_index, inv_count, loss_rows}, stream);
}

extern "C" int capmi_pg_ce_fwd_bwd(const float* logits, const long long* caps, int B, int T, int L, int V, int tgt_off,
                                   const int* lens, int t_first, const float* adv, const float* inv_count,
                                   float* logp_rows, float* loss_rows, float* dlogits, int dl_time_major,
                                   void* stream) {
  CAPMI_REQUIRE(logits && caps && lens && adv && logp_rows && loss_rows, CAPMI_EINVAL);
  CAPMI_REQUIRE(B > 0 && T > 0 && V > 0 && tgt_off >= 0 && t_first >= 0 && L >= T + tgt_off, CAPMI_EINVAL);
  CAPMI_REQUIRE(!dlogits || (inv_count && dlogits != logits), CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * T < (1LL << 31), CAPMI_ERANGE);
  return launch_ce_rows(logits, caps, B, T, L, V, tgt_off, dlogits, dl_time_major,
                        PgForm{lens, t_first, adv, inv_count, logp_rows, loss_rows}, stream);
}

extern "C" int capmi_count_targets(const long long* caps, int B, int T, int L, int tgt_off, long long ignore_index,
                                   int* count, float* inv_count, void* stream) {
  CAPMI_REQUIRE(caps && inv_count && B > 0 && T > 0 && tgt_off >= 0 && L >= T + tgt_off, CAPMI_EINVAL);
  CAPMI_REQUIRE((long long)B * T < (1LL << 31), CAPMI_ERANGE);
  hipLaunchKernelGGL(count_targets_kernel, dim3(1), dim3(1024), 0, as_stream(stream), caps, B, T, L, tgt_off,
                     ignore_index, count, inv_count);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_loss_finalize(const float* loss_rows, int n, int nrows, const float* reg_part, int nreg,
                                   float* out, void* stream) {
  CAPMI_REQUIRE(loss_rows && out && n > 0 && nrows > 0 && (nreg == 0 || reg_part), CAPMI_EINVAL);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(1024), 0, as_stream(stream), loss_rows, n,
                     1.f / (float)nrows, reg_part, nreg, out);
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
