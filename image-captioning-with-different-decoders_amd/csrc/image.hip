// Image preprocessing on the GPU: the reference's per-image CPU transform
// Resize((224, 224)) -> ToTensor -> Normalize(mean, std) (models/attention.py:296-301, applied in
// dataset.py:55-59 by DataLoader workers) as two kernels over a batch of decoded uint8 RGB images
// of any sizes. Only the JPEG decode stays on the host; the uint8 pixels (4x fewer bytes than the
// fp32 tensor) cross PCIe.
//
// Resize is torchvision's PIL path (Image.resize(size, BILINEAR), reducing_gap None), restated
// from Pillow's Resample.c so that the result is bit-identical to it:
//   * separable antialiasing triangle filter, support = max(1, in/out); per output index the taps
//     [xmin, xmin + xmax) and weights w = f((x + xmin - center + 0.5) / filterscale) normalised to
//     sum 1 in double (precompute_coeffs), then 22-bit fixed point (normalize_coeffs_8bpc);
//   * horizontal pass first, rounded to uint8 (clip8: (acc + 2^21) >> 22, clamped), then the
//     vertical pass over that intermediate, rounded to uint8 again;
// the double arithmetic is evaluated in Pillow's order with FMA contraction off. ToTensor +
// Normalize: (u8 / 255.f - mean[c]) / std[c] in fp32, as torchvision does it.
//
// The device image cache splits that in two: capmi_resize_u8_slots stores the resampled uint8 image
// into a slot of a resident cache, once per image and run, and capmi_gather_normalize_u8 turns the slots a batch
// names into the normalised fp32 tensor, every step, with the same expression and so the same bits.
#include <cmath>

#include "common.h"

namespace {

constexpr int kPrec = 22;  // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for ONE output index `xx`: fills k[0..n)
// (fixed point) and returns the first source index; n = the tap count (<= kmax).
#pragma clang fp contract(off)
__device__ int resample_taps(int in_size, int out_size, int xx, int kmax, int* k, int* n) {
  const double scale = (double)(float)in_size / out_size;  // (in1 - in0) / outSize, box as floats
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;                 // bilinear support 1.0
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > kmax) xmax = kmax;  // never for kmax = 2*ceil(support)+1 (host-checked)
  double w[32];
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = (x + xmin - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    const double v = t < 1.0 ? 1.0 - t : 0.0;
    w[x] = v;
    ww += v;
  }
  for (int x = 0; x < xmax; ++x) {
    double v = w[x];
    if (ww != 0.0) v /= ww;
    k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrec)) : (int)(0.5 + v * (1 << kPrec));
  }
  *n = xmax;
  return xmin;
}
#pragma clang fp contract(on)

__device__ __forceinline__ unsigned char clip8(int acc) {
  const int v = acc >> kPrec;  // arithmetic shift: floor, as Pillow's lookup index
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// horizontal pass: tmp[b][y][ox][c] (uint8) for every source row y of image b
__global__ void resize_h_kernel(const unsigned char* __restrict__ src, const long long* __restrict__ offs,
                                const int* __restrict__ hs, const int* __restrict__ ws, int OW, int Hmax, int kmax,
                                unsigned char* __restrict__ tmp) {
  const int b = blockIdx.z, y = blockIdx.y;
  const int H = hs[b], W = ws[b];
  if (y >= H) return;
  const unsigned char* row = src + offs[b] + (long long)y * W * 3;
  unsigned char* out = tmp + (((long long)b * Hmax + y) * OW) * 3;
  for (int ox = blockIdx.x * blockDim.x + threadIdx.x; ox < OW; ox += gridDim.x * blockDim.x) {
    int k[32], n;
    const int x0 = resample_taps(W, OW, ox, kmax, k, &n);
    int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
    for (int i = 0; i < n; ++i) {
      const unsigned char* p = row + (x0 + i) * 3;
      s0 += p[0] * k[i];
      s1 += p[1] * k[i];
      s2 += p[2] * k[i];
    }
    out[ox * 3 + 0] = clip8(s0);
    out[ox * 3 + 1] = clip8(s1);
    out[ox * 3 + 2] = clip8(s2);
  }
}

// vertical pass + ToTensor + Normalize: out[b][c][oy][ox] fp32
__global__ void resize_v_norm_kernel(const unsigned char* __restrict__ tmp, const int* __restrict__ hs, int OH,
                                     int OW, int Hmax, int kmax, float m0, float m1, float m2, float s0_,
                                     float s1_, float s2_, float* __restrict__ out) {
  const int b = blockIdx.z, oy = blockIdx.y;
  const int H = hs[b];
  int k[32], n;
  const int y0 = resample_taps(H, OH, oy, kmax, k, &n);
  const unsigned char* base = tmp + ((long long)b * Hmax) * OW * 3;
  const long long plane = (long long)OH * OW;
  float* ob = out + (long long)b * 3 * plane + (long long)oy * OW;
  for (int ox = blockIdx.x * blockDim.x + threadIdx.x; ox < OW; ox += gridDim.x * blockDim.x) {
    int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
      const unsigned char* p = base + ((long long)(y0 + i) * OW + ox) * 3;
      a0 += p[0] * k[i];
      a1 += p[1] * k[i];
      a2 += p[2] * k[i];
    }
    ob[ox] = ((float)clip8(a0) / 255.f - m0) / s0_;
    ob[plane + ox] = ((float)clip8(a1) / 255.f - m1) / s1_;
    ob[2 * plane + ox] = ((float)clip8(a2) / 255.f - m2) / s2_;
  }
}

// vertical pass into the image cache: the same rounded bytes, stored as they are (HWC) into slots[slot[b]]
__global__ void resize_v_slots_kernel(const unsigned char* __restrict__ tmp, const int* __restrict__ hs,
                                      const int* __restrict__ slot, long long n_slots, int OH, int OW, int Hmax,
                                      int kmax, unsigned char* __restrict__ slots) {
  const int b = blockIdx.z, oy = blockIdx.y;
  const long long sl = slot[b];
  if (sl < 0 || sl >= n_slots) return;
  const int H = hs[b];
  int k[32], n;
  const int y0 = resample_taps(H, OH, oy, kmax, k, &n);
  const unsigned char* base = tmp + ((long long)b * Hmax) * OW * 3;
  unsigned char* ob = slots + ((sl * OH + oy) * OW) * 3;
  for (int ox = blockIdx.x * blockDim.x + threadIdx.x; ox < OW; ox += gridDim.x * blockDim.x) {
    int a0 = 1 << (kPrec - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
      const unsigned char* p = base + ((long long)(y0 + i) * OW + ox) * 3;
      a0 += p[0] * k[i];
      a1 += p[1] * k[i];
      a2 += p[2] * k[i];
    }
    ob[ox * 3 + 0] = clip8(a0);
    ob[ox * 3 + 1] = clip8(a1);
    ob[ox * 3 + 2] = clip8(a2);
  }
}

struct Norm3 {
  float m[3], s[3];
};

__device__ __forceinline__ float norm_u8(unsigned v, float m, float s) { return ((float)v / 255.f - m) / s; }

// ToTensor + Normalize of cached images. An image is flat on both sides: P = OH*OW pixels of 3 bytes in its slot,
// three planes of P floats in `out`. Four pixels per lane: 12 consecutive source bytes (three dwords; consecutive
// lanes read consecutive 12-B groups) and one 16-B store per plane. Needs P % 4 == 0, slots 4-B and out 16-B
// aligned (the host picks the kernel): then every slot and every plane starts aligned.
__global__ void gather_norm4_kernel(const unsigned char* __restrict__ slots, long long n_slots,
                                    const int* __restrict__ slot, int P4, Norm3 nm, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long sl = slot[b];
  if (sl < 0 || sl >= n_slots) return;
  const long long P = (long long)P4 * 4;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(slots + sl * P * 3);
  float* ob = out + (long long)b * 3 * P;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < P4; g += gridDim.x * blockDim.x) {
    const uint32_t w0 = src[3 * g], w1 = src[3 * g + 1], w2 = src[3 * g + 2];  // r0g0b0r1 g1b1r2g2 b2r3g3b3
    float4 r, gr, bl;
    r.x = norm_u8(w0 & 255u, nm.m[0], nm.s[0]);
    gr.x = norm_u8((w0 >> 8) & 255u, nm.m[1], nm.s[1]);
    bl.x = norm_u8((w0 >> 16) & 255u, nm.m[2], nm.s[2]);
    r.y = norm_u8(w0 >> 24, nm.m[0], nm.s[0]);
    gr.y = norm_u8(w1 & 255u, nm.m[1], nm.s[1]);
    bl.y = norm_u8((w1 >> 8) & 255u, nm.m[2], nm.s[2]);
    r.z = norm_u8((w1 >> 16) & 255u, nm.m[0], nm.s[0]);
    gr.z = norm_u8(w1 >> 24, nm.m[1], nm.s[1]);
    bl.z = norm_u8(w2 & 255u, nm.m[2], nm.s[2]);
    r.w = norm_u8((w2 >> 8) & 255u, nm.m[0], nm.s[0]);
    gr.w = norm_u8((w2 >> 16) & 255u, nm.m[1], nm.s[1]);
    bl.w = norm_u8(w2 >> 24, nm.m[2], nm.s[2]);
    reinterpret_cast<float4*>(ob)[g] = r;
    reinterpret_cast<float4*>(ob + P)[g] = gr;
    reinterpret_cast<float4*>(ob + 2 * P)[g] = bl;
  }
}

// the same, one pixel per lane: any P, any alignment
__global__ void gather_norm1_kernel(const unsigned char* __restrict__ slots, long long n_slots,
                                    const int* __restrict__ slot, long long P, Norm3 nm, float* __restrict__ out) {
  const int b = blockIdx.y;
  const long long sl = slot[b];
  if (sl < 0 || sl >= n_slots) return;
  const unsigned char* src = slots + sl * P * 3;
  float* ob = out + (long long)b * 3 * P;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long long)gridDim.x * blockDim.x) {
    ob[p] = norm_u8(src[3 * p], nm.m[0], nm.s[0]);
    ob[P + p] = norm_u8(src[3 * p + 1], nm.m[1], nm.s[1]);
    ob[2 * P + p] = norm_u8(src[3 * p + 2], nm.m[2], nm.s[2]);
  }
}

}  // namespace

extern "C" int capmi_resize_taps_max(int in_size, int out_size) {
  if (in_size <= 0 || out_size <= 0) return -CAPMI_EINVAL;
  const double scale = (double)in_size / out_size;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

extern "C" int capmi_resize_normalize_u8(const unsigned char* src, const long long* offsets, const int* heights,
                                         const int* widths, int B, int max_h, int max_w, int OH, int OW,
                                         const float* mean, const float* std, void* tmp, float* out,
                                         void* stream) {
  CAPMI_REQUIRE(src && offsets && heights && widths && mean && std && tmp && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(B >= 0 && max_h > 0 && max_w > 0 && OH > 0 && OW > 0, CAPMI_EINVAL);
  if (B == 0) return 0;
  // taps per output index: the largest reduction factor over both axes and every image
  const int kmax = std::max(capmi_resize_taps_max(max_w, OW), capmi_resize_taps_max(max_h, OH));
  CAPMI_REQUIRE(kmax <= 32, CAPMI_ERANGE);  // reductions up to 15x
  CAPMI_REQUIRE(B <= 65535 && max_h <= 65535 && OH <= 65535, CAPMI_ERANGE);
  hipStream_t s = as_stream(stream);
  const int tx = std::min(256, OW);
  hipLaunchKernelGGL(resize_h_kernel, dim3(cdiv(OW, tx), max_h, B), dim3(tx), 0, s, src, offsets, heights, widths,
                     OW, max_h, kmax, static_cast<unsigned char*>(tmp));
  CAPMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(resize_v_norm_kernel, dim3(cdiv(OW, tx), OH, B), dim3(tx), 0, s,
                     static_cast<const unsigned char*>(tmp), heights, OH, OW, max_h, kmax, mean[0], mean[1], mean[2],
                     std[0], std[1], std[2], out);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_resize_u8_slots(const unsigned char* src, const long long* offsets, const int* heights,
                                     const int* widths, const int* slot, int n, int max_h, int max_w, int OH, int OW,
                                     void* tmp, unsigned char* slots, long long n_slots, void* stream) {
  CAPMI_REQUIRE(src && offsets && heights && widths && slot && tmp && slots, CAPMI_EINVAL);
  CAPMI_REQUIRE(n >= 0 && max_h > 0 && max_w > 0 && OH > 0 && OW > 0 && n_slots > 0, CAPMI_EINVAL);
  if (n == 0) return 0;
  const int kmax = std::max(capmi_resize_taps_max(max_w, OW), capmi_resize_taps_max(max_h, OH));
  CAPMI_REQUIRE(kmax <= 32, CAPMI_ERANGE);  // reductions up to 15x
  CAPMI_REQUIRE(n <= 65535 && max_h <= 65535 && OH <= 65535, CAPMI_ERANGE);
  hipStream_t s = as_stream(stream);
  const int tx = std::min(256, OW);
  hipLaunchKernelGGL(resize_h_kernel, dim3(cdiv(OW, tx), max_h, n), dim3(tx), 0, s, src, offsets, heights, widths, OW,
                     max_h, kmax, static_cast<unsigned char*>(tmp));
  CAPMI_LAUNCH_CHECK();
  hipLaunchKernelGGL(resize_v_slots_kernel, dim3(cdiv(OW, tx), OH, n), dim3(tx), 0, s,
                     static_cast<const unsigned char*>(tmp), heights, slot, n_slots, OH, OW, max_h, kmax, slots);
  CAPMI_LAUNCH_CHECK();
  return 0;
}

extern "C" int capmi_gather_normalize_u8(const unsigned char* slots, long long n_slots, const int* slot, int B, int OH,
                                         int OW, const float* mean, const float* std, float* out, void* stream) {
  CAPMI_REQUIRE(slots && slot && mean && std && out, CAPMI_EINVAL);
  CAPMI_REQUIRE(n_slots > 0 && B >= 0 && OH > 0 && OW > 0, CAPMI_EINVAL);
  if (B == 0) return 0;
  CAPMI_REQUIRE(B <= 65535, CAPMI_ERANGE);
  const long long P = (long long)OH * OW;
  CAPMI_REQUIRE(P <= 0x7fffffffLL, CAPMI_ERANGE);
  Norm3 nm;
  for (int c = 0; c < 3; ++c) nm.m[c] = mean[c], nm.s[c] = std[c];
  hipStream_t s = as_stream(stream);
  if (P % 4 == 0 && (reinterpret_cast<uintptr_t>(slots) & 3u) == 0 && aligned16(out)) {
    const int P4 = (int)(P / 4);
    hipLaunchKernelGGL(gather_norm4_kernel, dim3(cdiv(P4, 256), B), dim3(256), 0, s, slots, n_slots, slot, P4, nm, out);
  } else {
    hipLaunchKernelGGL(gather_norm1_kernel, dim3(cdiv(P, 256), B), dim3(256), 0, s, slots, n_slots, slot, P, nm, out);
  }
  CAPMI_LAUNCH_CHECK();
  return 0;
}
