// Device-side pieces shared by the x3 GEMM family (gemm_x3 / x3p / x3s / x3w / x3c) and, where the definition is
// the same, by gemm_bf16.hip and gemm_nt.hip: vector types, the raw-buffer descriptor, the out-of-range offset and
// the two forms of the x3 arithmetic that more than one kernel spells the same way.
#pragma once
#include "gemm_args.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

constexpr unsigned kOOB = 0x80000000u;  // buffer offset past every operand: the load returns 0, the store is dropped
constexpr int kSc1 = 16;                // buffer-op aux bit: sc1 (write-through store / L1-bypassing load)

// raw buffer descriptor over [p, p + bytes)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}

__device__ __forceinline__ bf16x4 x3_cvt4(float4 v) {
  bf16x4 r;
  r.x = (__bf16)v.x;
  r.y = (__bf16)v.y;
  r.z = (__bf16)v.z;
  r.w = (__bf16)v.w;
  return r;
}
// the exact three-term split of four fp32 values: h0 = RNE(v), h1 = RNE(v - h0), h2 = v - h0 - h1 (every
// difference exact in fp32; split3_pair in gemm_args.h is the packed-pair form of the same arithmetic)
__device__ __forceinline__ float4 x3_back4(bf16x4 h) {
  return make_float4((float)h.x, (float)h.y, (float)h.z, (float)h.w);
}
__device__ __forceinline__ float4 x3_sub4(float4 a, float4 b) {
  return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
}
__device__ __forceinline__ void x3_split4(float4 v, bf16x4& h0, bf16x4& h1, bf16x4& h2) {
  h0 = x3_cvt4(v);
  const float4 r1 = x3_sub4(v, x3_back4(h0));
  h1 = x3_cvt4(r1);
  h2 = x3_cvt4(x3_sub4(r1, x3_back4(h1)));
}

// the six kept products of one 16x16x32 block, smallest terms first into the fp32 accumulator:
// a1 b1, a0 b2, a2 b0, a0 b1, a1 b0, a0 b0
__device__ __forceinline__ f32x4 x3_mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
  return c;
}
