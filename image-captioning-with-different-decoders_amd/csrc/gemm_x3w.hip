// fp32-accurate conv WEIGHT gradient on the bf16 matrix cores ("x3w", round 4): C[m][n] = sum_k A[k][m] B[k][n],
// k = output pixel, A = dY (the conv output's gradient, fp32 [pixel][Cout]) and B = the conv input relu(bn(y))
// as fp32 k rows ([pixel][Cin]: a 1x1 conv) or the implicit im2col of the NHWC input (n = (kh, kw, ci), the
// packed weight order; stride / padding taps read zeros), the BN-apply + ReLU applied to B in the kernel
// (in_scale / in_shift). Replaces the weight-gradient half of nn.Conv2d's backward for the trainable layer2-4
// convs of EncoderAttention.fine_tune (models/encoder.py:112-121, driven by models/attention.py:417-430).
//
// Both operands are K-OUTER in memory (a k-tile is 32 pixel rows of channels): the transpose of what the MFMA
// takes (each lane 8 consecutive k of one m / n). Each thread loads its fp32 float4s of the next k-tile while
// the current one is multiplied, then splits them exactly into the three bf16 terms of gemm_x3 (split3_pair)
// and stores them row-major into a swizzled LDS image; the MFMA operands are read back with
// ds_read_b64_tr_b16, which hands each 16-lane group a 4 k-row x 16-column block column-major, so two reads
// give a lane its 8 consecutive k. x3 arithmetic (six cross products above 2^-23 |a||b|, fp32 accumulation,
// smallest terms first); tile 256 x 128 (M x N), 512 threads as 4 x 2 waves of 64 x 64 (16 blocks of
// v_mfma_f32_16x16x32_bf16 x 6 products per 32-deep k-tile), LDS double buffer of 2 x 72 KiB, one barrier
// per k-tile. A weight gradient has few output tiles (layer3's 3x3: 18) and a long k (12544 pixels at
// batch 64): the k range is split S ways so the grid fills the CUs, and the S partial slabs are summed in a
// fixed order afterwards (deterministic). It replaces the split-staging nts kernel's weight gradients (round-3
// VERDICT: 0.26 of the x3 bound, 244 MB per launch against 28 MB).
// gemm_w16_kernel (round 6, CAPMI_GEMM_X3W | CAPMI_GEMM_BF16): the same kernel with one term per operand -- each
// fp32 value rounded to bf16 (RNE, the CAPMI_GEMM_BF16 operand contract) and one product per block -- for the
// bf16 configuration's decoder weight gradients (capmi/decoder_core.py).
#include "x3_common.h"

namespace {

constexpr int WBM = 256, WBN = 128, WBK = 32, WNT = 512;
constexpr int WA_ROWB = WBM * 2;            // bytes per A k-row per plane (256 bf16)
constexpr int WB_ROWB = WBN * 2;            // bytes per B k-row per plane (128 bf16)
constexpr int WA_PLANE = WBK * WA_ROWB;     // 16 KiB
constexpr int WB_PLANE = WBK * WB_ROWB;     // 8 KiB
constexpr int WA_BYTES = 3 * WA_PLANE;      // 48 KiB
constexpr int WBUF = WA_BYTES + 3 * WB_PLANE;  // 72 KiB per buffer
typedef short s16x4_w __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4_w* lds_s16x4_w;

// 16-B chunk c of k-row r is stored in slot c ^ wsw(r). A transposed read's 32-lane half takes k-rows
// {8h .. 8h+3, 8h+8 .. 8h+11} (or those + 4) x the same 32 bytes of columns; rows 256 / 512 B apart share
// their banks, so the XOR by 2 x (the row's index in that set of 8) puts the 16 chunks on 16 distinct slots
// of the 64-bank window (conflict-free)
__device__ __forceinline__ int wsw(int r) { return ((r & 3) | (((r >> 3) & 1) << 2)) << 1; }

// one ds_read_b64_tr_b16: the 4 k-rows r0 + (lane & 15) / 4 ... of this lane's group, columns c0 + 4 (lane & 3)
__device__ __forceinline__ s16x4_w tr_read(const unsigned char* plane, int rowb, int r, int col) {
  const int off = r * rowb + ((((col >> 3) ^ wsw(r))) << 4) + ((col & 4) << 1);
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_w)(plane + off));
}

// BMODE: CAPMI_B_KROWS (1, B dense k rows) or CAPMI_B_CONV_NHWC (2, implicit im2col of the conv input);
// SK: k-split into partial slabs (the grid's S > 1); TERMS: 3 (x3) or 1 (bf16 operands)
template <int BMODE, bool SK, int TERMS>
__device__ __forceinline__ void wgrad_body(const GemmArgs& args) {
  static_assert(TERMS == 3 || TERMS == 1, "terms");
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * WBUF];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wid >> 1) * 64, wn0 = (wid & 1) * 64;
  f32x4 acc4[4][4];

  auto mainloop = [&](const capmi_gemm_problem& P, int m0, int n0, int k_lo, int k_hi) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc4[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkt = (k_hi - k_lo + WBK - 1) / WBK;
    if (nkt <= 0) return;
    const int M = P.M, N = P.N;
    const long long planeB = BMODE == 2 ? (long long)P.cN * P.cH * P.cW * P.cCin : (long long)P.K * P.ldb;
    const auto ra = buf_rsrc(P.A, (unsigned)((long long)P.K * P.lda * 4));
    const auto rb = buf_rsrc(P.B, (unsigned)(planeB * 4));
    // prologue scale / shift through descriptors sized to the channel count (a read past it returns 0)
    const unsigned ss_bytes = P.in_scale ? (unsigned)((BMODE == 2 ? P.cCin : N) * 4) : 0u;
    const auto rsc = buf_rsrc(P.in_scale ? (const void*)P.in_scale : P.A, ss_bytes);
    const auto rsh = buf_rsrc(P.in_shift ? (const void*)P.in_shift : P.A, ss_bytes);
    // A = dY fp32 [k][lda]: a k-tile is 32 rows x 256 columns = 2048 float4, 4 per thread: float4 f =
    // tid + 512 i is row tid / 64 + 8 i, columns m0 + 4 (tid % 64) (one wave writes one whole LDS row)
    const int a_c4 = tid & 63, a_r0 = tid >> 6;
    const bool a_mok = m0 + 4 * a_c4 < M;
    // B fp32 [k][ldb] or the conv input: 32 rows x 128 columns = 1024 float4, 2 per thread: row tid / 32 + 16 i,
    // columns n0 + 4 (tid % 32); a thread keeps its n (and so its tap and channels) for the whole k-loop
    const int b_c4 = tid & 31, b_r0 = tid >> 5;
    const int b_n = n0 + 4 * b_c4;
    const bool b_nok = b_n < N;
    int b_ci = b_n, b_kh = 0, b_kw = 0;
    if (BMODE == 2) {
      const int tap = b_n / P.cCin;
      b_ci = b_n - tap * P.cCin;
      b_kh = tap / P.cKW;
      b_kw = tap - b_kh * P.cKW;
    }
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool pro = P.in_scale != nullptr;
    if (pro && b_nok) {
      sc = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsc, (unsigned)b_ci * 4u, 0, 0));
      sh = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsh, (unsigned)b_ci * 4u, 0, 0));
    }
    // conv B: each of the thread's two k-rows walks pixels k_lo + b_r0 + 16 i, + 32 per k-tile; its (image,
    // oh, ow) advances by 32 pixels = dq output rows + dr columns without a division (the load past the
    // last k-tile may step past the last image: it is masked by pix < k_hi)
    const int dq = WBK / max(P.cWo, 1), dr = WBK - dq * max(P.cWo, 1);
    int pn[2] = {0, 0}, poh[2] = {0, 0}, pow_[2] = {0, 0};
    if (BMODE == 2) {
      const int hw = P.cHo * P.cWo;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int pix = k_lo + b_r0 + 16 * i;
        pn[i] = pix / hw;
        const int rem = pix - pn[i] * hw;
        poh[i] = rem / P.cWo;
        pow_[i] = rem - poh[i] * P.cWo;
      }
    }
    // one register set, two k-tiles deep (round 4): during tile kt's MFMAs each of the thread's six float4
    // pieces (4 of dY, 2 of the input) is split from its register into LDS for tile kt + 1 and at once reloaded
    // with tile kt + 2's -- the load has a whole k-tile to land, and the split's VALU / ds_writes interleave with
    // the MFMAs instead of standing between two k-tiles
    float4 ra4[4], rb4[2];
    unsigned bmask = 0;
    auto load_piece = [&](int kt, int pc) {
      const int k = k_lo + kt * WBK;
      if (pc < 4) {
        const int row = k + a_r0 + 8 * pc;
        const bool ok = a_mok && row < k_hi;
        ra4[pc] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 ra, ok ? (unsigned)(((long long)row * P.lda + m0 + 4 * a_c4) * 4) : kOOB, 0, 0));
        return;
      }
      const int i = pc - 4;
      const int pix = k + b_r0 + 16 * i;
      unsigned off = kOOB;
      if (BMODE == 2) {
        const int ih = poh[i] * P.cStride - P.cPad + b_kh, iw = pow_[i] * P.cStride - P.cPad + b_kw;
        if (b_nok && pix < k_hi && (unsigned)ih < (unsigned)P.cH && (unsigned)iw < (unsigned)P.cW)
          off = (unsigned)(((pn[i] * P.cH + ih) * P.cW + iw) * P.cCin + b_ci) * 4u;
        // the next k-tile's pixel (a piece's loads are issued in k-tile order)
        // (selects, no branch: the host guarantees dq + 1 < 2 Ho, so two wraps of oh suffice)
        pow_[i] += dr;
        poh[i] += dq;
        const bool cw = pow_[i] >= P.cWo;
        pow_[i] -= cw ? P.cWo : 0;
        poh[i] += cw;
#pragma unroll
        for (int w2 = 0; w2 < 2; ++w2) {
          const bool ch = poh[i] >= P.cHo;
          poh[i] -= ch ? P.cHo : 0;
          pn[i] += ch;
        }
      } else if (b_nok && pix < k_hi) {
        off = (unsigned)(((long long)pix * P.ldb + b_n) * 4);
      }
      rb4[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rb, off, 0, 0));
      bmask = (bmask & ~(1u << i)) | ((unsigned)(off != kOOB) << i);
    };
    // registers -> (B: BN-apply + ReLU, padding taps zero AFTER it) -> three swizzled bf16 planes
    auto store_piece = [&](int buf, int pc) {
      unsigned char* base = lds + buf * WBUF;
      if (pc < 4) {
        const int r = a_r0 + 8 * pc;
        const int o = r * WA_ROWB + (((a_c4 >> 1) ^ wsw(r)) << 4) + (a_c4 & 1) * 8;
        unsigned lo[3], hi[3];  // (TERMS = 1: only term 0 = RNE(x) is stored; the rest is dead code)
        split3_pair(ra4[pc].x, ra4[pc].y, lo);
        split3_pair(ra4[pc].z, ra4[pc].w, hi);
#pragma unroll
        for (int p = 0; p < TERMS; ++p) *reinterpret_cast<uint2*>(base + p * WA_PLANE + o) = make_uint2(lo[p], hi[p]);
        return;
      }
      const int i = pc - 4;
      const int r = b_r0 + 16 * i;
      const int o = r * WB_ROWB + (((b_c4 >> 1) ^ wsw(r)) << 4) + (b_c4 & 1) * 8;
      // (no branch: the piece shares a scheduling region with MFMAs; without the prologue sc / sh are 1 / 0,
      // and relu(x) could differ from x -- so select)
      const float4 u = rb4[i];
      const float4 f = make_float4(fmaxf(fmaf(u.x, sc.x, sh.x), 0.f), fmaxf(fmaf(u.y, sc.y, sh.y), 0.f),
                                   fmaxf(fmaf(u.z, sc.z, sh.z), 0.f), fmaxf(fmaf(u.w, sc.w, sh.w), 0.f));
      const bool keep = (bmask >> i) & 1u;
      float4 v;
      v.x = keep ? (pro ? f.x : u.x) : 0.f;
      v.y = keep ? (pro ? f.y : u.y) : 0.f;
      v.z = keep ? (pro ? f.z : u.z) : 0.f;
      v.w = keep ? (pro ? f.w : u.w) : 0.f;
      unsigned lo[3], hi[3];
      split3_pair(v.x, v.y, lo);
      split3_pair(v.z, v.w, hi);
#pragma unroll
      for (int p = 0; p < TERMS; ++p)
        *reinterpret_cast<uint2*>(base + WA_BYTES + p * WB_PLANE + o) = make_uint2(lo[p], hi[p]);
    };
    // transposed fragment reads: lane l of group g = l / 16 takes k-rows 8g + (l & 15) / 4 (+ 4), columns
    // base + 4 (l & 3); it receives column l & 15 of those 4 rows, k = 8g .. 8g + 3 (+ 4 .. 7)
    const int g8 = (lane >> 4) * 8, q = (lane & 15) >> 2, c4 = (lane & 3) * 4;
    // tile kt from buffer buf: its fragments, then four 24-MFMA blocks with the six pieces of tile kt + 1 split
    // into buffer buf ^ 1 (last read by the previous step; barrier since) and reloaded with tile kt + 2
    auto step = [&](int kt, int buf) {
      const unsigned char* A_ = lds + buf * WBUF;
      const unsigned char* B_ = A_ + WA_BYTES;
      auto frag = [&](const unsigned char* plane, int rowb, int col) {
        const s16x4_w lo = tr_read(plane, rowb, g8 + q, col);
        const s16x4_w hi = tr_read(plane, rowb, g8 + 4 + q, col);
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      };
      bf16x8 b[4][TERMS];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int p = 0; p < TERMS; ++p) b[j][p] = frag(B_ + p * WB_PLANE, WB_ROWB, wn0 + 16 * j + c4);
      // A fragments one 16-row block at a time (12 VGPRs live instead of 48)
      bf16x8 a[TERMS];
#pragma unroll
      for (int p = 0; p < TERMS; ++p) a[p] = frag(A_ + p * WA_PLANE, WA_ROWB, wm0 + c4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bf16x8 an[TERMS];
        if (i + 1 < 4) {
#pragma unroll
          for (int p = 0; p < TERMS; ++p) an[p] = frag(A_ + p * WA_PLANE, WA_ROWB, wm0 + 16 * (i + 1) + c4);
        }
        __builtin_amdgcn_sched_barrier(0);
        // pieces i (and 2 + i for i >= 2: the input's two) of tile kt + 1 -> LDS, then their tile kt + 2 loads
        store_piece(buf ^ 1, i);
        if (i >= 2) store_piece(buf ^ 1, 2 + i);
        load_piece(kt + 2, i);
        if (i >= 2) load_piece(kt + 2, 2 + i);
        // per accumulator the six products smallest terms first (gemm_x3p.hip's order); one term: a0 b0
        if constexpr (TERMS == 3) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[j][1], acc4[i][j], 0, 0, 0);
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[j][2], acc4[i][j], 0, 0, 0);
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[j][0], acc4[i][j], 0, 0, 0);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[j][1], acc4[i][j], 0, 0, 0);
            acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[j][0], acc4[i][j], 0, 0, 0);
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc4[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[j][0], acc4[i][j], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < (TERMS == 3 ? 24 : 4); ++r) {  // one MFMA, then up to two VALU (the piece's split)
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (i + 1 < 4) {
#pragma unroll
          for (int p = 0; p < TERMS; ++p) a[p] = an[p];
        }
      }
      __syncthreads();
    };
    // tile 0 split into buffer 0 up front, tile 1 loaded; the last step splits the (all-zero, OOB) tile past the
    // end into the idle buffer, and its loads past the end read zeros
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) load_piece(0, pc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) store_piece(0, pc);
#pragma unroll
    for (int pc = 0; pc < 6; ++pc) load_piece(1, pc);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) step(kt, kt & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the loads past the end: drained before the epilogue)
  };

  // epilogue: C (fp32, ldc) = alpha A.B (+ beta C); 16x16 blocks: lane l holds rows 4 (l / 16) .. + 3 of
  // column l % 16 of each block
  auto epilogue = [&](const capmi_gemm_problem& P, int tm, int tn) {
    const int M = P.M, N = P.N;
    const int m0 = tm * WBM, n0 = tn * WBN;
    const float alpha = P.alpha * (P.alpha_ptr ? *P.alpha_ptr : 1.f);
    const float beta = P.beta;
    float* C = P.C;
    const long long ldc = P.ldc;
    const int cl = lane & 15, rq = lane >> 4;
    if (args.plain_epi) {  // store-only form (host: plain_epilogue): 16 row offsets per lane once
      const auto rc = buf_rsrc(C, (unsigned)((long long)M * ldc * 4));
      unsigned roff[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wm0 + 16 * i + 4 * rq + r;
          roff[i][r] = row < M ? (unsigned)row * (unsigned)ldc * 4u : kOOB;
        }
      const unsigned cb = (unsigned)(n0 + wn0 + cl) * 4u;
      float cold[4][4][4];  // + beta C: all loads before the first store (they may alias: no interleaving)
      if (args.plain_epi == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              cold[i][j][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rc, roff[i][r] + cb + 64u * j, 0, 0));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float v = acc4[i][j][r];
            if (args.plain_epi == 2) v = fmaf(beta, cold[i][j][r], v);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, roff[i][r] + cb + 64u * j, 0, 0);
          }
      return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = n0 + wn0 + 16 * j + cl;
      if (col >= N) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + wm0 + 16 * i + 4 * rq + r;
          if (row < M) {
            float* cp = C + (long long)row * ldc + col;
            float v = acc4[i][j][r] * alpha;
            if (beta != 0.f) v = fmaf(beta, *cp, v);
            *cp = v;
          }
        }
    }
  };

  // grid = tiles x S k-splits (S = args.kchunk[0] k-tiles each; the host reduces the S partial slabs with
  // capmi_splitk_reduce, a fixed order: deterministic). XCD-aware order: blocks of one XCD (blockIdx % 8)
  // are contiguous in bid, and bid = z * tiles + t, so an XCD runs the tiles of one k-chunk z: the chunk's
  // dY rows are read into that XCD's L2 once for all its tiles
  const capmi_gemm_problem& P = args.p[0];
  const int tiles_n = args.tiles_n[0], tiles = args.tiles_m[0] * tiles_n;
  int bid = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, x = bid & 7;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
  }
  const int z = bid / tiles, t = bid - z * tiles;
  const int tm = t / tiles_n, tn = t - tm * tiles_n;
  const int kc = args.kchunk[0] * WBK;
  const int k_lo = z * kc, k_hi = min(P.K, k_lo + kc);
  mainloop(P, tm * WBM, tn * WBN, k_lo, k_hi);
  if (!SK) {
    epilogue(P, tm, tn);
    return;
  }
  // k-split: the raw partial into slab z of the workspace ([S][M][ldp], ldp = tiles_n * WBN)
  const int ldp = tiles_n * WBN;
  const auto rc = buf_rsrc(args.sk_part + (long long)z * P.M * ldp, (unsigned)((long long)P.M * ldp * 4));
  const int cl = lane & 15, rq = lane >> 4;
  const int m0 = tm * WBM, n0 = tn * WBN;
  const unsigned cb = (unsigned)(n0 + wn0 + cl) * 4u;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = m0 + wm0 + 16 * i + 4 * rq + r;
      const unsigned ro = row < P.M ? (unsigned)row * (unsigned)ldp * 4u : kOOB;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc4[i][j][r]), rc, ro + cb + 64u * j, 0, 0);
    }
}

template <int BMODE, bool SK>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) gemm_x3w_kernel(const GemmArgs args) {
  wgrad_body<BMODE, SK, 3>(args);
}

template <int BMODE, bool SK>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) gemm_w16_kernel(const GemmArgs args) {
  wgrad_body<BMODE, SK, 1>(args);
}

}  // namespace

int gemm_x3w_launch(const GemmArgs& a, int bmode, int blocks, hipStream_t s, int terms) {
  const dim3 g(blocks), b(WNT);
  const bool sk = a.kchunk[0] * WBK < a.p[0].K;  // k split over several workgroups: partial slabs
  if (terms == 1) {
    if (bmode == 2) {
      if (sk)
        CAPMI_KLAUNCH((gemm_w16_kernel<2, true>), g, b, 0, s, a);
      else
        CAPMI_KLAUNCH((gemm_w16_kernel<2, false>), g, b, 0, s, a);
    } else {
      if (sk)
        CAPMI_KLAUNCH((gemm_w16_kernel<1, true>), g, b, 0, s, a);
      else
        CAPMI_KLAUNCH((gemm_w16_kernel<1, false>), g, b, 0, s, a);
    }
  } else if (bmode == 2) {
    if (sk)
      CAPMI_KLAUNCH((gemm_x3w_kernel<2, true>), g, b, 0, s, a);
    else
      CAPMI_KLAUNCH((gemm_x3w_kernel<2, false>), g, b, 0, s, a);
  } else {
    if (sk)
      CAPMI_KLAUNCH((gemm_x3w_kernel<1, true>), g, b, 0, s, a);
    else
      CAPMI_KLAUNCH((gemm_x3w_kernel<1, false>), g, b, 0, s, a);
  }
  CAPMI_LAUNCH_CHECK();
  return 0;
}
