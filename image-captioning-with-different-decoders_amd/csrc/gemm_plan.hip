// Host launch planner of every GEMM family (no kernel in this file).
//
// A plan_* function per family validates one call and fills a GemmLaunch: the kernel arguments, the tile, the
// workgroup size, the stream-K decision and what attaching the stream-K workspace needs. capmi_gemm_sk_plan reports
// that record, capmi_gemm_sk_ex launches it (launch()), both through plan_flags(); capmi_gemm / capmi_gemm_ex and
// the x3s passes use the same pieces. The kernels and their launchers are in gemm.hip (generic v1), gemm_nt.hip
// (v2: fp32, bf16, three-term staging), gemm_bf16.hip, gemm_x3.hip, gemm_x3p.hip (x3p, x3d), gemm_x3s.hip,
// gemm_x3w.hip and gemm_x3c.hip (declared in gemm_args.h).
#include <cstdlib>

#include "common.h"

#include "gemm_args.h"

#define CAPMI_TRY(expr)                    \
  do {                                     \
    if (const int e__ = (expr)) return e__; \
  } while (0)

namespace {
// ------------------------------------------------------------------------------------
// knobs: every CAPMI_* variable the planner reads, each read once per process
// ------------------------------------------------------------------------------------
const char* knob_text(const char* name) { return getenv(name); }
int knob_int(const char* name, int unset) {
  const char* e = knob_text(name);
  return e ? atoi(e) : unset;
}
bool knob_is(const char* name, char c) {  // the value is exactly the one character c
  const char* e = knob_text(name);
  return e && e[0] == c && e[1] == 0;
}
bool knob_starts(const char* name, char c) {  // the value begins with c
  const char* e = knob_text(name);
  return e && e[0] == c;
}

struct Knobs {
  // CUs the stream-K grids are sized for, default (and for any value outside 1 .. CUs - 1) all of them (A/B
  // measurement: fewer persistent workers than CUs leave CUs free for the concurrently running decoder stream)
  int sk_cus = knob_int("CAPMI_SK_CUS", 0);
  // XCD-grouped stream-K (gemm_nt.hip), default on; "1" turns it off (A/B)
  bool sk_xcd_groups = !knob_is("CAPMI_SK_GROUPS", '1');
  // hybrid data-parallel + stream-K schedule (gemm_nt.hip), default on; "0" turns it off (A/B)
  bool sk_hybrid = !knob_is("CAPMI_SK_HYBRID", '0');
  // "1": data-parallel grids everywhere, default off (A/B measurement: a persistent stream-K grid holds every CU
  // until it ends, a data-parallel one frees CUs as its tiles retire)
  bool sk_off = knob_is("CAPMI_SK_OFF", '1');
  // bit mask of the x3 kernel families launched data-parallel instead of stream-K (1 gemm_x3, 2 x3p, 4 x3d),
  // default 1 (round 3): in the pipelined step, where the decoder stream holds CUs a stream-K worker may wait on,
  // gemm_x3 measured faster data-parallel (headline 5987-5995 -> 6035-6048, fine-tune 1775 -> 1795 img/s, one box;
  // small grids excepted, plan_x3); x3p (-10 %) and x3d (-7 %) keep stream-K
  int sk_family_off = knob_int("CAPMI_SK_FAMILY_OFF", 1);
  // the three-term conv weight gradients keep the fp32 wgrad tile rule (128x128 / 128x64, one workgroup per CU),
  // default on: fine-tune config 1633 -> 1647 img/s against 64x64 (fewer re-reads of dY and the im2col rows);
  // "0": 64x64 (A/B)
  bool x3_wgrad_wide = !knob_is("CAPMI_X3_WGRAD_WIDE", '0');
  // the encoder-sized three-term GEMMs that keep the fp32 tile rule instead of 64x64 (bit mask, default 0, A/B):
  // 1 the 1x1 weight gradients (k rows, K >= 8192 output pixels), 2 the 1x1 data gradients (M >= 8192 output
  // pixels). The decoder's GEMMs stay below both bounds.
  int x3_keep_tile = knob_int("CAPMI_X3_KEEP_TILE", 0);
  // a leading '0': the general epilogue everywhere instead of the store-only one, default off (A/B arm)
  bool x3_plain_epi = !knob_starts("CAPMI_X3_PLAIN_EPI", '0');
  // a leading '3' (32) forces x3p's one-workgroup-per-CU form, default off (A/B)
  bool x3p_force32 = knob_starts("CAPMI_X3P_BK", '3');
  // a leading 'c' (col): x3p walks its tiles column-major (an XCD's contiguous range shares B), default row-major
  bool x3p_cols_first = knob_starts("CAPMI_X3P_ORDER", 'c');
  // x3d's two-deep A pipeline: 0 / 1 off / on everywhere, default (negative) plan_x3d's per-launch rule
  int x3d_pipe = knob_int("CAPMI_X3D_PIPE", -1);
  // a leading '1': x3d keeps stream-K for C = A.B + beta C, default off (A/B)
  bool x3d_beta_sk = knob_starts("CAPMI_X3D_BETA_SK", '1');
  // bf16-IO: the largest K of the one-stage short-k form, default 256 (A/B)
  int bf16_st1_k = knob_int("CAPMI_BF16_ST1_K", 256);
  // bf16-IO: a leading '1' lets the bf16 convs run stream-K, default off (round 3: data-parallel grids measured
  // faster in the pipelined bf16 step, config 5)
  bool bf16_sk = knob_starts("CAPMI_BF16_SK", '1');
  // bf16-IO: 2 / 4 forces one depth of the LDS-DMA ring, default (any other value) plan_bf16_io's rule (A/B)
  int bf16_stages = knob_int("CAPMI_BF16_STAGES", 0);
};
const Knobs& knobs() {
  static const Knobs k;
  return k;
}

// ------------------------------------------------------------------------------------
// the device as the planner sees it
// ------------------------------------------------------------------------------------
int cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cache[dev] = n;
  }
  return cache[dev];
}

int sk_cus() {
  static const int n = [] {
    const int v = knobs().sk_cus;
    return v > 0 && v < cu_count() ? v : cu_count();
  }();
  return n;
}

constexpr int kSkMaxWgPerCu = 4;
long long sk_flag_bytes(int cus) { return ((long long)(cus * kSkMaxWgPerCu + 1) * 4 + 255) / 256 * 256; }

// resident workgroups per CU of the NT kernel for a tile shape (LDS / register bound)
// (terms 3: three bf16 LDS planes per operand, 60 KB for 64x64 and >= 90 KB for the larger tiles)
int gemm_nt_wg_per_cu(int bm, int bn, int terms) {
  if (terms == 3) return bm == 64 && bn == 64 ? 2 : 1;
  return bm == 64 && bn == 64 ? 4 : 2;
}

// ------------------------------------------------------------------------------------
// the plan record
// ------------------------------------------------------------------------------------
enum Family { FAM_NT, FAM_BF16_IO, FAM_X3, FAM_X3P, FAM_X3D, FAM_X3S, FAM_X3C, FAM_X3W };

struct GemmLaunch {
  GemmArgs a;
  Family family;
  int amode, bmode;
  int bm, bn, threads;
  bool sk;          // stream-K decided (x3w: a k-split, S > 1)
  long long total;  // workgroups of the data-parallel launch (x3w: output tiles, each run by `extra` workgroups)
  // what sk_attach takes: resident workgroups, k-tiles per output tile, the hybrid schedule
  long long slots;
  int nkt;
  bool hybrid;
  // what capmi_gemm_sk_plan reports as `generic` and the family's launcher takes: v2 / v1 0 / 1 (the generic
  // kernel), bf16-IO the LDS stages, x3p the k-tile depth, x3d 32, x3w the k-splits S, x3s the persistent grid,
  // x3c the tiles
  int extra;
  int terms;      // v2 operand staging (0 fp32, 1 bf16, 3 three-term split); x3w 3 / 1
  bool nt_ok;     // v2 kernel eligible (else the generic one), and its float4 loads
  bool vec;
  long long lda;  // x3s: floats per A row
};

// ------------------------------------------------------------------------------------
// pieces every family shares
// ------------------------------------------------------------------------------------
// tiles / (rounds x slots): how full the rounds of a data-parallel grid on `slots` resident workgroups are
double grid_fill(long long total, long long slots) {
  const long long rounds = (total + slots - 1) / slots;
  return (double)total / (double)(rounds * slots);
}
// the grid would leave a costly partial last round: the stream-K condition of every family
bool underfilled(long long total, long long slots) { return grid_fill(total, slots) < 0.9; }

// Does problem p take the store-only epilogue of the x3 kernels with bn-wide column tiles? 0: no; 1: C = A.B;
// 2: C = A.B + beta C (read-modify-write through the same offsets; the fine-tune 1x1 data gradients accumulate
// into the block input's gradient). No alpha / bias / relu / row remap; whole column tiles; C addressable with
// 32-bit byte offsets; rows past M read zeros in A, so their accumulators add nothing to the BN sums.
int store_only(const capmi_gemm_problem& p, int bn) {
  const bool ok = p.alpha == 1.f && p.alpha_ptr == nullptr && p.bias == nullptr && p.bias2 == nullptr &&
                  !p.relu && p.c_r1 <= 0 && p.ksplit == 1 && p.N % bn == 0 && p.ldc >= p.N &&
                  (long long)p.M * p.ldc * 4 < (1LL << 31);
  return ok ? (p.beta == 0.f ? 1 : 2) : 0;
}
// the same as a choice (x3 / x3p / x3d / x3w / bf16-IO), subject to CAPMI_X3_PLAIN_EPI; x3s and x3c, whose only
// form it is, require store_only() == 1 whatever the knob says
int plain_epilogue(const capmi_gemm_problem& p, int bn) { return knobs().x3_plain_epi ? store_only(p, bn) : 0; }

// the BN prologue's pointers come as a pair, each 16-byte aligned
bool prologue_paired(const capmi_gemm_problem& p) { return (p.in_scale == nullptr) == (p.in_shift == nullptr); }
bool prologue_aligned(const capmi_gemm_problem& p) {
  return p.in_scale == nullptr || (aligned16(p.in_scale) && aligned16(p.in_shift));
}

// conv geometry, A the NHWC input: one row per output pixel, k = (kh, kw, ci)
bool conv_a_shape(const capmi_gemm_problem& p) {
  return p.K == p.cKH * p.cKW * p.cCin && p.M == p.cN * p.cHo * p.cWo;
}
// conv geometry, B the NHWC input of a weight gradient: k = output pixel, n = (kh, kw, ci) (implicit im2col)
bool conv_b_shape(const capmi_gemm_problem& p) {
  return p.cCin % 4 == 0 && p.N == p.cKH * p.cKW * p.cCin && p.K == p.cN * p.cHo * p.cWo;
}
bool fits31(long long bytes) { return bytes < (1LL << 31); }
long long conv_input_elems(const capmi_gemm_problem& p) { return (long long)p.cN * p.cH * p.cW * p.cCin; }

// operand A of the x3 / x3p / x3d / bf16-IO families, addressed with 32-bit byte offsets at `ebytes` bytes per
// element (all planes): the NHWC conv input with channels in whole k-tiles of cin_mult, or dense rows of lda
int require_a(const capmi_gemm_problem& p, int amode, int cin_mult, int lda_mult, int ebytes) {
  if (amode == CAPMI_A_CONV_NHWC) {
    CAPMI_REQUIRE(p.cCin % cin_mult == 0 && conv_a_shape(p), CAPMI_EINVAL);
    CAPMI_REQUIRE(fits31(conv_input_elems(p) * ebytes), CAPMI_ERANGE);
  } else {
    CAPMI_REQUIRE(p.lda % lda_mult == 0 && p.lda >= p.K, CAPMI_EALIGN);
    CAPMI_REQUIRE(fits31((long long)p.M * p.lda * ebytes), CAPMI_ERANGE);
  }
  return 0;
}
// operand B = W[N][K] of the same families as bf16 planes of rows of ldb: 16-byte row chunks, 32-bit offsets
bool b_planes_aligned(const capmi_gemm_problem& p) {
  return aligned16(p.A) && aligned16(p.B) && p.ldb % 8 == 0 && p.ldb >= p.K;
}
bool b_planes_fit(const capmi_gemm_problem& p, int planes) { return fits31((long long)planes * p.N * p.ldb * 2); }
// the modes of those families: B = W[N][K], A dense rows or the NHWC conv input
bool forward_modes(int amode, int bmode) {
  return bmode == CAPMI_B_NMAJOR_W && (amode == CAPMI_A_KMAJOR || amode == CAPMI_A_CONV_NHWC);
}

// the single-problem launch of bm x bn tiles, one workgroup per tile
void fill_one(GemmLaunch& L, Family family, const capmi_gemm_problem& p, int amode, int bmode, int bm, int bn,
              int threads) {
  GemmArgs& a = L.a;
  memset(&a, 0, sizeof(a));
  a.nprob = 1;
  a.p[0] = p;
  a.tiles_m[0] = (int)cdiv(p.M, bm);
  a.tiles_n[0] = (int)cdiv(p.N, bn);
  a.plain_epi = plain_epilogue(p, bn);
  L.total = (long long)a.tiles_m[0] * a.tiles_n[0];
  a.tiles_begin[1] = (int)L.total;
  L.family = family;
  L.amode = amode;
  L.bmode = bmode;
  L.bm = bm;
  L.bn = bn;
  L.threads = threads;
  L.sk = false;
  L.slots = 0;
  L.nkt = 0;
  L.hybrid = false;
  L.extra = 0;
  L.terms = 0;
  L.nt_ok = L.vec = false;
  L.lda = 0;
}

// Attach the stream-K workspace (the flags, then one parked-partial slot per worker) to a launch of `total` output
// tiles of `nkt` k-tiles each on `slots` resident workgroups. hybrid: with more than two rounds of tiles, all but the
// last 1-2 rounds' worth run whole before the stream-K part. What a null workspace means is the caller's rule.
int sk_attach(GemmArgs& a, long long total, int nkt, long long slots, bool hybrid, void* workspace,
              long long ws_bytes) {
  CAPMI_REQUIRE(aligned16(workspace), CAPMI_EINVAL);
  CAPMI_REQUIRE(ws_bytes >= capmi_gemm_workspace_bytes(), CAPMI_ERANGE);
  a.sk_nkt = nkt;
  a.sk_dp_tiles = hybrid && knobs().sk_hybrid && total >= 2 * slots ? (int)((total / slots - 1) * slots) : 0;
  a.sk_units = (total - a.sk_dp_tiles) * a.sk_nkt;
  a.sk_workers = (int)std::min<long long>(slots, a.sk_units);
  a.sk_groups = knobs().sk_xcd_groups && a.sk_workers % 8 == 0 && total >= 64 ? 8 : 1;
  a.sk_flags = static_cast<int*>(workspace);
  a.sk_part = reinterpret_cast<float*>(static_cast<char*>(workspace) + sk_flag_bytes(cu_count()));
  return 0;
}

// ------------------------------------------------------------------------------------
// v1 / v2 (gemm.hip, gemm_nt.hip): fp32, bf16 and three-term staged operands
// ------------------------------------------------------------------------------------
long long tiles_of(const capmi_gemm_problem* probs, int nprob, int bm, int bn) {
  long long t = 0;
  for (int i = 0; i < nprob; ++i)
    t += (long long)((probs[i].M + bm - 1) / bm) * ((probs[i].N + bn - 1) / bn) * probs[i].ksplit;
  return t;
}

// the grouped data-parallel launch of capmi_gemm / capmi_gemm_ex (and what plan_nt_staged starts from)
int plan_nt_group(const capmi_gemm_problem* probs, int nprob, int amode, int bmode, int tile, GemmLaunch& g) {
  CAPMI_REQUIRE(probs != nullptr && nprob >= 1 && nprob <= CAPMI_MAX_GROUP, CAPMI_EINVAL);
  CAPMI_REQUIRE(amode >= 0 && amode <= 4 && bmode >= 0 && bmode <= 2, CAPMI_EINVAL);
  CAPMI_REQUIRE(bmode != 2 || amode == 1, CAPMI_EINVAL);
  CAPMI_REQUIRE(tile >= CAPMI_TILE_128 && tile <= CAPMI_TILE_128_W8, CAPMI_EINVAL);
  CAPMI_REQUIRE(amode != 4 || bmode == 0, CAPMI_EINVAL);
  GemmArgs& a = g.a;
  memset(&a, 0, sizeof(a));
  a.nprob = nprob;
  bool vec = true;
  // v2 kernel eligible: row-major A (dense / conv) with B = W[N][K], or the transposed-staging
  // forms (A stored as k rows and/or B stored as k rows) of the backward GEMMs
  bool nt_ok = ((amode == 0 || amode == 2 || amode == 4) && bmode == 0) || ((amode == 0 || amode == 1) && bmode == 1) ||
               (amode == 1 && bmode == 2);
  for (int i = 0; i < nprob; ++i) {
    const capmi_gemm_problem& p = probs[i];
    CAPMI_REQUIRE(p.M >= 0 && p.N >= 0 && p.K >= 0 && p.ksplit >= 1, CAPMI_EINVAL);
    CAPMI_REQUIRE(p.A && p.B && p.C, CAPMI_EINVAL);
    CAPMI_REQUIRE(p.ksplit == 1 || p.c_split_stride > 0, CAPMI_EINVAL);
    CAPMI_REQUIRE(p.stats == nullptr || p.ksplit == 1, CAPMI_EINVAL);
    if (amode == 2) {
      CAPMI_REQUIRE(p.cCin % kGemmV1BK == 0 && p.cCin % 4 == 0, CAPMI_EALIGN);
      CAPMI_REQUIRE(conv_a_shape(p), CAPMI_EINVAL);
      CAPMI_REQUIRE(aligned16(p.A), CAPMI_EALIGN);
      CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
      CAPMI_REQUIRE(aligned16(p.B) && p.ldb % 4 == 0, CAPMI_EALIGN);
      nt_ok = nt_ok && p.cCin % 32 == 0;
    }
    if (amode == 4) {
      CAPMI_REQUIRE(p.cCin == 4 && conv_a_shape(p), CAPMI_EINVAL);
      CAPMI_REQUIRE(aligned16(p.A) && aligned16(p.B) && p.ldb % 4 == 0 && p.in_scale == nullptr,
                    CAPMI_EALIGN);
    }
    if (bmode == 2) {
      CAPMI_REQUIRE(conv_b_shape(p), CAPMI_EINVAL);
      CAPMI_REQUIRE(p.K < (1 << 24), CAPMI_ERANGE);
      CAPMI_REQUIRE(aligned16(p.B), CAPMI_EALIGN);
      CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
    }
    if (amode == 3) {
      CAPMI_REQUIRE(conv_a_shape(p), CAPMI_EINVAL);
    }
    if (amode == 0) {
      vec = vec && aligned16(p.A) && p.lda % 4 == 0 && p.K % 4 == 0 && (p.a_r1 <= 0 || p.a_s2 % 4 == 0);
    } else if (amode == 1) {
      vec = vec && aligned16(p.A) && p.lda % 4 == 0 && p.M % 4 == 0 && (p.a_r1 <= 0 || p.a_s2 % 4 == 0);
    }
    if (bmode == 0)
      vec = vec && aligned16(p.B) && p.ldb % 4 == 0 && p.K % 4 == 0;
    else if (bmode == 2)
      vec = vec && p.N % 4 == 0;
    else
      vec = vec && aligned16(p.B) && p.ldb % 4 == 0 && p.N % 4 == 0;
    a.p[i] = p;
  }
  nt_ok = nt_ok && (vec || ((amode == 2 || amode == 4) && bmode == 0));
  CAPMI_REQUIRE(bmode != 2 || nt_ok, CAPMI_EALIGN);  // no generic-kernel form of the im2col B
  int bm = 128, bn = 128;
  g.threads = 256;
  if (tile == CAPMI_TILE_128_W8) {  // 512-thread 128x128 form: forward modes of the v2 kernel only
    CAPMI_REQUIRE(nt_ok && bmode == 0 && (amode == 0 || amode == 2 || amode == 4), CAPMI_EINVAL);
    g.threads = 512;
    tile = CAPMI_TILE_128;
  }
  if (tile == CAPMI_TILE_64) {
    bm = bn = 64;
  } else if (tile == CAPMI_TILE_128x64) {
    bn = 64;
  } else if (tile == CAPMI_TILE_AUTO) {
    if (!nt_ok) {
      bm = bn = (tiles_of(probs, nprob, 128, 128) >= 256 ? 128 : 64);
    } else {
      // measured on the ResNet-101 / decoder shapes (tools/gemm_sweep.py): the 64x64 tile
      // (4 WGs per CU) is the fastest or within noise of it on every one of them
      bm = bn = 64;
    }
  }
  if (!nt_ok && bm != bn) bn = bm = 128;
  const int bk = nt_ok ? 32 : kGemmV1BK;
  long long total = 0;
  for (int i = 0; i < nprob; ++i) {
    const capmi_gemm_problem& p = probs[i];
    a.tiles_m[i] = (p.M + bm - 1) / bm;
    a.tiles_n[i] = (p.N + bn - 1) / bn;
    int kc = (p.K + p.ksplit - 1) / p.ksplit;
    kc = ((kc + bk - 1) / bk) * bk;
    a.kchunk[i] = kc > 0 ? kc : bk;
    a.tiles_begin[i] = (int)total;
    total += (long long)a.tiles_m[i] * a.tiles_n[i] * p.ksplit;
  }
  a.tiles_begin[nprob] = (int)total;
  CAPMI_REQUIRE(total < (1LL << 31), CAPMI_ERANGE);
  g.family = FAM_NT;
  g.amode = amode;
  g.bmode = bmode;
  g.bm = bm;
  g.bn = bn;
  g.nt_ok = nt_ok;
  g.vec = vec;
  g.total = total;
  g.sk = false;
  g.slots = 0;
  g.nkt = 0;
  g.hybrid = true;
  g.extra = nt_ok ? 0 : 1;
  g.terms = 0;
  g.lda = 0;
  return 0;
}

// operand staging of the v2 kernel: 0 fp32, 1 bf16 (CAPMI_GEMM_BF16), 3 three-term split
// (CAPMI_GEMM_SPLIT3); -1 for any other flag combination
int flag_terms(int flags) {
  if (flags == 0) return 0;
  if (flags == CAPMI_GEMM_BF16) return 1;
  if (flags == CAPMI_GEMM_SPLIT3) return 3;
  return -1;
}
// the modes a split-staged (terms > 0) launch supports (gemm_nt.hip: gemm_nt_launch)
bool terms_mode_ok(int terms, int amode, int bmode) {
  if (terms == 0) return true;
  if (bmode == 0 && (amode == 2 || amode == 4)) return true;  // convs
  if (bmode == 2) return terms == 3 && amode == 1;             // conv weight gradients (three-term split)
  if (terms == 1 && bmode == 0) return amode == 0;
  return (amode == 0 && bmode <= 1) || (amode == 1 && bmode == 1);
}

// the single-problem launch of capmi_gemm_sk_ex with `terms`-staged operands: tile, 512-thread form, stream-K
int plan_nt_staged(const capmi_gemm_problem* prob, int amode, int bmode, int tile, int terms, GemmLaunch& g) {
  const bool bf16 = terms > 0;
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const int nkt = (prob->K + 31) / 32;
  const bool automatic = tile == CAPMI_TILE_AUTO;
  // measured (tools/gemm_sweep.py, ResNet-101 shapes at batch 64): with >= 16 k-tiles per
  // output tile, stream-K over 128x64 tiles is the fastest form; below that the per-segment
  // pipeline fill outweighs the balance gain and 64x64 data-parallel wins
  if (automatic) tile = nkt >= 16 ? CAPMI_TILE_128x64 : CAPMI_TILE_64;
  // conv weight gradients (k = output pixels, always >= 16 k-tiles; tools/wgrad_tile_ab.py, with
  // the k-major LDS images): 128x128 for the wide 3x3 ones (Cout >= 256, N = 9*Cin >= 2048:
  // layer3/4, 1-7 % faster than 128x64), 128x64 for the rest (layer2 3x3 and the 1x1 ones: 128x128
  // is up to 2x slower there, 64x64 5-12 % slower)
  if (automatic && amode == CAPMI_A_MMAJOR && bmode == CAPMI_B_CONV_NHWC)
    tile = (prob->M >= 256 && prob->N >= 2048) ? CAPMI_TILE_128 : CAPMI_TILE_128x64;
  // three-term split staging: 64x64 everywhere (two workgroups per CU; the larger tiles hold one:
  // tools/dec_gemm_ab.py --tile, 5-20 % faster on every decoder GEMM at 64x64)
  const Knobs& kn = knobs();
  const bool keep = (bmode == CAPMI_B_CONV_NHWC && kn.x3_wgrad_wide) ||
                    ((kn.x3_keep_tile & 1) && amode == CAPMI_A_MMAJOR && bmode == CAPMI_B_KROWS && prob->K >= 8192) ||
                    ((kn.x3_keep_tile & 2) && amode == CAPMI_A_KMAJOR && bmode == CAPMI_B_NMAJOR_W && prob->M >= 8192);
  if (automatic && terms == 3 && !keep) tile = CAPMI_TILE_64;
  CAPMI_TRY(plan_nt_group(prob, 1, amode, bmode, tile, g));
  // the 512-thread 128x128 form (tools/w8_ab.sh over all 19 encoder conv shapes, batch 64):
  // 2-12% faster wherever N >= 128 and either the k-loop is long (>= 16 k-tiles) or N <= 256;
  // slower for N = 64 (half the tile idle) and for N >= 512 with a short k-loop (64x64 keeps
  // 4 workgroups per CU to hide the epilogue)
  if (automatic && g.nt_ok && !bf16 && bmode == 0 && (amode == 0 || amode == 2 || amode == 4) &&
      prob->ksplit == 1 && prob->M >= 2048 && prob->N >= 128 && (nkt >= 16 || prob->N <= 256))
    CAPMI_TRY(plan_nt_group(prob, 1, amode, bmode, CAPMI_TILE_128_W8, g));
  g.terms = terms;
  g.nkt = nkt;
  g.slots = (long long)sk_cus() * (g.threads == 512 ? 1 : gemm_nt_wg_per_cu(g.bm, g.bn, terms));
  // short k-loops (< 16 k-tiles) stay data-parallel even in the hybrid form: splitting the last
  // rounds' tiles there cost 6-10 % on the layer1-3 1x1 shapes (tools/hybrid_ab.sh);
  // stream-K only when the data-parallel grid would leave a costly partial last round
  g.sk = g.nt_ok && prob->ksplit == 1 && g.total > 0 && (!automatic || nkt >= 16) && underfilled(g.total, g.slots) &&
         !kn.sk_off;
  return 0;
}

// flags 0 / CAPMI_GEMM_BF16 / CAPMI_GEMM_SPLIT3 of capmi_gemm_sk_ex
int plan_nt(const capmi_gemm_problem* prob, int amode, int bmode, int tile, int terms, GemmLaunch& g) {
  CAPMI_REQUIRE(terms >= 0 && terms_mode_ok(terms, amode, bmode), CAPMI_EINVAL);
  CAPMI_TRY(plan_nt_staged(prob, amode, bmode, tile, terms, g));
  // shapes the split forms do not cover (unaligned / generic-kernel problems, the 512-thread form, a prologue on
  // dense rows): the fp32 kernel, planned again as such
  if (terms > 0 && !(g.nt_ok && g.threads == 256 &&
                     (prob->in_scale == nullptr || amode == CAPMI_A_CONV_NHWC || bmode == CAPMI_B_CONV_NHWC)))
    CAPMI_TRY(plan_nt_staged(prob, amode, bmode, tile, 0, g));
  return 0;
}

// ------------------------------------------------------------------------------------
// CAPMI_GEMM_BF16_IO: bf16 A / B / C (gemm_bf16.hip), plain conv / dense GEMM with BN statistics; BM = 128.
// The plan query (operands = false) answers for any K % 64 == 0 problem; the launcher validates the operands.
// have_ws: stream-K only with a workspace, and stream-K changes the stages.
// ------------------------------------------------------------------------------------
int plan_bf16_io(const capmi_gemm_problem* prob, int amode, int bmode, int tile, bool operands, bool have_ws,
                 GemmLaunch& L) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(forward_modes(amode, bmode), CAPMI_EINVAL);
  if (operands) {
    CAPMI_REQUIRE(p.A && p.B && p.C && p.M >= 0 && p.N > 0 && p.K > 0 && p.K % 64 == 0, CAPMI_EINVAL);
    CAPMI_REQUIRE(p.ksplit == 1 && !p.bias && !p.bias2 && !p.alpha_ptr && p.alpha == 1.f && p.beta == 0.f &&
                      !p.relu && p.a_r1 <= 0 && p.c_r1 <= 0,
                  CAPMI_EINVAL);
    // no prologue: the bf16 conv input is materialised once per tensor (capmi_bn_relu_bf16)
    CAPMI_REQUIRE(p.in_scale == nullptr && p.in_shift == nullptr, CAPMI_EINVAL);
    CAPMI_REQUIRE(b_planes_aligned(p) && p.ldc >= p.N, CAPMI_EALIGN);
    CAPMI_REQUIRE(b_planes_fit(p, 1), CAPMI_ERANGE);
    CAPMI_TRY(require_a(p, amode, 64, 8, 2));
  } else {
    CAPMI_REQUIRE(p.K > 0 && p.K % 64 == 0, CAPMI_EINVAL);
  }
  const Knobs& kn = knobs();
  // AUTO on a short k (K <= 256: the bf16 config's 1x1 c3 convs, layer1's K = 64 convs and downsample, the c1 of
  // layer1): 128x64 tiles, one LDS stage, four workgroups per CU, data-parallel (round 5: l3 c3 20.0 -> 17.1 us, l2 c3
  // 24.7 -> 18.4, l1 c3 33.3 -> 24.3; at K = 512 a tie and above it slower). Round 6: alone, the K = 256 convs on 128+
  // columns run faster on the DMA ring below (l3 c3 17.3 -> 16.0 us, ds2 29.3 -> 28.1), but in the pipelined config-5
  // step the one-stage form stays ahead (13330 -> 13365 img/s, three interleaved rounds, same box); CAPMI_BF16_ST1_K = k
  // moves the bound (A/B)
  const bool st1 = tile == CAPMI_TILE_AUTO && p.K <= kn.bf16_st1_k;
  // AUTO on a grid of 128x128 tiles that fills at most half the CUs (layer4's 3136-row convs: 100 tiles):
  // 128x64 tiles, twice the workgroups (round 5: l4 3x3 53.2 -> 40.8 us, l4 c1 25.8 -> 18.9; the 400-tile
  // layer4 c3 / downsample and layer3's 196-tile grids stay at 128x128, where 128x64 measured slower)
  const bool narrow = tile == CAPMI_TILE_AUTO && 2 * cdiv(p.M, 128) * cdiv(p.N, 128) <= cu_count();
  const int bn =
      (st1 || narrow || tile == CAPMI_TILE_128x64 || tile == CAPMI_TILE_64 || (tile == CAPMI_TILE_AUTO && p.N <= 64))
          ? 64 : 128;
  fill_one(L, FAM_BF16_IO, p, amode, bmode, 128, bn, 256);  // (bf16 C: the fp32 bound on M * ldc is the stricter one)
  if (p.ldc % 8 != 0 || !aligned16(p.C)) L.a.plain_epi = 0;  // (its 16-B row-chunk stores)
  L.slots = (long long)sk_cus() * 2;
  L.nkt = p.K / 64;
  // (round 3) stream-K for the bf16 convs only on CAPMI_BF16_SK=1: data-parallel grids measured faster in the
  // pipelined bf16 step (config 5)
  L.sk = !st1 && kn.bf16_sk && !kn.sk_off && have_ws && p.K / 64 >= 4 && underfilled(L.total, L.slots);
  // (round 6) data-parallel: the LDS-DMA ring (gemm_bf16.hip), four k-tiles deep at one workgroup per CU when the grid
  // is one round of tiles (layer3's 196-tile and layer4's 200-tile grids: l3 3x3 28.7 -> 23.4 us, l3 c1 15.8 -> 12.5,
  // l4 c1 17.5 -> 14.7), else two deep at two workgroups per CU (l2 3x3 25.3 -> 21.4, l1 3x3 35.6 -> 31.4, ds3 27.4 ->
  // 23.3, l4 c3 15.2 -> 13.1); CAPMI_BF16_STAGES = 2 / 4 forces one depth (A/B)
  const int forced = kn.bf16_stages == 2 || kn.bf16_stages == 4 ? kn.bf16_stages : 0;
  L.extra = st1 ? 1 : L.sk ? 2 : forced ? forced : L.total <= cu_count() ? 4 : 2;
  L.threads = bf16_threads(bn, L.extra, L.sk);
  return 0;
}

// ------------------------------------------------------------------------------------
// the x3 families: fp32-accurate three-term bf16 products
// ------------------------------------------------------------------------------------
bool sk_family_off(int bit) { return (knobs().sk_family_off & bit) != 0; }

// what x3 / x3p / x3d require alike of a call
int require_x3(const capmi_gemm_problem* prob, int amode, int bmode) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(forward_modes(amode, bmode), CAPMI_EINVAL);
  CAPMI_REQUIRE(p.A && p.B && p.C && p.M >= 0 && p.N > 0 && p.K > 0 && p.K % 32 == 0 && p.ksplit == 1, CAPMI_EINVAL);
  return 0;
}
// their stream-K rule: one workgroup per CU, k-tiles of 32, hybrid schedule
void x3_stream_k(GemmLaunch& L, int family_bit, bool small_grid_exempt) {
  L.slots = sk_cus();
  L.nkt = L.a.p[0].K / 32;
  L.hybrid = true;
  L.sk = !knobs().sk_off && (!sk_family_off(family_bit) || (small_grid_exempt && L.total * 4 < L.slots)) &&
         L.total > 0 && L.nkt >= 8 && underfilled(L.total, L.slots);
}

// CAPMI_GEMM_X3: fp32 A x three-plane bf16 B (gemm_x3.hip), one 512-thread workgroup per CU
int plan_x3(const capmi_gemm_problem* prob, int amode, int bmode, int tile, GemmLaunch& L) {
  CAPMI_TRY(require_x3(prob, amode, bmode));
  const capmi_gemm_problem& p = *prob;
  // the prologue is the conv input's BN-apply + ReLU: dense A takes none
  CAPMI_REQUIRE(amode == CAPMI_A_CONV_NHWC || (!p.in_scale && !p.in_shift), CAPMI_EINVAL);
  CAPMI_REQUIRE(prologue_paired(p), CAPMI_EINVAL);
  CAPMI_REQUIRE(p.stats == nullptr || p.c_r1 <= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(b_planes_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(b_planes_fit(p, 3), CAPMI_ERANGE);
  CAPMI_REQUIRE(amode == CAPMI_A_CONV_NHWC || p.a_r1 <= 0, CAPMI_EALIGN);
  CAPMI_TRY(require_a(p, amode, 32, 4, 4));
  const int bn = (tile == CAPMI_TILE_128x64 || tile == CAPMI_TILE_64 || (tile == CAPMI_TILE_AUTO && p.N <= 64)) ? 64 : 128;
  fill_one(L, FAM_X3, p, amode, bmode, 128, bn, 512);
  // (round 3) more than two rounds of tiles: data-parallel -- the hardware's dynamic dispatch beat the hybrid
  // schedule there (layer1 c1: 55 vs 69 us, layer1 3x3: 154 vs 156; CAPMI_SK_OFF A/B on one box)
  // with the family data-parallel (the default), grids under a quarter of the CUs keep stream-K: a few long-k
  // tiles would otherwise run on a few CUs and accumulate the whole k serially (conv grids are >= 100 tiles)
  x3_stream_k(L, 1, true);
  L.sk = L.sk && (L.total + L.slots - 1) / L.slots <= 2;
  return 0;
}

// CAPMI_GEMM_X3P: three-plane A and B (gemm_x3p.hip), 256x128 tiles, 1-2 workgroups per CU
// Two forms: BK = 16 with two workgroups per CU (their DMA waits and barriers interleave) as a
// plain data-parallel grid when there are at least 2 x CUs tiles and they fill >= 70 % of the last
// round; otherwise BK = 32, one workgroup per CU, stream-K when the tile count leaves the chip
// under-filled (l3 c3, 392 tiles: 49 us stream-K vs 102 us as one 2-per-CU round).
int plan_x3p(const capmi_gemm_problem* prob, int amode, int bmode, GemmLaunch& L) {
  CAPMI_TRY(require_x3(prob, amode, bmode));
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(!p.in_scale && !p.in_shift && p.a_r1 <= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(p.stats == nullptr || p.c_r1 <= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(b_planes_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(b_planes_fit(p, 3), CAPMI_ERANGE);
  CAPMI_TRY(require_a(p, amode, 32, 8, 6));  // three bf16 planes
  fill_one(L, FAM_X3P, p, amode, bmode, 256, 128, 512);
  L.a.tile_cols_first = knobs().x3p_cols_first ? 1 : 0;
  const long long slots2 = 2LL * sk_cus();
  if (!knobs().x3p_force32 && L.total >= slots2 && grid_fill(L.total, slots2) >= 0.7) {
    L.extra = 16;
    return 0;
  }
  L.extra = 32;
  x3_stream_k(L, 2, false);
  return 0;
}

// CAPMI_GEMM_X3D: fp32 A (+ BN prologue for convs) split in-kernel x three-plane B in the x3p k order
// (gemm_x3p.hip, ASPLIT): 256x128 tiles, 512 threads, k-tiles of 32, one workgroup per CU, stream-K
// when the tiles under-fill the chip
int plan_x3d(const capmi_gemm_problem* prob, int amode, int bmode, GemmLaunch& L) {
  CAPMI_TRY(require_x3(prob, amode, bmode));
  const capmi_gemm_problem& p = *prob;
  // dense rows take the prologue when k is the channel (a 1x1 conv's input: lda == K)
  CAPMI_REQUIRE(amode == CAPMI_A_CONV_NHWC || (!p.in_scale && !p.in_shift) || p.lda == p.K, CAPMI_EINVAL);
  CAPMI_REQUIRE(prologue_paired(p), CAPMI_EINVAL);
  CAPMI_REQUIRE(p.a_r1 <= 0 && (p.stats == nullptr || p.c_r1 <= 0), CAPMI_EINVAL);
  CAPMI_REQUIRE(b_planes_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(b_planes_fit(p, 3), CAPMI_ERANGE);
  CAPMI_TRY(require_a(p, amode, 32, 4, 4));
  fill_one(L, FAM_X3D, p, amode, bmode, 256, 128, 512);
  L.extra = 32;
  // the two-deep A pipeline (round 4, per-conv A/B at batch 64, one box): 4-9 % faster without the BN
  // prologue and on the conv-mode prologue above layer4's 3136 rows; 1-5 % slower on the dense-row prologue
  // (layer2/3 c3) and layer4's 3x3 -- those keep the one-deep loop. CAPMI_X3D_PIPE=0 / 1: off / on everywhere
  const int force = knobs().x3d_pipe;
  const bool pro = p.in_scale != nullptr;
  L.a.x3d_pipe = force >= 0 ? force : (!pro || (amode == CAPMI_A_CONV_NHWC && p.M > 3136)) ? 1 : 0;
  x3_stream_k(L, 4, false);
  // C = A.B + beta C (the fine-tune 1x1 data gradients accumulating into the block input's gradient): the
  // data-parallel form, whose epilogue loads each column block of C ahead of its stores (the stream-K forms sit
  // at the register cap and keep the interleaved load / store); CAPMI_X3D_BETA_SK=1 keeps stream-K (A/B)
  if (L.a.plain_epi == 2 && !knobs().x3d_beta_sk) L.sk = false;
  return 0;
}

// CAPMI_GEMM_X3W (gemm_x3w.hip): conv weight gradient dW = dY^T . im2col(X), both operands fp32 k rows (pixels),
// split in-kernel; 256 x 128 tiles, one workgroup per CU, the k range split S ways so that tiles x S fills the
// CUs once (S partial slabs in the workspace after the stream-K flags, summed by capmi_splitk_reduce's kernel).
// ws_floats: the workspace's capacity for slabs; terms 3 (x3) or 1 (bf16: gemm_w16_kernel, round 6, ABI 26)
int plan_x3w(const capmi_gemm_problem* prob, int amode, int bmode, long long ws_floats, int terms, GemmLaunch& L) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(amode == CAPMI_A_MMAJOR && (bmode == CAPMI_B_KROWS || bmode == CAPMI_B_CONV_NHWC), CAPMI_EINVAL);
  // K = 0 is refused: the kernel would leave C untouched where C = beta C is the contract
  CAPMI_REQUIRE(p.A && p.B && p.C && p.M > 0 && p.N > 0 && p.K > 0 && p.ksplit == 1, CAPMI_EINVAL);
  CAPMI_REQUIRE(!p.bias && !p.bias2 && !p.relu && !p.stats && p.a_r1 <= 0 && p.c_r1 <= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(prologue_paired(p), CAPMI_EINVAL);
  CAPMI_REQUIRE(p.M % 4 == 0 && p.N % 4 == 0 && p.lda >= p.M && p.lda % 4 == 0 && p.ldc >= p.N, CAPMI_EALIGN);
  CAPMI_REQUIRE(aligned16(p.A) && aligned16(p.B), CAPMI_EALIGN);
  CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE(fits31((long long)p.K * p.lda * 4), CAPMI_ERANGE);
  if (bmode == CAPMI_B_CONV_NHWC) {
    CAPMI_REQUIRE(conv_b_shape(p), CAPMI_EINVAL);
    CAPMI_REQUIRE(fits31(conv_input_elems(p) * 4), CAPMI_ERANGE);
    // the kernel advances each pixel walk by a 32-pixel k-tile with at most two wraps of the output row
    CAPMI_REQUIRE(p.cWo > 0 && p.cHo > 0 && 32 / p.cWo + 1 < 2 * p.cHo, CAPMI_ERANGE);
  } else {
    CAPMI_REQUIRE(p.ldb % 4 == 0 && p.ldb >= p.N, CAPMI_EALIGN);
    CAPMI_REQUIRE(fits31((long long)p.K * p.ldb * 4), CAPMI_ERANGE);
  }
  fill_one(L, FAM_X3W, p, amode, bmode, 256, 128, 512);
  L.terms = terms;
  const long long nkt = std::max<long long>(1, (p.K + 31) / 32);
  // k-splits: one round of workgroups over the CUs, at least 4 k-tiles each, slabs within the workspace;
  // a k-split sums in fp32 partials, so the host requires alpha 1 / beta 0 for it (the weight gradients)
  const long long slab = (long long)p.M * L.a.tiles_n[0] * 128;
  long long s = std::max<long long>(1, std::min<long long>(sk_cus() / L.total, nkt / 4));
  s = std::min<long long>(s, ws_floats / slab);
  if (!(p.alpha == 1.f && p.beta == 0.f && p.alpha_ptr == nullptr)) s = 1;
  s = std::max<long long>(s, 1);
  const long long kc = (nkt + s - 1) / s;
  L.a.kchunk[0] = (int)kc;
  L.extra = (int)((nkt + kc - 1) / kc);
  L.sk = L.extra > 1;
  return 0;
}

// CAPMI_GEMM_X3S (gemm_x3s.hip): K = 64, N in {64, 128, 256}, dense rows or a 1x1 / stride-1 conv input
// (optional prologue), store-only epilogue; grid = two persistent workgroups per CU over 64-row tiles
int plan_x3s(const capmi_gemm_problem* prob, int amode, int bmode, GemmLaunch& L) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(forward_modes(amode, bmode), CAPMI_EINVAL);
  CAPMI_REQUIRE(p.A && p.B && p.C && p.M >= 0 && p.K == 64 && (p.N == 64 || p.N == 128 || p.N == 256), CAPMI_EINVAL);
  // the store-only epilogue is x3s's only form (independent of the CAPMI_X3_PLAIN_EPI A/B switch)
  CAPMI_REQUIRE(store_only(p, p.N) == 1, CAPMI_EINVAL);
  CAPMI_REQUIRE(p.a_r1 <= 0 && prologue_paired(p), CAPMI_EINVAL);
  long long lda;
  if (amode == CAPMI_A_CONV_NHWC) {
    CAPMI_REQUIRE(p.cKH == 1 && p.cKW == 1 && p.cStride == 1 && p.cPad == 0 && p.cCin == 64 && p.cHo == p.cH &&
                      p.cWo == p.cW && p.M == p.cN * p.cHo * p.cWo,
                  CAPMI_EINVAL);
    lda = p.cCin;
  } else {
    CAPMI_REQUIRE(p.in_scale == nullptr, CAPMI_EINVAL);
    lda = p.lda;
  }
  CAPMI_REQUIRE(aligned16(p.A) && aligned16(p.B) && lda % 4 == 0 && lda >= 64 && p.ldb % 8 == 0 && p.ldb >= 64,
                CAPMI_EALIGN);
  CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE((reinterpret_cast<uintptr_t>(p.stats) & 7u) == 0, CAPMI_EALIGN);
  CAPMI_REQUIRE(fits31((long long)p.M * lda * 4) && b_planes_fit(p, 3), CAPMI_ERANGE);
  fill_one(L, FAM_X3S, p, amode, bmode, 64, p.N, 256);
  L.total = L.a.tiles_m[0];
  L.lda = lda;
  L.extra = (int)std::max<long long>(1, std::min<long long>(L.total, 2LL * cu_count()));
  return 0;
}

// the two passes that replace "x3s conv -> stored y -> bn_add_relu" (gemm_x3s.hip): plan_x3s's rules, N = 256
int plan_x3s_pass(const capmi_gemm_problem* prob, int amode, bool need_c, GemmLaunch& L) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  capmi_gemm_problem p = *prob;
  if (!need_c && p.C == nullptr) {  // the statistics pass has no C: plan it as the product it stands for
    p.C = const_cast<float*>(p.A);
    p.ldc = p.N;
  }
  CAPMI_TRY(plan_x3s(&p, amode, CAPMI_B_NMAJOR_W, L));
  CAPMI_REQUIRE(p.N == 256, CAPMI_EINVAL);
  if (!need_c) L.a.p[0].C = nullptr;
  return 0;
}

// CAPMI_GEMM_X3C (gemm_x3c.hip, round 4): the direct 3x3 conv for short channel axes (layer1)
int plan_x3c(const capmi_gemm_problem* prob, int amode, int bmode, GemmLaunch& L) {
  CAPMI_REQUIRE(prob != nullptr, CAPMI_EINVAL);
  const capmi_gemm_problem& p = *prob;
  CAPMI_REQUIRE(amode == CAPMI_A_CONV_NHWC && bmode == CAPMI_B_NMAJOR_W, CAPMI_EINVAL);
  CAPMI_REQUIRE(p.A && p.B && p.C && p.M >= 0 && p.N == 64 && p.ksplit == 1, CAPMI_EINVAL);
  CAPMI_REQUIRE(p.cKH == 3 && p.cKW == 3 && p.cStride == 1 && p.cPad == 1 && p.cHo == p.cH && p.cWo == p.cW &&
                    p.cCin % 32 == 0 && p.K == 9 * p.cCin && p.M == p.cN * p.cH * p.cW &&
                    p.cW <= gemm_x3c_max_width(),
                CAPMI_EINVAL);
  CAPMI_REQUIRE(store_only(p, 64) == 1 && p.a_r1 <= 0, CAPMI_EINVAL);  // its only epilogue, as x3s
  CAPMI_REQUIRE(prologue_paired(p), CAPMI_EINVAL);
  CAPMI_REQUIRE(aligned16(p.A) && aligned16(p.B) && p.ldb == p.K, CAPMI_EALIGN);
  CAPMI_REQUIRE(prologue_aligned(p), CAPMI_EALIGN);
  CAPMI_REQUIRE((reinterpret_cast<uintptr_t>(p.stats) & 7u) == 0, CAPMI_EALIGN);
  CAPMI_REQUIRE(fits31(conv_input_elems(p) * 4) && b_planes_fit(p, 3), CAPMI_ERANGE);
  CAPMI_REQUIRE(gemm_x3c_band_fits(p), CAPMI_EINVAL);  // (e.g. many 1-row images per tile)
  fill_one(L, FAM_X3C, p, amode, bmode, 256, 64, 512);
  L.total = L.a.tiles_m[0];
  L.extra = (int)L.total;
  return 0;
}

// ------------------------------------------------------------------------------------
// flags -> family -> plan; the launch
// ------------------------------------------------------------------------------------
// The workspace as a plan sees it: bf16-IO plans stream-K only with one, x3w bounds its k-splits by the floats
// behind the stream-K flags. The plan query assumes the library's own workspace; operands = false is the query.
int plan_flags(const capmi_gemm_problem* prob, int amode, int bmode, int tile, int flags, bool operands, bool have_ws,
               long long ws_floats, GemmLaunch& L) {
  switch (flags) {
    case CAPMI_GEMM_BF16_IO: return plan_bf16_io(prob, amode, bmode, tile, operands, have_ws, L);
    case CAPMI_GEMM_X3: return plan_x3(prob, amode, bmode, tile, L);
    case CAPMI_GEMM_X3P: return plan_x3p(prob, amode, bmode, L);
    case CAPMI_GEMM_X3D: return plan_x3d(prob, amode, bmode, L);
    case CAPMI_GEMM_X3S: return plan_x3s(prob, amode, bmode, L);
    case CAPMI_GEMM_X3C: return plan_x3c(prob, amode, bmode, L);
    case CAPMI_GEMM_X3W: return plan_x3w(prob, amode, bmode, ws_floats, 3, L);
    case CAPMI_GEMM_X3W | CAPMI_GEMM_BF16: return plan_x3w(prob, amode, bmode, ws_floats, 1, L);
    default: return plan_nt(prob, amode, bmode, tile, flag_terms(flags), L);
  }
}

// the family's kernel launcher on `blocks` workgroups
int launch_kernel(const GemmLaunch& L, const GemmArgs& a, int blocks, hipStream_t s) {
  switch (L.family) {
    case FAM_NT:
      if (!L.nt_ok) return gemm_v1_launch(a, L.amode, L.bmode, L.bm, L.vec, blocks, s);
      return gemm_nt_launch(a, L.amode, L.bmode, L.bm, L.bn, blocks, s, L.terms, L.threads);
    case FAM_BF16_IO: return gemm_bf16_launch(a, L.amode, L.bm, L.bn, blocks, s, L.extra);
    case FAM_X3: return gemm_x3_launch(a, L.amode, L.bn, blocks, s);
    case FAM_X3P: return gemm_x3p_launch(a, L.amode, L.extra, blocks, s);
    case FAM_X3D: return gemm_x3d_launch(a, L.amode, blocks, s);
    case FAM_X3S: return gemm_x3s_launch(a.p[0], L.lda, (int)L.total, L.extra, s);
    case FAM_X3C: return gemm_x3c_launch(a.p[0], (int)L.total, s);
    case FAM_X3W: return gemm_x3w_launch(a, L.bmode, blocks, s, L.terms);
  }
  return CAPMI_EINVAL;
}

// Launch a plan: nothing for an empty grid; the data-parallel grid; or, stream-K decided, the persistent grid on the
// attached workspace. Without a workspace the v2 kernel's stream-K plan is refused and the x3 families run the
// data-parallel form of the same plan. x3w: S k-split slabs in the workspace, then their sum.
int launch(const GemmLaunch& L, void* workspace, long long ws_bytes, hipStream_t s) {
  if (L.total == 0) return 0;
  if (L.family == FAM_X3W) {
    CAPMI_REQUIRE(workspace == nullptr || aligned16(workspace), CAPMI_EINVAL);
    const int S = L.extra;
    if (S == 1) return launch_kernel(L, L.a, (int)L.total, s);
    GemmArgs a = L.a;
    a.sk_part = reinterpret_cast<float*>(static_cast<char*>(workspace) + sk_flag_bytes(cu_count()));
    CAPMI_TRY(launch_kernel(L, a, (int)(L.total * S), s));
    const capmi_gemm_problem& p = a.p[0];
    const int ldp = a.tiles_n[0] * 128;
    return capmi_splitk_reduce(a.sk_part, S, (long long)p.M * ldp, p.M, p.N, ldp, nullptr, p.C, p.ldc, s);
  }
  CAPMI_REQUIRE(!L.sk || workspace != nullptr || L.family != FAM_NT, CAPMI_EINVAL);
  if (!L.sk || workspace == nullptr) return launch_kernel(L, L.a, (int)L.total, s);
  GemmArgs a = L.a;
  CAPMI_TRY(sk_attach(a, L.total, L.nkt, L.slots, L.hybrid, workspace, ws_bytes));
  return launch_kernel(L, a, a.sk_workers, s);
}
}  // namespace

// ------------------------------------------------------------------------------------
// the C ABI (include/capmi.h)
// ------------------------------------------------------------------------------------
extern "C" int capmi_gemm_stat_tiles(int M, int tile) {
  // statistics rows are always kept per 64-row slice, whatever tile ran (see capmi.h)
  (void)tile;
  return (M + 63) / 64;
}

extern "C" long long capmi_gemm_workspace_flag_bytes(void) { return sk_flag_bytes(cu_count()); }

extern "C" long long capmi_gemm_workspace_bytes(void) {
  const int cus = cu_count();
  // parked partials: (WGs per CU) * BM * BN floats per CU is 64 KB for 4 x 64x64 and for
  // 2 x 128x64, 128 KB for 2 x 128x128 and 1 x 256x128
  return sk_flag_bytes(cus) + (long long)cus * 128 * 1024;
}

extern "C" int capmi_gemm(const capmi_gemm_problem* probs, int nprob, int amode, int bmode,
                          int tile, void* stream) {
  return capmi_gemm_ex(probs, nprob, amode, bmode, tile, 0, stream);
}

extern "C" int capmi_gemm_ex(const capmi_gemm_problem* probs, int nprob, int amode, int bmode, int tile, int flags,
                             void* stream) {
  const int terms = flag_terms(flags);
  CAPMI_REQUIRE(terms >= 0, CAPMI_EINVAL);
  CAPMI_REQUIRE(terms == 0 || (terms_mode_ok(terms, amode, bmode) && tile != CAPMI_TILE_128_W8), CAPMI_EINVAL);
  GemmLaunch g;
  CAPMI_TRY(plan_nt_group(probs, nprob, amode, bmode, tile, g));
  // shapes the split forms do not cover (unaligned / generic-kernel problems, a prologue): the fp32 kernel
  bool split_ok = g.nt_ok && g.vec;
  for (int i = 0; i < nprob; ++i) split_ok = split_ok && probs[i].in_scale == nullptr;
  g.terms = split_ok ? terms : 0;
  return launch(g, nullptr, 0, as_stream(stream));
}

extern "C" int capmi_gemm_sk_plan(const capmi_gemm_problem* prob, int amode, int bmode, int tile, int flags,
                                  int* bm, int* bn, int* stream_k, int* generic, int* threads) {
  GemmLaunch L;
  const long long ws_floats = (capmi_gemm_workspace_bytes() - capmi_gemm_workspace_flag_bytes()) / 4;
  CAPMI_TRY(plan_flags(prob, amode, bmode, tile, flags, false, true, ws_floats, L));
  if (threads) *threads = L.threads;
  if (bm) *bm = L.bm;
  if (bn) *bn = L.bn;
  if (stream_k) *stream_k = L.sk ? 1 : 0;
  if (generic) *generic = L.extra;
  return 0;
}

extern "C" int capmi_gemm_sk_ex(const capmi_gemm_problem* prob, int amode, int bmode, int tile, int flags,
                                void* workspace, long long ws_bytes, void* stream) {
  GemmLaunch L;
  const long long flag_bytes = sk_flag_bytes(cu_count());
  const long long ws_floats = workspace != nullptr && ws_bytes > flag_bytes ? (ws_bytes - flag_bytes) / 4 : 0;
  CAPMI_TRY(plan_flags(prob, amode, bmode, tile, flags, true, workspace != nullptr, ws_floats, L));
  return launch(L, workspace, ws_bytes, as_stream(stream));
}

extern "C" int capmi_gemm_sk(const capmi_gemm_problem* prob, int amode, int bmode, int tile,
                             void* workspace, long long ws_bytes, void* stream) {
  return capmi_gemm_sk_ex(prob, amode, bmode, tile, 0, workspace, ws_bytes, stream);
}

extern "C" int capmi_gemm_x3s_stats(const capmi_gemm_problem* prob, int amode, void* stream) {
  GemmLaunch L;
  CAPMI_TRY(plan_x3s_pass(prob, amode, false, L));
  const capmi_gemm_problem& p = L.a.p[0];
  CAPMI_REQUIRE(p.stats != nullptr, CAPMI_EINVAL);
  if (p.M == 0) return 0;
  return gemm_x3s_stats_launch(p, L.lda, (int)L.total, L.extra, as_stream(stream));
}

extern "C" int capmi_gemm_x3s_tail(const capmi_gemm_problem* prob, int amode, const float* scale, const float* shift,
                                   const float* other, long long ld_other, const float* res_scale,
                                   const float* res_shift, int acc_is_residual, void* stream) {
  GemmLaunch L;
  CAPMI_REQUIRE(scale && shift && other && (acc_is_residual == 0 || acc_is_residual == 1), CAPMI_EINVAL);
  // the accumulator's own BN: scale / shift as the main branch, res_scale / res_shift as the residual branch
  CAPMI_REQUIRE(acc_is_residual ? (res_scale && res_shift) : (!res_scale && !res_shift), CAPMI_EINVAL);
  CAPMI_TRY(plan_x3s_pass(prob, amode, true, L));
  capmi_gemm_problem& p = L.a.p[0];
  CAPMI_REQUIRE(aligned16(other), CAPMI_EALIGN);
  CAPMI_REQUIRE(ld_other >= p.N && (long long)p.M * ld_other * 4 < (1LL << 31), CAPMI_EINVAL);
  // rows past M are dropped by the two descriptors' bounds: a ragged last tile's offsets must not wrap 32 bits
  CAPMI_REQUIRE(((long long)p.M + 63) * std::max(ld_other, p.ldc) * 4 < (1LL << 32), CAPMI_ERANGE);
  if (p.M == 0) return 0;
  p.stats = nullptr;
  const X3sTail e{scale, shift, other, ld_other, res_scale, res_shift};
  return gemm_x3s_tail_launch(p, L.lda, (int)L.total, L.extra, e, acc_is_residual != 0, as_stream(stream));
}
