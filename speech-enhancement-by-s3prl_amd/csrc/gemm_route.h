// gemm_route.h -- which kernel runs a se_gemm_bf16 call: one pure function of the call's shape facts.
//
// Host-only and free of HIP (a plain C++ compiler takes it: tests/test_gemm_route.py walks it under the sanitizers).  One predicate per
// route says what that kernel CAN run; gemm_route() alone holds the order of preference and the measured thresholds.  The launchers
// (gemm2.hip, gemm6.hip, gemm4.hip) re-check their predicate and fail the call otherwise: handing them anything else is a programming error.
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace se {

constexpr int kGemmActIdentity = 0, kGemmActGelu = 3;      // = SE_ACT_IDENTITY / SE_ACT_GELU of se_amd.h (static_assert in gemm.hip)

// A call that passed se_gemm_bf16's argument checks: M, N, K > 0, K % 64 == 0, lda / ldw >= K and multiples of 8, ldc >= N, A and W 16-B
// aligned, at least one output.
struct GemmCall {
  int M, N, K, lda, ldw, ldc, act;
  bool has_bias, has_residual, has_bf16, has_f32;
  bool vec_ok;        // the vector epilogues' rows are 16-B aligned: ldc % 8 == 0 and bias / residual / both outputs 16-B aligned (null counts)
  bool ptrs16;        // the row-complete kernel's test: every pointer of the call 16-B aligned (null counts)
};

enum class GemmRoute {
  Tile128x2,          // gemm2.hip <2, 2, 0>: 128 x 128 tiles, two workgroups per CU
  RowComplete768,     // gemm4.hip gemm7_res_ln_kernel<0, 0, 0, 1, 0>: 128 x 768 row tiles, no LayerNorm
  Persistent256,      // gemm6.hip gemm6p_bf16_kernel: 256 x 256 tiles dealt to one workgroup per CU
  Tile256,            // gemm6.hip gemm6_bf16_kernel: 256 x 256, one workgroup per tile
  PingPong256x128,    // gemm2.hip <4, 3, 1>
  Lockstep256x128,    // gemm2.hip <4, 3, 0>
};

// The switches that survive (A/B tools and tests set them), read once by gemm_tuning().
struct GemmTuning {
  int small_m = 4096;               // SE_AMD_GEMM_SMALL_M: row count up to which the 128 x 128 kernel is used (kernel benchmarks set 0)
  int row_complete = 1;             // SE_AMD_GEMM7_PLAIN: 0 restores the 256 x 256 x 64 kernel for N = 768
  int row_complete_min_k = 1536;    // SE_AMD_GEMM7_PLAIN_MINK
  int persistent = 1;               // SE_AMD_GEMM6P: 0 = one workgroup per tile for every shape
  int dual = 1;                     // SE_AMD_GEMM6_DUAL: 0 = FFN1 pre-activation and GELU as two launches
  int group_m = 4;                  // SE_AMD_GEMM_GROUPM: tile rows swept n-major inside an XCD's range (256 x 256 kernels)
  int group_m2 = 1;                 // SE_AMD_GEMM_GROUPM2: the same for gemm2.hip
  int late_start = 2;               // SE_AMD_GEMM6P_LATE | SE_AMD_GEMM6P_SKEW << 8 (gemm6p_bf16_kernel's staggered start)
};

inline GemmTuning gemm_tuning_from_env() {
  GemmTuning t;
  auto env = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
  env("SE_AMD_GEMM_SMALL_M", t.small_m);
  env("SE_AMD_GEMM7_PLAIN", t.row_complete);
  env("SE_AMD_GEMM7_PLAIN_MINK", t.row_complete_min_k);
  env("SE_AMD_GEMM6P", t.persistent);
  env("SE_AMD_GEMM6_DUAL", t.dual);
  env("SE_AMD_GEMM_GROUPM", t.group_m);
  env("SE_AMD_GEMM_GROUPM2", t.group_m2);
  env("SE_AMD_GEMM6P_LATE", t.late_start);
  int skew = 0;
  env("SE_AMD_GEMM6P_SKEW", skew);
  t.late_start |= (skew & 0xff) << 8;
  if (t.group_m < 1) t.group_m = 1;
  if (t.group_m2 < 1) t.group_m2 = 1;
  return t;
}

inline const GemmTuning& gemm_tuning() {
  static const GemmTuning t = gemm_tuning_from_env();
  return t;
}

// ---- what each kernel can run

// the compile-time epilogues shared by the 256 x 256 kernels and gemm2.hip's specialised forms: 4-column vector stores, one output,
// identity or GELU
inline bool gemm_vec_one_out(const GemmCall& c) {
  const bool vec = c.vec_ok && (c.N % 4 == 0) && (c.ldc % 4 == 0);
  const bool one_out = c.has_bf16 != c.has_f32;
  return vec && one_out && (c.act == kGemmActIdentity || c.act == kGemmActGelu);
}

inline bool gemm_tile128x2_ok(const GemmCall&) { return true; }          // generic epilogue: any validated call
inline bool gemm_lockstep256x128_ok(const GemmCall&) { return true; }    // the same kernel family at 256 x 128
inline bool gemm_pingpong256x128_ok(const GemmCall& c) { return c.K >= 2 * 64; }      // its prologue waits for K-tile 0 with K-tile 1 in flight

// 64-deep K-tiles, at least two, 32-bit source offsets, every pointer 16-B aligned; N = ldc = 768, no activation
inline bool gemm_row_complete768_ok(const GemmCall& c) {
  return c.N == 768 && c.ldc == 768 && c.act == kGemmActIdentity && c.vec_ok && c.K % 64 == 0 && c.K >= 128 &&
         (size_t)c.M * c.lda < (1u << 31) && (size_t)768 * c.ldw < (1u << 31) && c.ptrs16;
}

// gemm6_bf16_kernel's instantiations: bf16 or fp32 out, identity or GELU, without residual; identity + residual -> fp32
inline bool gemm_tile256_ok(const GemmCall& c) {
  if (!gemm_vec_one_out(c) || c.K % 64 != 0 || c.K < 2 * 64) return false;
  const bool gelu = c.act == kGemmActGelu;
  return !c.has_residual || (!gelu && !c.has_bf16);
}

// the persistent kernel's shape: whole column tiles, an even number of K-tiles (at least four), 16-B output rows, 32-bit source offsets,
// several tiles per CU.  Shared with se_gemm6_dual_gelu_launch.
inline bool gemm_persistent256_shape_ok(int M, int N, int K, int lda, int ldw, int ldc) {
  return N % 256 == 0 && N <= 8192 && K % 64 == 0 && (K / 64) % 2 == 0 && K >= 4 * 64 && (ldc % 8) == 0 && (size_t)M * lda < (1u << 31) &&
         (size_t)N * ldw < (1u << 31) && (size_t)((M + 255) / 256) * (N / 256) > 256;
}

// bf16 output without residual (vec_ok covers the output's 16-B alignment)
inline bool gemm_persistent256_ok(const GemmCall& c) {
  return gemm_tile256_ok(c) && c.has_bf16 && !c.has_residual && gemm_persistent256_shape_ok(c.M, c.N, c.K, c.lda, c.ldw, c.ldc);
}

inline bool gemm_route_ok(GemmRoute r, const GemmCall& c) {
  switch (r) {
    case GemmRoute::Tile128x2: return gemm_tile128x2_ok(c);
    case GemmRoute::RowComplete768: return gemm_row_complete768_ok(c);
    case GemmRoute::Persistent256: return gemm_persistent256_ok(c);
    case GemmRoute::Tile256: return gemm_tile256_ok(c);
    case GemmRoute::PingPong256x128: return gemm_pingpong256x128_ok(c);
    case GemmRoute::Lockstep256x128: return gemm_lockstep256x128_ok(c);
  }
  return false;
}

// ---- the order of preference and the thresholds

inline GemmRoute gemm_route(const GemmCall& c, const GemmTuning& t) {
  // serving-size batches (M = B*T <= 8 utterances of 10 s): a 1 001-row GEMM makes 4 row tiles of 256 -- 36 workgroups for the QKV
  // projection on 256 CUs.  128 x 128 tiles at two workgroups per CU fill the chip 4x better: 0.85 vs 1.85 ms per utterance pass
  // at B = 1, 1.81 vs 2.61 ms at B = 8 (tools/small_batch_sweep.sh); from B = 16 on the large tiles win again.
  // Round 2, with the 64-deep kernels: the crossover moved down to ~4 000 rows (ms per pass, small / large tiles: B = 4 1.14 / 1.14,
  // B = 5 1.30 / 1.22, B = 6 1.51 / 1.37, B = 8 1.69 / 1.57), so the threshold is 4 096 rows (was 8 192).
  if (c.M <= t.small_m) return GemmRoute::Tile128x2;
  // round 4: N = 768 with K >= 1536 goes to the row-complete kernel without its LayerNorm (gemm4.hip: 251 tiles of 128 x 768 = ONE round,
  // where 256 x 256 tiles make 1.48).  Same box, interleaved (profiles/r04_revalidate.txt): fine-tune step 18.59 / 18.70 -> 18.30 / 18.28 ms.
  // ... from 160 row tiles on (M > 20 352: the x3 batch sweep, profiles/r04_x3_rowln_batch.txt); below that the 256 x 256 / 256 x 128
  // kernels cover the chip better
  if (t.row_complete && c.K >= t.row_complete_min_k && (c.M + 127) / 128 >= 160 && gemm_row_complete768_ok(c)) return GemmRoute::RowComplete768;
  // 256 x 256 kernels for wide outputs (enough tiles to fill 256 CUs several times).  Round 4: N = 768 outputs with a long reduction (the
  // training path's FFN2 forward and FFN1 input gradient, K = 3072: 190 vs 205 us) also run faster there in spite of the 1.48-round tile
  // count; at K = 768 the 256 x 128 ping-pong kernel keeps its lead (66 vs 70 us)
  if (c.N >= 1536 || (c.N >= 768 && c.K >= 1536)) {
    if (t.persistent && gemm_persistent256_ok(c)) return GemmRoute::Persistent256;
    if (gemm_tile256_ok(c)) return GemmRoute::Tile256;
  }
  return gemm_pingpong256x128_ok(c) ? GemmRoute::PingPong256x128 : GemmRoute::Lockstep256x128;
}

}  // namespace se
