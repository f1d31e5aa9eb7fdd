// gemm.hip -- C[M,N] = epilogue(A[M,K] . W[N,K]^T + bias): the encoder's dense contractions on bf16 MFMA
// (rows B1-B4: QKV / attention-output / FFN / spec-head projections).
//
// Both operands are K-contiguous (activations row-major, nn.Linear weights (out, in)), which is exactly the
// lane layout of v_mfma_f32_16x16x32_bf16 (lane l: row l&15, k = 8 (l>>4) .. +7).
//
// This file is the entry point only: validate -> gemm_route() (gemm_route.h: the one place that says which kernel runs which call)
// -> launch.  The kernels live in gemm2.hip (128 x 128 and 256 x 128 tiles), gemm6.hip (256 x 256, persistent or one workgroup per
// tile) and gemm4.hip (128 x 768 row-complete tiles).
// Bound: MFMA (2 M N K flop against the 2.5 PFLOP/s dense bf16 peak).
#include "gemm_launch.h"

static_assert(se::kGemmActIdentity == SE_ACT_IDENTITY && se::kGemmActGelu == SE_ACT_GELU, "gemm_route.h mirrors se_act");

extern "C" int se_gemm_bf16(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias,
                            const float* residual_f32, int M, int N, int K, int act,
                            uint16_t* out_bf16, float* out_f32, int ldc, void* stream) {
  SE_REQUIRE(A && W && (out_bf16 || out_f32), "se_gemm_bf16: null argument");
  SE_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0, "se_gemm_bf16: K=%d must be a positive multiple of %d", K, 64);
  SE_REQUIRE(lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0, "se_gemm_bf16: lda/ldw must be >= K and multiples of 8 (16-B rows)");
  SE_REQUIRE(ldc >= N, "se_gemm_bf16: ldc < N");
  SE_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)W % 16) == 0, "se_gemm_bf16: operands must be 16-B aligned");
  const se::GemmArgs g{A, lda, W, ldw, bias, residual_f32, M, N, K, act, out_bf16, out_f32, ldc, se::as_stream(stream)};
  const se::GemmRoute route = se::gemm_route(se::gemm_call_of(g), se::gemm_tuning());
  switch (route) {
    case se::GemmRoute::RowComplete768:
      return se_gemm7_plain_launch(A, lda, W, ldw, bias, residual_f32, M, K, out_bf16, out_f32, stream);
    case se::GemmRoute::Persistent256:
    case se::GemmRoute::Tile256:
      return se::launch_gemm6(g, route);
    case se::GemmRoute::Tile128x2:
    case se::GemmRoute::PingPong256x128:
    case se::GemmRoute::Lockstep256x128:
      return se::launch_gemm2(g, route);
  }
  SE_REQUIRE(false, "se_gemm_bf16: no route");
}

// internal (not part of the public header): the route of a call under default tuning, as the GemmRoute value.  `aligned`: every pointer of
// the call is 16-B aligned.  Touches no device.
extern "C" int se_gemm_route_of(int M, int N, int K, int lda, int ldw, int ldc, int act, int has_bias, int has_residual, int has_bf16, int has_f32,
                                int aligned) {
  SE_REQUIRE(M > 0 && N > 0 && K > 0 && K % 64 == 0 && lda >= K && ldw >= K && lda % 8 == 0 && ldw % 8 == 0 && ldc >= N && (has_bf16 || has_f32),
             "se_gemm_route_of: not a valid se_gemm_bf16 call (M=%d N=%d K=%d lda=%d ldw=%d ldc=%d)", M, N, K, lda, ldw, ldc);
  const se::GemmCall c{M, N, K, lda, ldw, ldc, act, has_bias != 0, has_residual != 0, has_bf16 != 0, has_f32 != 0,
                       aligned && ldc % 8 == 0, aligned != 0};
  return static_cast<int>(se::gemm_route(c, se::GemmTuning{}));
}
