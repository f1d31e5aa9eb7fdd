// gemm_launch.h -- a validated se_gemm_bf16 call and the per-file launchers that gemm.hip's switch hands it to (internal).
#pragma once
#include "common.h"
#include "gemm_route.h"

namespace se {

struct GemmArgs {
  const uint16_t* A; int lda; const uint16_t* W; int ldw; const float* bias; const float* residual; int M, N, K, act;
  uint16_t* out_bf16; float* out_f32; int ldc; hipStream_t st;
};

inline GemmCall gemm_call_of(const GemmArgs& g) {
  const uintptr_t epi = (uintptr_t)g.out_bf16 | (uintptr_t)g.out_f32 | (uintptr_t)g.residual | (uintptr_t)g.bias;
  GemmCall c{g.M, g.N, g.K, g.lda, g.ldw, g.ldc, g.act, g.bias != nullptr, g.residual != nullptr, g.out_bf16 != nullptr, g.out_f32 != nullptr, false, false};
  c.vec_ok = (g.ldc % 8 == 0) && (epi % 16 == 0);      // vector epilogue needs 16-B aligned rows of every tensor it touches
  c.ptrs16 = (((uintptr_t)g.A | (uintptr_t)g.W | epi) % 16) == 0;
  return c;
}

// Each takes the routes of its file only and re-checks the route's predicate (gemm_route.h): anything else fails with SE_ERR_INVALID.
int launch_gemm2(const GemmArgs& g, GemmRoute route);      // gemm2.hip: Tile128x2, PingPong256x128, Lockstep256x128
int launch_gemm6(const GemmArgs& g, GemmRoute route);      // gemm6.hip: Persistent256, Tile256

}  // namespace se

// gemm4.hip: RowComplete768 (N = ldc = 768, no activation).  Exported for its direct test.
extern "C" int se_gemm7_plain_launch(const uint16_t* A, int lda, const uint16_t* W, int ldw, const float* bias, const float* residual_f32, int M, int K,
                                     uint16_t* out_bf16, float* out_f32, void* stream);
