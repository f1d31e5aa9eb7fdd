// Stand-alone check of csrc/gemm_route.h (built and run by tests/test_gemm_route.py with the host compiler, -Wall -Werror and the address /
// undefined-behaviour sanitizers; includes nothing else of the project).  Over a grid of se_gemm_bf16 calls it checks that
//   1. the chosen route's own predicate holds,
//   2. the 256 x 128 routes accept every validated call, so dispatch is total,
//   3. the route equals what the try-and-fall-through chain that gemm_route() replaced would have launched.  That chain is restated below
//      launcher by launcher, each with its own "return 1 = not mine" conditions, exactly as se_gemm_bf16, se_gemm7_plain_launch,
//      se_gemm6_launch and se_gemm2_launch had them; it shares no code with the header.
#include <stdio.h>

#include "gemm_route.h"

namespace {

struct Raw {
  int M, N, K, lda, ldw, ldc, act;
  bool bias, res, obf, of32;
  bool aligned;      // bias / residual / outputs 16-B aligned (A and W always are: se_gemm_bf16 requires it)
};

enum Old { kOldGemm2Small, kOldGemm7Plain, kOldGemm6Persistent, kOldGemm6Tile, kOldGemm2PingPong, kOldGemm2Lockstep };

// se_gemm7_plain_launch: 1 = not mine
int old_gemm7_plain(const Raw& r) {
  if (!(r.K % 64 == 0 && r.K >= 128 && (size_t)r.M * r.lda < (1u << 31) && (size_t)768 * r.ldw < (1u << 31))) return 1;
  if (!r.aligned) return 1;
  return 0;
}

// se_gemm6_launch: 1 = not mine
int old_gemm6(const Raw& r, int vec_ok, int persistent, Old* out) {
  const bool vec = vec_ok && (r.N % 4 == 0) && (r.ldc % 4 == 0);
  const bool one_out = r.obf != r.of32;
  if (!vec || !one_out || r.K % 64 != 0 || r.K < 2 * 64 || (r.act != 0 && r.act != 3)) return 1;
  const bool gelu = r.act == 3, res = r.res, obf = r.obf;
  if (persistent && obf && !res && r.N % 256 == 0 && r.N <= 8192 && (r.K / 64) % 2 == 0 && r.K >= 4 * 64 && (r.ldc % 8) == 0 && r.aligned &&
      (size_t)r.M * r.lda < (1u << 31) && (size_t)r.N * r.ldw < (1u << 31) && (size_t)((r.M + 256 - 1) / 256) * (r.N / 256) > 256) {
    *out = kOldGemm6Persistent;
    return 0;
  }
  *out = kOldGemm6Tile;
  if (!gelu && !res && obf) return 0;
  if (gelu && !res && obf) return 0;
  if (!gelu && res && !obf) return 0;
  if (!gelu && !res && !obf) return 0;
  if (gelu && !res && !obf) return 0;
  return 1;
}

// se_gemm3_launch (N >= 1536 only): 1 = not mine.  It never took a call that se_gemm6_launch had declined; the walk asserts that too.
int old_gemm3(const Raw& r, int vec_ok) {
  const bool vec = vec_ok && (r.N % 4 == 0) && (r.ldc % 4 == 0);
  const bool one_out = r.obf != r.of32;
  if (!vec || !one_out || r.K % 32 != 0 || r.K < 3 * 32 || (r.act != 0 && r.act != 3)) return 1;
  const bool gelu = r.act == 3, res = r.res, obf = r.obf;
  if (!gelu && !res && obf) return 0;
  if (gelu && !res && obf) return 0;
  if (!gelu && res && !obf) return 0;
  if (!gelu && !res && !obf) return 0;
  if (gelu && !res && !obf) return 0;
  return 1;
}

// se_gemm_bf16 with its default switches except the three that survive as routing switches
bool old_route(const Raw& r, int small_m, int plain7, int plain7_mink, int persistent, Old* out) {
  const int vec_ok = (r.ldc % 8 == 0) && r.aligned;
  if (r.M <= small_m) { *out = kOldGemm2Small; return true; }
  if (plain7 && r.N == 768 && r.ldc == 768 && r.K >= plain7_mink && r.act == 0 && vec_ok && (r.M + 127) / 128 >= 160) {
    if (old_gemm7_plain(r) == 0) { *out = kOldGemm7Plain; return true; }
  }
  if (r.N >= 1536 || (r.N >= 768 && r.K >= 1536)) {
    if (old_gemm6(r, vec_ok, persistent, out) == 0) return true;
  }
  if (r.N >= 1536 && old_gemm3(r, vec_ok) == 0) return false;      // the retired 256 x 256 kernel would have run: not expected for any call
  *out = (r.K >= 2 * 64) ? kOldGemm2PingPong : kOldGemm2Lockstep;
  return true;
}

se::GemmRoute as_route(Old o) {
  switch (o) {
    case kOldGemm2Small: return se::GemmRoute::Tile128x2;
    case kOldGemm7Plain: return se::GemmRoute::RowComplete768;
    case kOldGemm6Persistent: return se::GemmRoute::Persistent256;
    case kOldGemm6Tile: return se::GemmRoute::Tile256;
    case kOldGemm2PingPong: return se::GemmRoute::PingPong256x128;
    default: return se::GemmRoute::Lockstep256x128;
  }
}

}  // namespace

int main() {
  const int Ms[] = {1, 128, 4096, 4097, 7168, 7169, 20352, 20353, 32032};
  const int Ns[] = {128, 201, 768, 1536, 2304, 3072};
  const int Ks[] = {64, 128, 256, 768, 1536, 3072};
  const int acts[] = {0, 3, 1};      // identity, GELU, ReLU
  se::GemmTuning tunings[3];
  tunings[1].row_complete = 0;
  tunings[2].persistent = 0;
  long calls = 0, bad = 0;
  long per_route[6] = {0, 0, 0, 0, 0, 0};
  for (const se::GemmTuning& t : tunings)
    for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int act : acts)
      for (int bias = 0; bias < 2; ++bias) for (int res = 0; res < 2; ++res) for (int outs = 1; outs < 4; ++outs) for (int aligned = 0; aligned < 2; ++aligned) {
        const Raw r{M, N, K, K, K, N, act, bias != 0, res != 0, (outs & 1) != 0, (outs & 2) != 0, aligned != 0};
        const se::GemmCall c{M, N, K, K, K, N, act, r.bias, r.res, r.obf, r.of32, aligned && N % 8 == 0, aligned != 0};
        const se::GemmRoute got = se::gemm_route(c, t);
        ++calls;
        const int gi = static_cast<int>(got);
        bool ok = gi >= 0 && gi < 6;
        if (ok) ++per_route[gi];
        ok = ok && se::gemm_route_ok(got, c);                                                             // 1
        ok = ok && se::gemm_lockstep256x128_ok(c) && (se::gemm_pingpong256x128_ok(c) || K == 64);          // 2
        Old old = kOldGemm2Lockstep;
        ok = ok && old_route(r, t.small_m, t.row_complete, t.row_complete_min_k, t.persistent, &old) && as_route(old) == got;      // 3
        if (!ok && ++bad <= 20)
          fprintf(stderr, "MISMATCH M=%d N=%d K=%d act=%d bias=%d res=%d outs=%d aligned=%d: route %d, chain %d\n", M, N, K, act, bias, res, outs, aligned, gi,
                  static_cast<int>(as_route(old)));
      }
  printf("calls %ld bad %ld routes", calls, bad);
  for (long n : per_route) printf(" %ld", n);
  printf("\n");
  // a walk that never reaches a route proves nothing about it
  for (long n : per_route)
    if (n == 0) return 2;
  return bad ? 1 : 0;
}
