// Stand-alone check of csrc/mhsa_route.h (built and run by tests/test_mhsa_route.py with the host compiler, -Wall -Werror and the address /
// undefined-behaviour sanitizers; includes nothing else of the project).  Over a grid of attention forward calls it checks that
//   1. the route equals the kernel that the launch chain which mhsa_route() replaced would have launched,
//   2. mhsa_grid() gives that chain's grid and workgroup size,
//   3. the chosen route's own predicate holds exactly where the old chain launched, and fails exactly where the old chain failed the call
//      (the 8-wave kernel's 31-bit DMA offsets, the dropout kernel's 32-bit pair index): there is no fall-back in either.
// The old chain is restated below function by function, as mhsa_fwd_launch, mhsa_prescaled_launch, se_mhsaN_fwd_launch and
// se_mhsa_fwd_prescaled_bf16 had it in the product build; it shares no code with the header.
#include <stdio.h>

#include "mhsa_route.h"

namespace {

enum OldKernel { kOldFwd300, kOldFwd210, kOldFwd301, kOldMhsaN841 };      // mhsa_fwd_kernel<3,0,0> / <2,1,0> / <3,0,1>, mhsaN_fwd_kernel<8,4,1>

struct OldLaunch {
  OldKernel kernel;
  int grid_x, threads;
  bool failed;        // an SE_REQUIRE of the chain returned SE_ERR_INVALID instead of launching
};

// mhsa_fwd_launch (se_mhsa_fwd_bf16, se_mhsa_fwd_lse_bf16) with SE_AMD_MHSA_OCC unset
OldLaunch old_fwd(int B, int T, int heads, bool thr16) {
  OldLaunch o{kOldFwd300, (T + 128 - 1) / 128, 256, false};
  if (thr16) {
    o.kernel = kOldFwd210;
    if (!((double)B * heads * T * ((T + 1) / 2) < 4294967296.0)) o.failed = true;
  }
  return o;
}

// se_mhsaN_fwd_launch(nw = 8, wpe = 4)
OldLaunch old_mhsaN(int T, int heads) {
  const int H = heads * 64, nw = 8;
  OldLaunch o{kOldMhsaN841, (T + nw * 32 - 1) / (nw * 32), 512, false};
  if (!((double)T * 3.0 * H * 2.0 < 2147483648.0)) o.failed = true;
  return o;
}

// mhsa_prescaled_launch(pipe) for the two variants of the product build
OldLaunch old_prescaled(int T, int heads, int pipe) {
  if (pipe == 10) return old_mhsaN(T, heads);
  return OldLaunch{kOldFwd301, (T + 128 - 1) / 128, 256, false};
}

// se_mhsa_fwd_prescaled_bf16: pipe = SE_AMD_MHSA_PIPE (-1 unset), min_wgs = SE_AMD_MHSA8_MIN_WGS
OldLaunch old_prescaled_default(int B, int T, int heads, int pipe, int min_wgs) {
  if (pipe >= 0) return old_prescaled(T, heads, pipe);
  const long wgs8 = (long)((T + 255) / 256) * heads * B;
  return old_prescaled(T, heads, wgs8 >= min_wgs ? 10 : 0);
}

se::MhsaRoute as_route(OldKernel k) {
  switch (k) {
    case kOldFwd300: return se::MhsaRoute::Wave4;
    case kOldFwd210: return se::MhsaRoute::Wave4Dropout;
    case kOldFwd301: return se::MhsaRoute::Wave4Prescaled;
    default: return se::MhsaRoute::Wave8Prescaled;
  }
}

}  // namespace

int main() {
  const int Bs[] = {1, 2, 15, 16, 32, 59, 191, 192, 767, 768, 769, 65535};
  const int Ts[] = {1, 64, 127, 128, 129, 255, 256, 257, 1001, 466033, 466034, 5592406};      // 466034 x 12 heads, 5592406 x 1 head: past 2^31 bytes
  const int Hs[] = {1, 2, 4, 12, 13};
  se::MhsaTuning tunings[4];
  tunings[1].force_variant = 0;
  tunings[2].force_variant = 10;
  tunings[3].wave8_min_wgs = 1;
  long calls = 0, bad = 0, failed_calls = 0;
  long per_route[4] = {0, 0, 0, 0};
  long at_wgs[3] = {0, 0, 0};      // default-tuning prescaled calls with 767 / 768 / 769 8-wave workgroups
  for (const se::MhsaTuning& t : tunings)
    for (int B : Bs) for (int T : Ts) for (int heads : Hs) for (int prescaled = 0; prescaled < 2; ++prescaled) for (int dropout = 0; dropout < 2; ++dropout) {
      if (prescaled && dropout) continue;      // the prescaled entries have no dropout
      for (int v = 0; v <= 16; ++v)
        if (se::mhsa_variant_ok(v) != (v == 0 || v == 10)) ++bad;
      const OldLaunch old = prescaled ? old_prescaled_default(B, T, heads, t.force_variant, t.wave8_min_wgs) : old_fwd(B, T, heads, dropout != 0);
      const se::MhsaCall c{B, T, heads, prescaled != 0, dropout != 0};
      const se::MhsaRoute got = se::mhsa_route(c, t);
      const se::MhsaGrid g = se::mhsa_grid(got);
      ++calls;
      const int gi = static_cast<int>(got);
      bool ok = gi >= 0 && gi < 4;
      if (ok) ++per_route[gi];
      ok = ok && as_route(old.kernel) == got;                                               // 1
      ok = ok && (T + g.rows - 1) / g.rows == old.grid_x && g.threads == old.threads;       // 2
      ok = ok && se::mhsa_route_ok(got, c) == !old.failed;                                  // 3
      if (old.failed) {
        ++failed_calls;
        // and only for the two stated reasons
        const bool dma31 = got == se::MhsaRoute::Wave8Prescaled && !((double)T * 3.0 * (heads * 64) * 2.0 < 2147483648.0);
        const bool pair32 = got == se::MhsaRoute::Wave4Dropout && !((double)B * heads * T * ((T + 1) / 2) < 4294967296.0);
        ok = ok && (dma31 || pair32);
      }
      if (prescaled && t.force_variant < 0 && t.wave8_min_wgs == 768) {
        const long wgs8 = (long)((T + 255) / 256) * heads * B;
        if (wgs8 >= 767 && wgs8 <= 769) {
          ++at_wgs[wgs8 - 767];
          ok = ok && (got == se::MhsaRoute::Wave8Prescaled) == (wgs8 >= 768);
        }
      }
      if (!ok && ++bad <= 20)
        fprintf(stderr, "MISMATCH B=%d T=%d heads=%d prescaled=%d dropout=%d force=%d min_wgs=%d: route %d grid %d x %d, chain %d grid %d x %d failed %d\n", B, T,
                heads, prescaled, dropout, t.force_variant, t.wave8_min_wgs, gi, (T + g.rows - 1) / g.rows, g.threads, static_cast<int>(as_route(old.kernel)),
                old.grid_x, old.threads, (int)old.failed);
    }
  printf("calls %ld bad %ld routes", calls, bad);
  for (long n : per_route) printf(" %ld", n);
  printf(" failed %ld wgs767-769 %ld %ld %ld\n", failed_calls, at_wgs[0], at_wgs[1], at_wgs[2]);
  // a walk that never reaches a route, a failing call or one side of the threshold proves nothing about it
  for (long n : per_route)
    if (n == 0) return 2;
  if (failed_calls == 0 || at_wgs[0] == 0 || at_wgs[1] == 0 || at_wgs[2] == 0) return 2;
  return bad ? 1 : 0;
}
