// stoi_walk.cpp -- stand-alone host program over csrc/stoi_tables.h (built by tests/test_stoi_host.py with -Wall -Werror and the address /
// undefined-behaviour sanitizers): prints the resampler's taps, the window, the band edges and the counting rules for the test to compare with
// the numpy restatement (tests/stoi_ref.py).
#include "stoi_tables.h"

#include <stdio.h>

int main() {
  for (int fs : {16000, 10000, 8000, 44100}) {
    int p = 0, q = 0;
    const bool ok = se::stoi_rate(fs, &p, &q);
    printf("rate %d ok %d p %d q %d\n", fs, ok ? 1 : 0, ok ? p : 0, ok ? q : 0);
  }
  std::vector<double> g;
  const int L = se::stoi_make_taps(5, 8, &g);
  double sum = 0.0;
  for (double v : g) sum += v;
  printf("taps L %d n %zu sum %.17g centre %.17g branch %d\n", L, g.size(), sum, g[L], se::stoi_branch_taps(5, L));
  for (int r = 0; r < 5; ++r) {
    double s = 0.0;
    for (size_t i = r; i < g.size(); i += 5) s += g[i];
    printf("phase %d %.17g\n", r, s);
  }
  for (int i : {0, 1, 37, 145, 289, 291, 580}) printf("tap %d %.17g\n", i, g[i]);
  double w[se::kStoiFrame];
  se::stoi_make_window(w);
  for (int i : {0, 1, 127, 128, 255}) printf("win %d %.17g\n", i, w[i]);
  int lo[se::kStoiBands], hi[se::kStoiBands];
  se::stoi_band_edges(lo, hi);
  printf("lo");
  for (int b = 0; b < se::kStoiBands; ++b) printf(" %d", lo[b]);
  printf("\nhi");
  for (int b = 0; b < se::kStoiBands; ++b) printf(" %d", hi[b]);
  printf("\n");
  for (long long len : {-3ll, 0ll, 1ll, 255ll, 408ll, 409ll, 410ll, 4800ll, 9001ll, 16000ll, 64000ll, 160000ll}) {
    const long long n16 = (long long)se::stoi_n10(len, 5, 8), n1 = (long long)se::stoi_n10(len, 1, 1);
    printf("count %lld n10 %lld frames %lld n10_same %lld frames_same %lld\n", len, n16, (long long)se::stoi_frames(n16), n1,
           (long long)se::stoi_frames(n1));
  }
  for (long long k : {0ll, 1ll, 29ll, 30ll, 311ll})
    printf("kept %lld compact %lld segments %lld\n", k, (long long)se::stoi_compact_len(k), (long long)se::stoi_segments(k));
  return 0;
}
