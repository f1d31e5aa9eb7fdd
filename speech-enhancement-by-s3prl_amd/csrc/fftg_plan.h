// fftg_plan.h -- host side of the general STFT plan: the supported-geometry rules, the radix schedule and the tables of fftg.h's transform,
// all in float64.  Host-only: includes the C library and fftg.h, compiles without HIP (tests/fftg_walk.cpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <initializer_list>

#include "fftg.h"

namespace se {

constexpr int kFftgMinM = 16, kFftgMaxM = 512;      // n_fft = 2 m: 32 ... 1024
constexpr int kFftgMaxMels = 128;

// The supported set of se_plan_create_any (include/se_amd.h).  Returns 0, or the number of the violated rule with its text in `why`.
inline int fftg_check_geometry(int win, int hop, int n_freq, int n_mels, char* why, size_t why_len) {
  const int m = n_freq - 1, n_fft = 2 * m;
  int rest = m < 1 ? 0 : m;
  for (int f : {2, 3, 5})
    while (rest > 1 && rest % f == 0) rest /= f;
  if (rest != 1) {
    snprintf(why, why_len, "m = n_freq - 1 = %d must be of the form 2^a 3^b 5^c (it has the factor %d)", m, rest);
    return 1;
  }
  if (m < kFftgMinM || m > kFftgMaxM) {
    snprintf(why, why_len, "n_fft = 2 (n_freq - 1) = %d must lie in [%d, %d]", n_fft, 2 * kFftgMinM, 2 * kFftgMaxM);
    return 2;
  }
  if (win < 2 || win > n_fft) {
    snprintf(why, why_len, "win = %d must lie in [2, n_fft = %d]", win, n_fft);
    return 3;
  }
  if (hop > win / 2) {
    snprintf(why, why_len, "hop = %d must not exceed win / 2 = %d (the Hann overlap-add envelope must not vanish)", hop, win / 2);
    return 4;
  }
  if (hop < (n_fft + 7) / 8) {
    snprintf(why, why_len, "hop = %d must be at least ceil(n_fft / 8) = %d (bounded overlap)", hop, (n_fft + 7) / 8);
    return 5;
  }
  if (n_mels < 1 || n_mels > kFftgMaxMels) {
    snprintf(why, why_len, "n_mels = %d must lie in [1, %d]", n_mels, kFftgMaxMels);
    return 6;
  }
  return 0;
}

// radices from {4, 2, 3, 5}: fours first (fewest stages), then the odd factors.  False if m has another prime factor.
inline bool fftg_make_schedule(int m, FftgSchedule* sc) {
  sc->m = m;
  sc->n_stages = 0;
  int rest = m;
  for (int r : {4, 2, 3, 5})
    while (rest % r == 0) {
      if (sc->n_stages == kFftgMaxStages) return false;
      sc->radix[sc->n_stages++] = r;
      rest /= r;
    }
  return rest == 1 && m > 1;
}

// tw[t] = (cos, sin)(2 pi t / m), t < m: the stage twiddles;  rtw[k] = (cos, sin)(2 pi k / (2 m)), k < m: the recombination twiddles
inline void fftg_make_twiddles(int m, cf* tw, cf* rtw) {
  for (int t = 0; t < m; ++t) {
    tw[t] = cf_make((float)cos(2.0 * M_PI * (double)t / (double)m), (float)sin(2.0 * M_PI * (double)t / (double)m));
    rtw[t] = cf_make((float)cos(M_PI * (double)t / (double)m), (float)sin(M_PI * (double)t / (double)m));
  }
}

// periodic Hann of length win, centred in n_fft (left pad (n_fft - win) / 2, as torch.stft pads a short window)
inline void fftg_make_window(int n_fft, int win, float* w) {
  for (int n = 0; n < n_fft; ++n) w[n] = 0.f;
  const int left = (n_fft - win) / 2;
  for (int n = 0; n < win; ++n) w[left + n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)win));
}

}  // namespace se
