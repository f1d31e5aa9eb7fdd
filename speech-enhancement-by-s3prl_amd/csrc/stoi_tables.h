// stoi_tables.h -- host side of the STOI / ESTOI plan (stoi.hip): the resampling taps in float64, the analysis window, the third-octave band
// edges and the counting rules (resampled length, frame count, compacted length).  Plain C++ in the manner of fftg_plan.h: includes only the
// C / C++ standard library and compiles without HIP (tests/stoi_walk.cpp).  The counting rules are marked __host__ __device__ under hipcc so that
// the kernels count exactly as the host does.
//
// Definition (the algorithm of pystoi.stoi as evaluation.py:28-36 calls it; parity unpinned vs pystoi):
//   resample  fs -> 10000 by the rational polyphase FIR of Octave's resample: p / q = 10000 / fs reduced, fc = 1 / (2 max(p, q)),
//             L = ceil((60 - 8) / (28.714 fc / 10)), h = kaiser(2 L + 1, 0.1102 (60 - 8.7)) 2 p fc sinc(2 fc t), t = -L .. L, g = p h / sum(h);
//             y[n] = sum_m x[m] g[n q - m p + L], n < ceil(len p / q)  (zero phase)
//   frames    256 samples at hop 128, window hanning(258)[1:-1], starts 0, 128, ... <= n - 256
//   bands     15 third-octave bands from 150 Hz over the one-sided 512-point spectrum
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define STOI_HD __host__ __device__ __forceinline__
#else
#define STOI_HD inline
#endif

namespace se {

constexpr int kStoiFs = 10000;
constexpr int kStoiFrame = 256;       // N_FRAME
constexpr int kStoiHop = 128;
constexpr int kStoiNfft = 512;
constexpr int kStoiBands = 15;
constexpr int kStoiMinFreq = 150;
constexpr int kStoiSeg = 30;          // N: frames per correlation segment
constexpr double kStoiBeta = -15.0;
constexpr double kStoiDynRange = 40.0;
constexpr double kStoiEps = 2.220446049250313e-16;      // 2^-52
constexpr float kStoiTooShort = 1e-5f;                  // fewer than kStoiSeg kept frames

// ---- counting rules
STOI_HD int64_t stoi_n10(int64_t len, int p, int q) { return len <= 0 ? 0 : (len * p + q - 1) / q; }                       // ceil(len p / q)
STOI_HD int64_t stoi_frames(int64_t n) { return n < kStoiFrame ? 0 : (n - kStoiFrame) / kStoiHop + 1; }                     // range(0, n - 256 + 1, 128)
STOI_HD int64_t stoi_compact_len(int64_t kept) { return kept <= 0 ? 0 : (kept - 1) * kStoiHop + kStoiFrame; }
STOI_HD int64_t stoi_segments(int64_t kept) { return kept < kStoiSeg ? 0 : kept - kStoiSeg + 1; }

// p / q = 10000 / fs reduced.  False unless fs is one of the supported rates (16000, 10000).
inline bool stoi_rate(int fs, int* p, int* q) {
  if (fs != 16000 && fs != kStoiFs) return false;
  int a = kStoiFs, b = fs;
  while (b) { const int t = a % b; a = b; b = t; }
  *p = kStoiFs / a;
  *q = fs / a;
  return true;
}

// modified Bessel function of the first kind, order 0 (power series; converges to float64 for the arguments of a Kaiser window)
inline double stoi_i0(double x) {
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// the 2 L + 1 taps g of the p / q resampler; returns L
inline int stoi_make_taps(int p, int q, std::vector<double>* g) {
  const double fc = 1.0 / (2.0 * (double)(p > q ? p : q));
  const int L = (int)ceil((60.0 - 8.0) / (28.714 * fc / 10.0));
  const double beta = 0.1102 * (60.0 - 8.7);
  const int M = 2 * L + 1;
  g->assign(M, 0.0);
  double sum = 0.0;
  for (int n = 0; n < M; ++n) {
    const double t = (double)(n - L);
    const double r = t / (double)L;
    const double kais = stoi_i0(beta * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / stoi_i0(beta);
    const double a = M_PI * 2.0 * fc * t;
    const double sinc = (n == L) ? 1.0 : sin(a) / a;
    (*g)[n] = kais * 2.0 * (double)p * fc * sinc;
    sum += (*g)[n];
  }
  for (int n = 0; n < M; ++n) (*g)[n] = (double)p * (*g)[n] / sum;
  return L;
}

// taps per polyphase branch: branch r holds g[r], g[r + p], ...
inline int stoi_branch_taps(int p, int L) { return (2 * L + p) / p; }      // ceil((2 L + 1) / p)

// w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257)), n < 256: hanning(258)[1:-1]
inline void stoi_make_window(double* w) {
  for (int n = 0; n < kStoiFrame; ++n) w[n] = 0.5 * (1.0 - cos(2.0 * M_PI * (double)(n + 1) / (double)(kStoiFrame + 1)));
}

// band b sums the bins lo[b] .. hi[b] - 1 of the 512-point spectrum: the bins nearest to 150 2^((2 b -+ 1) / 6) Hz (first minimum, as argmin)
inline void stoi_band_edges(int* lo, int* hi) {
  for (int b = 0; b < kStoiBands; ++b) {
    const double fl = (double)kStoiMinFreq * pow(2.0, (2.0 * b - 1.0) / 6.0), fh = (double)kStoiMinFreq * pow(2.0, (2.0 * b + 1.0) / 6.0);
    double bl = 1e300, bh = 1e300;
    for (int k = 0; k <= kStoiNfft / 2; ++k) {
      const double f = (double)k * (double)kStoiFs / (double)kStoiNfft;
      if ((f - fl) * (f - fl) < bl) { bl = (f - fl) * (f - fl); lo[b] = k; }
      if ((f - fh) * (f - fh) < bh) { bh = (f - fh) * (f - fh); hi[b] = k; }
    }
  }
}

}  // namespace se
