// fftg_walk.cpp -- stand-alone host check of the general STFT plan's FFT core (csrc/fftg.h + csrc/fftg_plan.h, no HIP): for every length m it
// runs the scheduled Stockham transform, the real-transform post pass and the inverse pre-pass on random and impulse inputs and compares
// with a float64 direct DFT.  One line per m:
//   m <m> radices <r0>x<r1>... fft <e> rfft <e> inv <e> rinv <e>
// e = max |error| / max |exact| over both inputs:  fft  = complex forward transform of length m
//                                                   rfft = 2 m-point real transform (bins 0 .. m)
//                                                   inv  = ifft(fft(z)) against z
//                                                   rinv = real inverse (pre-pass + inverse transform) of the exact spectrum against x
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <complex>
#include <vector>

#include "fftg_plan.h"

using se::cf;
typedef std::complex<double> cd;

static double g_seed = 0.5;
static float rnd() {      // deterministic, in [-1, 1)
  g_seed = fmod(g_seed * 997.0 + 0.123456789, 1.0);
  return (float)(2.0 * g_seed - 1.0);
}

static std::vector<cd> dft(const std::vector<cd>& x, int dir) {
  const int n = (int)x.size();
  std::vector<cd> X(n);
  for (int k = 0; k < n; ++k) {
    cd acc = 0;
    for (int t = 0; t < n; ++t) acc += x[t] * std::polar(1.0, dir * 2.0 * M_PI * (double)((long long)k * t % n) / n);
    X[k] = acc;
  }
  return X;
}

struct Err { double fft = 0, rfft = 0, inv = 0, rinv = 0; };

static void upd(double* e, double err, double scale) { if (err / scale > *e) *e = err / scale; }

static void one_input(const se::FftgSchedule& sc, const std::vector<cf>& tw, const std::vector<cf>& rtw, const std::vector<float>& x, Err* e) {
  const int m = sc.m;
  auto nosync = [] {};
  std::vector<cf> a(m), b(m);
  std::vector<cd> z(m);
  for (int n = 0; n < m; ++n) {
    a[n] = se::cf_make(x[2 * n], x[2 * n + 1]);
    z[n] = cd(x[2 * n], x[2 * n + 1]);
  }
  // complex forward
  const cf* Z = se::fftg_run<-1>(sc, a.data(), b.data(), tw.data(), 0, 1, nosync);
  const std::vector<cd> Zr = dft(z, -1);
  double zmax = 0, zerr = 0;
  for (int k = 0; k < m; ++k) {
    zmax = fmax(zmax, std::abs(Zr[k]));
    zerr = fmax(zerr, std::abs(cd(Z[k].x, Z[k].y) - Zr[k]));
  }
  upd(&e->fft, zerr, zmax);
  // real transform of length 2 m: post pass
  std::vector<cd> xr(2 * m);
  for (int n = 0; n < 2 * m; ++n) xr[n] = x[n];
  const std::vector<cd> Xr = dft(xr, -1);
  std::vector<cf> X(m + 1);
  for (int k = 0; k <= m / 2; ++k) {
    cf xk, xn;
    se::fftg_post_pair(Z[k], Z[k == 0 ? 0 : m - k], rtw[k], &xk, &xn);
    X[k] = xk;
    if (2 * k != m) X[m - k] = xn;
  }
  double xmax = 0, xerr = 0;
  for (int k = 0; k <= m; ++k) {
    xmax = fmax(xmax, std::abs(Xr[k]));
    xerr = fmax(xerr, std::abs(cd(X[k].x, X[k].y) - Xr[k]));
  }
  upd(&e->rfft, xerr, xmax);
  // ifft(fft(z)) = z
  std::vector<cf> c(Z, Z + m), d(m);
  const cf* zi = se::fftg_run<+1>(sc, c.data(), d.data(), tw.data(), 0, 1, nosync);
  double smax = 0, ierr = 0;
  for (int n = 0; n < m; ++n) {
    smax = fmax(smax, std::abs(z[n]));
    ierr = fmax(ierr, std::abs(cd(zi[n].x / m, zi[n].y / m) - z[n]));
  }
  upd(&e->inv, ierr, smax);
  // real inverse from the EXACT spectrum (rounded to fp32): pre-pass + inverse transform
  std::vector<cf> P(m), Q(m);
  for (int k = 0; k <= m / 2; ++k) {
    cf xk = se::cf_make((float)Xr[k].real(), (float)Xr[k].imag());
    cf xn = se::cf_make((float)Xr[m - k].real(), (float)Xr[m - k].imag());
    if (k == 0) xk.y = xn.y = 0.f;
    cf zk, zn;
    se::fftg_pre_pair(xk, xn, rtw[k], &zk, &zn);
    P[k] = zk;
    if (k != 0) P[m - k] = zn;
  }
  const cf* xi = se::fftg_run<+1>(sc, P.data(), Q.data(), tw.data(), 0, 1, nosync);
  double rerr = 0;
  for (int n = 0; n < m; ++n) rerr = fmax(rerr, fmax(fabs(xi[n].x / m - x[2 * n]), fabs(xi[n].y / m - x[2 * n + 1])));
  upd(&e->rinv, rerr, smax);
}

int main() {
  const int sizes[] = {16, 18, 20, 30, 45, 100, 160, 200, 256, 375, 512};
  int bad = 0;
  for (int m : sizes) {
    se::FftgSchedule sc;
    if (!se::fftg_make_schedule(m, &sc)) { printf("m %d no schedule\n", m); bad = 1; continue; }
    std::vector<cf> tw(m), rtw(m);
    se::fftg_make_twiddles(m, tw.data(), rtw.data());
    Err e;
    std::vector<float> x(2 * m);
    for (auto& v : x) v = rnd();
    one_input(sc, tw, rtw, x, &e);
    for (int pos : {0, 1, m, 2 * m - 1}) {          // impulses: every output bin has magnitude 1
      for (auto& v : x) v = 0.f;
      x[pos] = 1.f;
      one_input(sc, tw, rtw, x, &e);
    }
    printf("m %d radices ", m);
    for (int s = 0; s < sc.n_stages; ++s) printf("%s%d", s ? "x" : "", sc.radix[s]);
    printf(" fft %.3e rfft %.3e inv %.3e rinv %.3e\n", e.fft, e.rfft, e.inv, e.rinv);
  }
  // geometry rules: one message per rule
  char why[256];
  const int rules[][5] = {{400, 160, 201, 40, 0}, {16, 8, 8, 40, 1}, {70, 35, 36, 40, 1}, {400, 160, 1025, 40, 2}, {600, 160, 257, 40, 3},
                          {400, 201, 201, 40, 4}, {400, 49, 201, 40, 5}, {400, 160, 201, 129, 6}};
  for (auto& r : rules) {
    const int got = se::fftg_check_geometry(r[0], r[1], r[2], r[3], why, sizeof(why));
    if (got != r[4]) { printf("rule mismatch win %d hop %d n_freq %d: %d != %d\n", r[0], r[1], r[2], got, r[4]); bad = 1; }
  }
  printf("rules %s\n", bad ? "bad" : "ok");
  return bad;
}
