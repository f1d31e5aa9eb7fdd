// fftg.h -- the FFT core of the general STFT / iSTFT kernels (stftg.hip, istftg.hip): a run-time-scheduled Stockham (autosort) mixed-radix
// complex FFT of length m = 2^a 3^b 5^c over a ping-pong pair of buffers the caller provides, plus the two passes that turn it into a
// 2 m-point real transform (post pass: Z -> X; pre-pass: X -> Z).
//
// Everything here is plain C++ marked __host__ __device__ under hipcc and unmarked under a host compiler: the identical arithmetic runs on
// LDS rows in the kernels and on plain arrays in tests/fftg_walk.cpp.  No HIP intrinsics, no includes beyond the C library.
//
// One stage of radix r at stride s (s = product of the radices of the stages before it, n = m / s the length still to transform):
//   work item i in [0, m / r):  p = i / s, q = i - p s
//   a_j = x[q + s (p + j n / r)]            j < r          (consecutive items read consecutive addresses)
//   b   = DFT_r(a)
//   y[q + s (r p + k)] = b_k W_m^(DIR p k s)               (W_n^(p k) = W_m^(p k s): ONE twiddle table of m entries serves every stage)
// After the last stage the result stands in natural order in the buffer written last.
#pragma once

#if defined(__HIPCC__)
#define FFTG_HD __host__ __device__ __forceinline__
#define FFTG_UNROLL _Pragma("unroll")
#else
#define FFTG_HD inline
#define FFTG_UNROLL
#endif

namespace se {

struct cf { float x, y; };      // complex fp32 (layout of float2)

constexpr int kFftgMaxStages = 9;      // 512 = 4^4 x 2: 5 stages; 486 = 2 x 3^5: 6

struct FftgSchedule {
  int m;
  int n_stages;
  int radix[kFftgMaxStages];
};

FFTG_HD cf cf_make(float x, float y) { cf r; r.x = x; r.y = y; return r; }
FFTG_HD cf cf_add(cf a, cf b) { return cf_make(a.x + b.x, a.y + b.y); }
FFTG_HD cf cf_sub(cf a, cf b) { return cf_make(a.x - b.x, a.y - b.y); }
FFTG_HD cf cf_mul(cf a, cf b) { return cf_make(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// multiplication by DIR i  (DIR = -1: the forward transform's -i)
template <int DIR>
FFTG_HD cf cf_muli(cf a) { return DIR < 0 ? cf_make(a.y, -a.x) : cf_make(-a.y, a.x); }
// tw holds (cos, sin)(2 pi t / m); the transform of direction DIR multiplies by exp(DIR i 2 pi t / m)
template <int DIR>
FFTG_HD cf cf_twiddle(cf a, cf w) { return DIR < 0 ? cf_make(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y) : cf_mul(a, w); }

template <int DIR>
FFTG_HD void fftg_bfly2(cf* v) {
  const cf a = v[0], b = v[1];
  v[0] = cf_add(a, b);
  v[1] = cf_sub(a, b);
}

template <int DIR>
FFTG_HD void fftg_bfly3(cf* v) {
  const float c = -0.5f, s = 0.86602540378443864676f;        // cos, sin of 2 pi / 3
  const cf t = cf_add(v[1], v[2]);
  const cf d = cf_muli<DIR>(cf_sub(v[1], v[2]));
  const cf e = cf_make(v[0].x + c * t.x, v[0].y + c * t.y);
  v[0] = cf_add(v[0], t);
  v[1] = cf_make(e.x + s * d.x, e.y + s * d.y);
  v[2] = cf_make(e.x - s * d.x, e.y - s * d.y);
}

template <int DIR>
FFTG_HD void fftg_bfly4(cf* v) {
  const cf a = cf_add(v[0], v[2]), b = cf_sub(v[0], v[2]);
  const cf c = cf_add(v[1], v[3]), d = cf_muli<DIR>(cf_sub(v[1], v[3]));
  v[0] = cf_add(a, c);
  v[1] = cf_add(b, d);
  v[2] = cf_sub(a, c);
  v[3] = cf_sub(b, d);
}

template <int DIR>
FFTG_HD void fftg_bfly5(cf* v) {
  const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;      // cos of 2 pi / 5, 4 pi / 5
  const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;       // sin of 2 pi / 5, 4 pi / 5
  const cf t1 = cf_add(v[1], v[4]), t2 = cf_add(v[2], v[3]);
  const cf d1 = cf_sub(v[1], v[4]), d2 = cf_sub(v[2], v[3]);
  const cf e1 = cf_make(v[0].x + c1 * t1.x + c2 * t2.x, v[0].y + c1 * t1.y + c2 * t2.y);
  const cf e2 = cf_make(v[0].x + c2 * t1.x + c1 * t2.x, v[0].y + c2 * t1.y + c1 * t2.y);
  const cf g1 = cf_muli<DIR>(cf_make(s1 * d1.x + s2 * d2.x, s1 * d1.y + s2 * d2.y));
  const cf g2 = cf_muli<DIR>(cf_make(s2 * d1.x - s1 * d2.x, s2 * d1.y - s1 * d2.y));
  v[0] = cf_add(v[0], cf_add(t1, t2));
  v[1] = cf_add(e1, g1);
  v[4] = cf_sub(e1, g1);
  v[2] = cf_add(e2, g2);
  v[3] = cf_sub(e2, g2);
}

template <int DIR, int R>
FFTG_HD void fftg_item_r(const cf* x, cf* y, const cf* tw, int m, int s, int i) {
  const int n1 = m / (s * R);
  const int p = i / s, q = i - p * s;
  cf v[R];
FFTG_UNROLL
  for (int j = 0; j < R; ++j) v[j] = x[q + s * (p + j * n1)];
  if (R == 2) fftg_bfly2<DIR>(v);
  if (R == 3) fftg_bfly3<DIR>(v);
  if (R == 4) fftg_bfly4<DIR>(v);
  if (R == 5) fftg_bfly5<DIR>(v);
  const int o = q + s * R * p;
  const int ts = p * s;                                   // twiddle index of k = 1; k ts < m
  y[o] = v[0];
FFTG_UNROLL
  for (int k = 1; k < R; ++k) y[o + s * k] = cf_twiddle<DIR>(v[k], tw[k * ts]);
}

// work item i (< m / r) of the stage with radix r at stride s
template <int DIR>
FFTG_HD void fftg_item(const cf* x, cf* y, const cf* tw, int m, int r, int s, int i) {
  switch (r) {
    case 2: fftg_item_r<DIR, 2>(x, y, tw, m, s, i); break;
    case 3: fftg_item_r<DIR, 3>(x, y, tw, m, s, i); break;
    case 4: fftg_item_r<DIR, 4>(x, y, tw, m, s, i); break;
    default: fftg_item_r<DIR, 5>(x, y, tw, m, s, i); break;
  }
}

// all stages over one buffer pair, work items i0, i0 + istep, ... of every stage (a host caller passes 0, 1; `sync` separates the stages).
// Returns the buffer that holds the result.
template <int DIR, typename Sync>
FFTG_HD cf* fftg_run(const FftgSchedule& sc, cf* a, cf* b, const cf* tw, int i0, int istep, Sync sync) {
  int s = 1;
  for (int st = 0; st < sc.n_stages; ++st) {
    const int r = sc.radix[st];
    for (int i = i0; i < sc.m / r; i += istep) fftg_item<DIR>(a, b, tw, sc.m, r, s, i);
    sync();
    cf* t = a; a = b; b = t;
    s *= r;
  }
  return a;
}

// ---- real transform of length 2 m through the m-point complex one.  rtw[k] = (cos, sin)(2 pi k / (2 m)), k <= m / 2.
// Forward post pass, pair k in [0, m / 2]: from Z = FFT_m(z), z[n] = x[2 n] + i x[2 n + 1], the bins X[k] and X[m - k] of the real
// transform (k = 0: X[0] and the Nyquist bin X[m]; 2 k = m: both are the same bin).
FFTG_HD void fftg_post_pair(cf zk, cf zn, cf w, cf* xk, cf* xn) {
  // E = (zk + conj(zn)) / 2 ; O = (zk - conj(zn)) / (2 i) ; P = W^k O, W^k = (c, -s)
  const cf E = cf_make(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
  const cf O = cf_make(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
  const cf P = cf_make(O.x * w.x + O.y * w.y, O.y * w.x - O.x * w.y);
  *xk = cf_make(E.x + P.x, E.y + P.y);            // X[k]
  *xn = cf_make(E.x - P.x, -(E.y - P.y));         // X[m - k] = conj(E - P)
}

// Inverse pre-pass, pair k in [0, m / 2]: from X[k], X[m - k] the entries Z[k], Z[m - k] with IFFT_m(Z)[n] = m (x[2 n] + i x[2 n + 1])
// (the 1 / m rides in the window).  The caller zeroes Im X[0] and Im X[m] (c2r semantics); for k = 0 *zn has no slot and is dropped.
FFTG_HD void fftg_pre_pair(cf xk, cf xn, cf w, cf* zk, cf* zn) {
  const cf E = cf_make(0.5f * (xk.x + xn.x), 0.5f * (xk.y - xn.y));
  const cf D = cf_make(0.5f * (xk.x - xn.x), 0.5f * (xk.y + xn.y));
  const cf O = cf_make(D.x * w.x - D.y * w.y, D.x * w.y + D.y * w.x);      // W^-k = (c, +s)
  *zk = cf_make(E.x - O.y, E.y + O.x);            // E + i O
  *zn = cf_make(E.x + O.y, O.x - E.y);            // conj(E) + i conj(O)
}

}  // namespace se
