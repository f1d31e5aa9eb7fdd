// stoi_bwd.hip -- the gradient of STOI / ESTOI (stoi.hip) in the processed signal, for training a head against the metric evaluate() reports
// (the reference's objective.py:16-45 declares `stoi` / `estoi` criteria on wav_predicted; parity unpinned vs asteroid / torch_stoi).  The
// keep mask, the kept-index list and the clean envelopes depend on the clean signal alone: constants of the differentiation.  One
// se_stoi_grad_f32 call runs the forward's launches (se_stoi_f32 itself: stoi_out is bit-identical) and then, all asynchronous on `stream`, no
// allocation, no host sync, no atomics (every scatter of the adjoint is written as a gather or as a fixed-order fold through the workspace):
//   score_bwd  one wave per (utterance, segment), lane <-> frame as stoi_score_kernel, fp64: the exact derivative of that kernel's arithmetic
//              (every + EPS kept; min(c y, x clip) passes the gradient through the branch taken; the scale c is differentiated through |y|;
//              ESTOI rows / columns with s <= 0 contribute 0) -> dseg (B, Jmax, 15, 30)
//   ge_fold    gE[b, r, col] = grad_scale / (J norm) sum over the <= 30 segments that contain col, ascending -> (B, 15, Fmax) fp32
//   inv        the inverse of kept_idx: source frame -> compact position or -1
//   bands_bwd  per (utterance, four compacted frames): the processed spectrum recomputed exactly as stoi_bands_kernel does, G = (gE / E) Y per
//              band (0 where E == 0 and outside the bands), gv[n] = Re sum_k G_k e^{+2 pi i k n / 512} by fftg.h's pre-pass + m = 256 complex
//              FFT with DIR = +1 (one-sided bins are independent outputs: no doubling), windowed -> gt (B, Fmax, 256)
//   gather     gy10[n] = sum over the <= 2 kept source frames that cover n of w (gt_k + the half of gt_{k -+ 1} that overlaps), w again.
//              At 10 kHz this writes grad itself.
//   resample^T gy[m] = sum_n gy10[n] g[n q - m p + L]: polyphase by the branch (L - m p) mod q of m, taps (q-branch-major) and the gy10 tile in
//              LDS, fp64 sums, 256 outputs per workgroup
// grad[b, m] is exactly 0 for m >= lengths[b], and the whole row for an utterance with fewer than 30 kept frames.
#include <math.h>
#include "common.h"
#include "fftg.h"
#include "stoi_dev.h"

namespace se {

constexpr int kStoiBwdOut = 256;                       // outputs per workgroup of the resampler adjoint

// dseg (B, Jmax, 15, 30) fp64: d (segment sum of stoi_score_kernel) / d (processed envelope) of the segment's 15 x 30 block
__global__ __launch_bounds__(256) void stoi_score_bwd_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int B, int Fmax, int Jmax,
                                                             int extended, double* __restrict__ dseg) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x * 4 + wave;
  const int J = (int)stoi_segments(kept[b]);
  if (seg >= J) return;                                   // wave-uniform
  const bool act = lane < kStoiSeg;
  double x[kStoiBands], y[kStoiBands], g[kStoiBands];
#pragma unroll
  for (int r = 0; r < kStoiBands; ++r) {
    const size_t o = (size_t)r * Fmax + seg + (act ? lane : 0);
    x[r] = act ? (double)tob[((size_t)b * kStoiBands) * Fmax + o] : 0.0;
    y[r] = act ? (double)tob[(((size_t)B + b) * kStoiBands) * Fmax + o] : 0.0;
  }
  const double inv_n = 1.0 / (double)kStoiSeg;
  if (!extended) {
    const double clip = 1.0 + pow(10.0, -kStoiBeta / 20.0);
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {
      // forward, as stoi_score_kernel
      const double nx = sqrt(wave_sum(x[r] * x[r])), ny = sqrt(wave_sum(y[r] * y[r]));
      const double c = nx / (ny + kStoiEps);
      const double a = c * y[r], cl = x[r] * clip;
      const bool take = !(cl < a);                          // fmin(a, cl) returned a
      const double yp = fmin(a, cl);
      const double mx = wave_sum(x[r]) * inv_n, my = wave_sum(yp) * inv_n;
      const double xc = act ? x[r] - mx : 0.0, yc = act ? yp - my : 0.0;
      const double nxc = sqrt(wave_sum(xc * xc)), nyc = sqrt(wave_sum(yc * yc));
      const double xn = xc / (nxc + kStoiEps);
      // u = yc / (nyc + EPS), value = sum u xn
      const double d = nyc + kStoiEps;
      const double s1 = wave_sum(xn * yc);
      const double g_yc = act ? xn / d - (nyc > 0.0 ? yc * s1 / (d * d * nyc) : 0.0) : 0.0;
      const double m_yc = wave_sum(g_yc) * inv_n;             // every wave sum stands outside the `act` selects: all 64 lanes take part
      const double g_yp = act ? g_yc - m_yc : 0.0;
      const double g_a = take ? g_yp : 0.0;
      // a = c y, c = nx / (ny + EPS): d c / d y = -nx y / ((ny + EPS)^2 ny)
      const double s2 = wave_sum(g_a * y[r]);
      const double dn = ny + kStoiEps;
      g[r] = act ? c * g_a - (ny > 0.0 ? nx * y[r] * s2 / (dn * dn * ny) : 0.0) : 0.0;
    }
  } else {
    double rs[kStoiBands];                                  // 1 / sqrt(sy) of the row, 0 where sy <= 0
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {                 // rows, as stoi_score_kernel; y[r] becomes the normalised row
      const double mx = wave_sum(x[r]) * inv_n, my = wave_sum(y[r]) * inv_n;
      const double xc = act ? x[r] - mx : 0.0, yc = act ? y[r] - my : 0.0;
      const double sx = wave_sum(xc * xc), sy = wave_sum(yc * yc);
      x[r] = sx > 0.0 ? xc / sqrt(sx) : 0.0;
      y[r] = sy > 0.0 ? yc / sqrt(sy) : 0.0;
      rs[r] = sy > 0.0 ? 1.0 / sqrt(sy) : 0.0;
    }
    double mx = 0.0, my = 0.0;                             // columns: in-lane over the 15 bands
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) { mx += x[r]; my += y[r]; }
    mx /= (double)kStoiBands;
    my /= (double)kStoiBands;
    double sx = 0.0, sy = 0.0, dot = 0.0;
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {
      const double xc = x[r] - mx, yc = y[r] - my;
      sx += xc * xc;
      sy += yc * yc;
      dot += xc * yc;
    }
    const bool valid = act && sx > 0.0 && sy > 0.0;
    const double rx = valid ? 1.0 / (sqrt(sx) * sqrt(sy)) : 0.0;       // value = dot rx
    const double ry = valid ? dot * rx / sy : 0.0;
    double gm = 0.0;
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {                 // d value / d (centred column)
      g[r] = (x[r] - mx) * rx - (y[r] - my) * ry;
      gm += g[r];
    }
    gm /= (double)kStoiBands;
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {                 // through the column mean, then the row's normalisation and mean
      const double g_yr = g[r] - gm;
      const double t = wave_sum(g_yr * y[r]);
      const double g_yc = act ? (g_yr - y[r] * t) * rs[r] : 0.0;
      const double m_yc = wave_sum(g_yc) * inv_n;
      g[r] = act ? g_yc - m_yc : 0.0;
    }
  }
  if (act) {
    double* o = dseg + (((size_t)b * Jmax + seg) * kStoiBands) * kStoiSeg + lane;
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) o[(size_t)r * kStoiSeg] = g[r];
  }
}

// gE (B, 15, Fmax) fp32 = grad_scale d stoi_b / d (processed envelope): the segments [col - 29, col] that exist, summed in ascending order
__global__ __launch_bounds__(256) void stoi_ge_fold_kernel(const double* __restrict__ dseg, const int* __restrict__ kept, int Fmax, int Jmax,
                                                           int extended, float grad_scale, float* __restrict__ gE) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= kStoiBands * Fmax) return;
  const int r = idx / Fmax, col = idx - r * Fmax;
  const int K = kept[b];
  const int J = (int)stoi_segments(K);
  float v = 0.f;
  if (J > 0 && col < K) {
    const int s_lo = max(0, col - (kStoiSeg - 1)), s_hi = min(J - 1, col);
    double a = 0.0;
    for (int s = s_lo; s <= s_hi; ++s) a += dseg[(((size_t)b * Jmax + s) * kStoiBands + r) * kStoiSeg + (col - s)];
    v = (float)(a * ((double)grad_scale / ((double)J * (double)(extended ? kStoiSeg : kStoiBands))));
  }
  gE[((size_t)b * kStoiBands + r) * Fmax + col] = v;
}

// inv (B, Fmax): compact position of every source frame, -1 for a dropped one.  One workgroup per utterance: kept_idx has no duplicates.
__global__ __launch_bounds__(256) void stoi_inv_kernel(const int* __restrict__ kept_idx, const int* __restrict__ kept, int Fmax, int* __restrict__ inv) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = kept[b];
  for (int i = tid; i < Fmax; i += 256) inv[(size_t)b * Fmax + i] = -1;
  __syncthreads();
  for (int k = tid; k < K; k += 256) inv[(size_t)b * Fmax + kept_idx[(size_t)b * Fmax + k]] = k;
}

// gt (B, Fmax, 256): w[t] gv_j[t], the gradient in the windowed compacted frame j < kept[b] (rows from kept[b] on are not written and not read)
__global__ __launch_bounds__(256) void stoi_bands_bwd_kernel(const float* __restrict__ ys, size_t ldx, const int* __restrict__ kept_idx,
                                                             const int* __restrict__ kept, int B, int Fmax, const float* __restrict__ window,
                                                             const cf* __restrict__ g_tw, const cf* __restrict__ g_rtw, FftgSchedule sched,
                                                             StoiBands bands, const float* __restrict__ tob, const float* __restrict__ gE,
                                                             float* __restrict__ gt) {
  __shared__ __attribute__((aligned(16))) cf bufA[kStoiFr * kStoiRow];
  __shared__ __attribute__((aligned(16))) cf bufB[kStoiFr * kStoiRow];
  __shared__ cf tw[kStoiM], rtw[kStoiM];
  __shared__ float win[kStoiFrame];
  __shared__ float coef[kStoiFr * kStoiPlane];              // gE / E of the bin's band, per frame; bins 0 .. 256
  __shared__ int s_idx[kStoiFr + 2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int j0 = blockIdx.x * kStoiFr;
  const int K = kept[b];
  if (K < kStoiSeg) return;                                 // workgroup-uniform: constant score, the gather writes zeros
  const int nf = min(kStoiFr, K - j0);
  if (nf <= 0) return;                                      // workgroup-uniform
  if (tid < kStoiFr + 2) {
    const int kk = j0 - 1 + tid;
    s_idx[tid] = (kk >= 0 && kk < K) ? kept_idx[(size_t)b * Fmax + kk] : -1;
  }
  for (int i = tid; i < kStoiM; i += 256) { tw[i] = g_tw[i]; rtw[i] = g_rtw[i]; }
  for (int i = tid; i < kStoiFrame; i += 256) win[i] = window[i];
  for (int i = tid; i < kStoiFr * kStoiPlane; i += 256) coef[i] = 0.f;
  __syncthreads();
  for (int it = tid; it < nf * kStoiBands; it += 256) {      // the bands are disjoint: every coef entry has one writer
    const int f = it / kStoiBands, band = it - f * kStoiBands;
    const size_t o = ((size_t)b * kStoiBands + band) * Fmax + j0 + f;
    const float E = tob[(size_t)B * kStoiBands * Fmax + o];
    const float cv = E > 0.f ? gE[o] / E : 0.f;
    for (int k = bands.lo[band]; k < bands.hi[band]; ++k) coef[f * kStoiPlane + k] = cv;
  }

  // ---- fill, as stoi_bands_kernel for the processed signal: transform tr = f
  for (int it = tid; it < nf * kStoiM; it += 256) {
    const int f = it / kStoiM, n = it - f * kStoiM;
    cf z = cf_make(0.f, 0.f);
    if (n < kStoiFrame / 2) {
      const float* s = ys + (size_t)b * ldx;
      const int ic = s_idx[f + 1];
      const int pa = 2 * n;
      const bool first = pa < kStoiHop;
      const int in = first ? s_idx[f] : s_idx[f + 2];
      const int sh = first ? kStoiHop : -kStoiHop;
      const float* sc = s + (size_t)ic * kStoiHop + pa;
      float v0 = win[pa] * sc[0], v1 = win[pa + 1] * sc[1];
      if (in >= 0) {
        const float* sn = s + (size_t)in * kStoiHop + pa + sh;
        v0 += win[pa + sh] * sn[0];
        v1 += win[pa + sh + 1] * sn[1];
      }
      z = cf_make(win[pa] * v0, win[pa + 1] * v1);
    }
    bufA[f * kStoiRow + n] = z;
  }
  __syncthreads();

  // ---- forward stages
  cf* src = bufA;
  cf* dst = bufB;
  {
    int s = 1;
    for (int st = 0; st < sched.n_stages; ++st) {
      const int r = sched.radix[st];
      const int per = kStoiM / r;
      for (int it = tid; it < nf * per; it += 256) {
        const int f = it / per, i = it - f * per;
        fftg_item<-1>(src + f * kStoiRow, dst + f * kStoiRow, tw, kStoiM, r, s, i);
      }
      __syncthreads();
      cf* t = src; src = dst; dst = t;
      s *= r;
    }
  }

  // ---- post pass (Z -> Y[k], Y[256 - k]), scale by the band's gE / E, pre-pass of the inverse into the other buffer.  The inverse of fftg.h
  //      returns half the two-sided sum: with X = G on bins 1 .. 255 that is Re sum G_k e^{+...}; the two real end bins count twice for it
  {
    const int pairs = kStoiM / 2 + 1;
    for (int it = tid; it < nf * pairs; it += 256) {
      const int f = it / pairs, k = it - f * pairs;
      const cf* Z = src + f * kStoiRow;
      cf X1, X2;
      fftg_post_pair(Z[k], Z[k == 0 ? 0 : kStoiM - k], rtw[k], &X1, &X2);
      const float c1 = coef[f * kStoiPlane + k], c2 = coef[f * kStoiPlane + kStoiM - k];
      cf G1 = cf_make(c1 * X1.x, c1 * X1.y), G2 = cf_make(c2 * X2.x, c2 * X2.y);
      if (k == 0) { G1 = cf_make(2.f * G1.x, 0.f); G2 = cf_make(2.f * G2.x, 0.f); }
      cf zk, zn;
      fftg_pre_pair(G1, G2, rtw[k], &zk, &zn);
      cf* D = dst + f * kStoiRow;
      D[k] = zk;
      if (k != 0) D[kStoiM - k] = zn;
    }
  }
  __syncthreads();
  { cf* t = src; src = dst; dst = t; }

  // ---- inverse stages
  {
    int s = 1;
    for (int st = 0; st < sched.n_stages; ++st) {
      const int r = sched.radix[st];
      const int per = kStoiM / r;
      for (int it = tid; it < nf * per; it += 256) {
        const int f = it / per, i = it - f * per;
        fftg_item<+1>(src + f * kStoiRow, dst + f * kStoiRow, tw, kStoiM, r, s, i);
      }
      __syncthreads();
      cf* t = src; src = dst; dst = t;
      s *= r;
    }
  }

  // ---- window: row f holds gv[0 .. 512) as 512 reals; the zero padding drops n >= 256
  for (int it = tid; it < nf * kStoiFrame; it += 256) {
    const int f = it / kStoiFrame, t = it - f * kStoiFrame;
    const float* xr = reinterpret_cast<const float*>(src + f * kStoiRow);
    gt[((size_t)b * Fmax + j0 + f) * kStoiFrame + t] = win[t] * xr[t];
  }
}

// out (B, ldo): the gradient in the 10 kHz signal.  Sample n is covered by the source frames n / 128 - 1 and n / 128; kept frame k received
// gc[128 k + t] = gt_k[t] + (t < 128 ? gt_{k-1}[t + 128] : gt_{k+1}[t - 128]).  Columns from the utterance's 10 kHz length on are zero.
__global__ __launch_bounds__(256) void stoi_gather_kernel(const float* __restrict__ gt, const int* __restrict__ inv, const int* __restrict__ kept,
                                                          const int64_t* __restrict__ lengths, int T, int p, int q, int Fmax,
                                                          const float* __restrict__ window, int ldo, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= ldo) return;
  const int K = kept[b];
  const int n10 = (int)stoi_n10(stoi_len(lengths, b, T), p, q);
  const int F = (int)stoi_frames(n10);
  float v = 0.f;
  if (K >= kStoiSeg && n < n10) {
    const int i1 = n / kStoiHop;
#pragma unroll
    for (int d = 1; d >= 0; --d) {                          // fixed order: the earlier frame first
      const int i = i1 - d;
      if (i < 0 || i >= F) continue;
      const int k = inv[(size_t)b * Fmax + i];
      if (k < 0) continue;
      const int t = n - i * kStoiHop;
      const float* gk = gt + ((size_t)b * Fmax + k) * kStoiFrame;
      float gc = gk[t];
      if (t < kStoiHop) { if (k > 0) gc += gk[t + kStoiHop - kStoiFrame]; }             // gt_{k-1}[t + 128]
      else if (k + 1 < K) gc += gk[kStoiFrame + t - kStoiHop];                           // gt_{k+1}[t - 128]
      v += window[t] * gc;
    }
  }
  out[(size_t)b * ldo + n] = v;
}

// grad (B, ld): grad[m] = sum_n gy10[n] g[n q - m p + L] over 0 <= n < n10, m < len; zero from len out to ld.  For one m the tap index
// runs over s, s + q, ... with s = (L - m p) mod q: branch s of the taps laid out [q][NTq] in LDS.
__global__ __launch_bounds__(kStoiBwdOut) void stoi_resample_adj_kernel(const float* __restrict__ gy10, int n10max, const int* __restrict__ kept,
                                                                        const int64_t* __restrict__ lengths, int T, int p, int q, int L, int NT,
                                                                        int NTq, int tileN, const float* __restrict__ taps, int ld,
                                                                        float* __restrict__ grad) {
  extern __shared__ __attribute__((aligned(16))) float ra_smem[];
  float* tile = ra_smem;               // [tileN]
  float* gq = ra_smem + tileN;         // [q][NTq]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * kStoiBwdOut, m = m0 + tid;
  const int64_t len = stoi_len(lengths, b, T);
  if (m0 >= len || kept[b] < kStoiSeg) {          // workgroup-uniform: nothing but zero fill
    if (m < ld) grad[(size_t)b * ld + m] = 0.f;
    return;
  }
  const int n10 = (int)stoi_n10(len, p, q);
  const int a0 = m0 * p - L;
  const int n_base = a0 >= 0 ? (a0 + q - 1) / q : -((-a0) / q);       // ceil(a0 / q): the first n of output m0
  const float* src = gy10 + (size_t)b * n10max;
  for (int i = tid; i < tileN; i += kStoiBwdOut) {
    const int n = n_base + i;
    tile[i] = (n >= 0 && n < n10) ? src[n] : 0.f;
  }
  for (int i = tid; i < q * NTq; i += kStoiBwdOut) {
    const int s = i / NTq, j = s + q * (i - s * NTq);                  // tap index
    gq[i] = j <= 2 * L ? taps[(j % p) * NT + j / p] : 0.f;
  }
  __syncthreads();
  if (m >= ld) return;
  float v = 0.f;
  if (m < len) {
    const int a = m * p - L;
    const int n_lo = a >= 0 ? (a + q - 1) / q : -((-a) / q);           // ceil(a / q)
    const int s = n_lo * q - a;                                        // in [0, q)
    const int jn = (2 * L - s) / q + 1;                                // taps of branch s (<= NTq)
    const float* g = gq + s * NTq;
    const float* t = tile + (n_lo - n_base);
    double acc = 0.0;
    for (int j = 0; j < jn; ++j) acc += (double)t[j] * (double)g[j];
    v = (float)acc;
  }
  grad[(size_t)b * ld + m] = v;
}

struct StoiGradLayout {
  StoiLayout f;
  int Jmax;
  size_t o_dseg, o_ge, o_gt, o_inv, o_gy10, total;
};

inline StoiGradLayout stoi_grad_layout(const se_stoi_plan* plan, int B, int T) {
  StoiGradLayout l;
  l.f = stoi_layout(plan, B, T);
  l.Jmax = (int)stoi_segments(l.f.Fmax);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t BF = (size_t)B * (size_t)l.f.Fmax;
  l.o_dseg = l.f.total;
  l.o_ge = l.o_dseg + al((size_t)8 * B * (size_t)l.Jmax * kStoiBands * kStoiSeg);
  l.o_gt = l.o_ge + al((size_t)4 * kStoiBands * BF);
  l.o_inv = l.o_gt + al((size_t)4 * kStoiFrame * BF);
  l.o_gy10 = l.o_inv + al(4 * BF);
  l.total = l.o_gy10 + (plan->d_taps ? al((size_t)4 * B * (size_t)l.f.n10max) : 0);
  return l;
}

}  // namespace se

extern "C" size_t se_stoi_grad_workspace_bytes(const se_stoi_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T <= 0) return 0;
  return se::stoi_grad_layout(plan, B, T).total;
}

extern "C" int se_stoi_grad_f32(const se_stoi_plan* plan, const float* clean, const float* processed, int ld, const int64_t* lengths, int B, int T,
                                int extended, float grad_scale, float* stoi_out, float* grad, void* workspace, size_t workspace_bytes,
                                void* stream) {
  SE_REQUIRE(plan && clean && processed && stoi_out && grad, "se_stoi_grad_f32: null argument");
  SE_REQUIRE(B > 0 && B <= 65535 && T > 0 && ld >= T, "se_stoi_grad_f32: bad shape (B=%d T=%d ld=%d)", B, T, ld);
  SE_REQUIRE((long long)ld * (plan->p > plan->q ? plan->p : plan->q) + 2ll * plan->L < (1ll << 31), "se_stoi_grad_f32: ld=%d too long", ld);
  const se::StoiGradLayout l = se::stoi_grad_layout(plan, B, T);
  SE_REQUIRE(workspace && workspace_bytes >= l.total, "se_stoi_grad_f32: workspace of %zu bytes, %zu needed (se_stoi_grad_workspace_bytes)",
             workspace_bytes, l.total);
  // the forward: its own entry point on the leading part of the workspace, which it lays out as se_stoi_layout does
  const int rc = se_stoi_f32(plan, clean, processed, ld, lengths, B, T, extended, stoi_out, nullptr, nullptr, workspace, l.f.total, stream);
  if (rc != SE_OK) return rc;
  hipStream_t st = se::as_stream(stream);
  const int Fmax = l.f.Fmax, p = plan->p, q = plan->q;
  if (Fmax < se::kStoiSeg)        // no utterance of T samples can keep 30 frames: every score is the constant
    return se::zero_async(grad, sizeof(float) * (size_t)B * (size_t)ld, st);
  char* ws = (char*)workspace;
  const float* tob = (const float*)(ws + l.f.o_tob);
  const int* kept_idx = (const int*)(ws + l.f.o_idx);
  const int* kept = (const int*)(ws + l.f.o_kept);
  double* dseg = (double*)(ws + l.o_dseg);
  float* gE = (float*)(ws + l.o_ge);
  float* gt = (float*)(ws + l.o_gt);
  int* inv = (int*)(ws + l.o_inv);
  float* gy10 = (float*)(ws + l.o_gy10);
  const float* ys = processed;
  size_t ldx = (size_t)ld;
  if (plan->d_taps) {
    ys = (const float*)(ws + l.f.o_xr) + (size_t)B * (size_t)l.f.n10max;
    ldx = (size_t)l.f.n10max;
  }

  hipLaunchKernelGGL(se::stoi_score_bwd_kernel, dim3((l.Jmax + 3) / 4, B), dim3(256), 0, st, tob, kept, B, Fmax, l.Jmax, extended, dseg);
  SE_LAUNCH_CHECK();
  hipLaunchKernelGGL(se::stoi_ge_fold_kernel, dim3((se::kStoiBands * Fmax + 255) / 256, B), dim3(256), 0, st, dseg, kept, Fmax, l.Jmax, extended,
                     grad_scale, gE);
  SE_LAUNCH_CHECK();
  hipLaunchKernelGGL(se::stoi_inv_kernel, dim3(B), dim3(256), 0, st, kept_idx, kept, Fmax, inv);
  SE_LAUNCH_CHECK();
  se::StoiBands bands;
  for (int i = 0; i < se::kStoiBands; ++i) { bands.lo[i] = plan->lo[i]; bands.hi[i] = plan->hi[i]; }
  hipLaunchKernelGGL(se::stoi_bands_bwd_kernel, dim3((Fmax + se::kStoiFr - 1) / se::kStoiFr, B), dim3(256), 0, st, ys, ldx, kept_idx, kept, B, Fmax,
                     plan->d_window, plan->d_tw, plan->d_rtw, plan->sched, bands, tob, gE, gt);
  SE_LAUNCH_CHECK();
  if (!plan->d_taps) {            // 10 kHz: y10 is the input itself
    hipLaunchKernelGGL(se::stoi_gather_kernel, dim3((ld + 255) / 256, B), dim3(256), 0, st, gt, inv, kept, lengths, T, p, q, Fmax, plan->d_window, ld,
                       grad);
    SE_LAUNCH_CHECK();
    return SE_OK;
  }
  hipLaunchKernelGGL(se::stoi_gather_kernel, dim3((l.f.n10max + 255) / 256, B), dim3(256), 0, st, gt, inv, kept, lengths, T, p, q, Fmax,
                     plan->d_window, l.f.n10max, gy10);
  SE_LAUNCH_CHECK();
  const int NTq = (2 * plan->L + q) / q;                                                    // ceil((2 L + 1) / q)
  const int tileN = ((se::kStoiBwdOut - 1) * p + 2 * plan->L) / q + 3;
  const size_t lds = sizeof(float) * ((size_t)tileN + (size_t)q * NTq);
  hipLaunchKernelGGL(se::stoi_resample_adj_kernel, dim3((ld + se::kStoiBwdOut - 1) / se::kStoiBwdOut, B), dim3(se::kStoiBwdOut), lds, st, gy10,
                     l.f.n10max, kept, lengths, T, p, q, plan->L, plan->NT, NTq, tileN, plan->d_taps, ld, grad);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
