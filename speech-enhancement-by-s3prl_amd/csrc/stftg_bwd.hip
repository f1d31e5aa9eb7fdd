// stftg_bwd.hip -- the adjoint of rows A1 + A2 as stftg.hip computes them (reflect padding of m = n_fft / 2, window, one-sided n_fft-point real
// transform) for BOTH plan kinds: d loss / d power and / or d loss / d (re, im) -> d loss / d wav.  With G = grad_complx + 2 grad_power X:
//   gy_f[n]     = Re sum_{k <= m} G_{f,k} e^{+2 pi i k n / N}      no doubling of the inner bins; Im G at k in {0, m} contributes nothing
//                 (a c2r transform of G_k / c_k, c_k = 1 at {0, m}, 2 elsewhere, times N: fftg.h with DIR = +1, as istftg.hip)
//   gpad[p]     = sum_f w[p - hop f] gy_f[p - hop f]               0 <= p < T + 2 m: overlap-add, NO envelope division
//   grad_wav[n] = gpad[n + m] + [1 <= n <= m] gpad[m - n] + [T - 1 - m <= n <= T - 2] gpad[2 (T - 1) + m - n]      the fold of the reflect padding
//
// Structured like istftg_kernel: a workgroup (256 threads) owns HB hop-blocks of gpad of one utterance and inverse-transforms the FRI = HB + halo
// frames that reach into that span (halo = floor((n_fft - 1) / hop) frames start before it; recomputed by the neighbours, re-read from L2):
//   pre    : one item = the bin PAIR (k, m - k) of a frame.  The global loads of kPreBatch items per thread are issued back to back, then
//            G -> Z[k], Z[m - k] (fftg_pre_pair) into LDS.  Loads only in this loop.
//   stages : fftg.h with DIR = +1, ping-pong in dynamic LDS
//   ola    : gpad[p] over the frames f in [0, F) that contain p; LDS reads and global STORES only.  m <= p < T + m goes straight to
//            grad_wav[p - m]; the 2 m samples of the two pads go to the workspace (B, 2 m)
// A second small launch (one workgroup per utterance) folds the pads into grad_wav -- one thread per sample, left fold before right fold -- and
// zero-fills [T, wav_stride).  Every workspace word it reads was written by the first launch of the same call.  No atomics, no allocation:
// repeats are bit-identical.  LDS 16 bufN + 24 m bytes, <= 48 KB unless the halo asks for more (plan.h: stftg_bwd_shape).
#include <stdlib.h>
#include "plan.h"
#include "prof.h"
#include "fftg.h"

namespace se {

constexpr int kPreBatch = 4;      // bin pairs a thread keeps in flight: up to 10 floats each

struct StftgBwdArgs {
  int F, T, hop, m;
  int HB, halo, FRI, S, bufN, maxov, wav_stride;
  FftgSchedule sched;
  const float* window;
  const cf* tw;
  const cf* rtw;
};

__global__ __launch_bounds__(kGThreads) void stftg_bwd_kernel(const float* __restrict__ grad_power, const float* __restrict__ grad_complx,
                                                              const float* __restrict__ complx, StftgBwdArgs a, float* __restrict__ grad_wav,
                                                              float* __restrict__ pads) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  const int m = a.m, K = m + 1, S = a.S, F = a.F, T = a.T, hop = a.hop, n_fft = 2 * m;
  cf* bufA = reinterpret_cast<cf*>(g_smem);
  cf* bufB = bufA + a.bufN;
  cf* tw = bufB + a.bufN;                                  // [m]
  cf* rtw = tw + m;                                        // [m]
  float* win = reinterpret_cast<float*>(rtw + m);          // [2 m]

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int span = a.HB * hop;
  const int p0 = blockIdx.x * span;                   // first padded sample of this workgroup
  const int P = T + n_fft;                            // padded length
  const int fbase = blockIdx.x * a.HB - a.halo;       // first frame reaching into the span (may be negative)
  const int flo = max(fbase, 0);
  const int fhi = min(fbase + a.FRI, F);              // exclusive
  const int nfr = max(fhi - flo, 0);                  // 0: the span lies past the last frame (T no multiple of the hop): gpad = 0 there

  for (int i = tid; i < m; i += kGThreads) { tw[i] = a.tw[i]; rtw[i] = a.rtw[i]; }
  for (int i = tid; i < n_fft; i += kGThreads) win[i] = a.window[i];
  __syncthreads();                                    // twiddles visible

  // ---- pre-pass: G -> Z rows (frame fl of the workgroup sits in row flo - fbase + fl).  X' = 2 G / c_k: the stages then return gy itself
  {
    const int pairs = m / 2 + 1;
    const int items = nfr * pairs;
    const size_t gbase = ((size_t)b * F + flo) * K;
    const float2* gc2 = reinterpret_cast<const float2*>(grad_complx);
    const float2* cx2 = reinterpret_cast<const float2*>(complx);
    cf* Z0 = bufA + (flo - fbase) * S;
    for (int base = 0; base < items; base += kGThreads * kPreBatch) {
      float2 ck[kPreBatch], cn[kPreBatch], xk[kPreBatch], xn[kPreBatch];
      float pk[kPreBatch], pn[kPreBatch];
#pragma unroll
      for (int u = 0; u < kPreBatch; ++u) {
        const int it = base + tid + kGThreads * u;
        const int fl = it / pairs, k = it - fl * pairs;
        const size_t g = gbase + (size_t)fl * K;
        const bool ok = it < items;
        ck[u] = cn[u] = xk[u] = xn[u] = make_float2(0.f, 0.f);
        pk[u] = pn[u] = 0.f;
        if (ok && grad_complx) { ck[u] = gc2[g + k]; cn[u] = gc2[g + m - k]; }
        if (ok && grad_power) { pk[u] = grad_power[g + k]; pn[u] = grad_power[g + m - k]; xk[u] = cx2[g + k]; xn[u] = cx2[g + m - k]; }
      }
#pragma unroll
      for (int u = 0; u < kPreBatch; ++u) {
        const int it = base + tid + kGThreads * u;
        if (it < items) {
          const int fl = it / pairs, k = it - fl * pairs;
          cf gk = cf_make(fmaf(2.f * pk[u], xk[u].x, ck[u].x), fmaf(2.f * pk[u], xk[u].y, ck[u].y));
          cf gn = cf_make(fmaf(2.f * pn[u], xn[u].x, cn[u].x), fmaf(2.f * pn[u], xn[u].y, cn[u].y));
          if (k == 0) { gk = cf_make(2.f * gk.x, 0.f); gn = cf_make(2.f * gn.x, 0.f); }      // c_k = 1 at {0, m}, imaginary parts dropped
          cf zk, zn;
          fftg_pre_pair(gk, gn, rtw[k], &zk, &zn);
          cf* Z = Z0 + fl * S;
          Z[k] = zk;
          if (k != 0) Z[m - k] = zn;                  // 2 k = m pairs the bin with itself: both values agree
        }
      }
    }
  }
  __syncthreads();

  // ---- stages (inverse)
  cf* src = bufA;
  cf* dst = bufB;
  {
    const int r0 = flo - fbase;
    int s = 1;
    for (int st = 0; st < a.sched.n_stages; ++st) {
      const int r = a.sched.radix[st];
      const int per = m / r;
      for (int it = tid; it < nfr * per; it += kGThreads) {
        const int fl = it / per, i = it - fl * per;
        fftg_item<+1>(src + (r0 + fl) * S, dst + (r0 + fl) * S, tw, m, r, s, i);
      }
      __syncthreads();
      cf* t = src; src = dst; dst = t;
      s *= r;
    }
  }

  // ---- overlap-add; the loop contains LDS reads and global STORES only
  const float* xs = reinterpret_cast<const float*>(src);    // row f - fbase: 2 m reals gy_f[0 .. n_fft) at stride 2 S floats
  float* wrow = grad_wav + (size_t)b * a.wav_stride;
  float* prow = pads + (size_t)b * n_fft;
  for (int o = tid; o < span; o += kGThreads) {
    const int p = p0 + o;
    if (p >= P) break;
    const int f_last = min(p / hop, F - 1);
    float acc = 0.f;
    for (int t = 0; t < a.maxov; ++t) {
      const int f = f_last - t;
      const int rr = p - f * hop;
      if (f >= 0 && rr < n_fft) acc = fmaf(xs[(f - fbase) * 2 * S + rr], win[rr], acc);
    }
    if (p < m) prow[p] = acc;                         // left pad
    else if (p < T + m) wrow[p - m] = acc;
    else prow[p - T] = acc;                           // right pad: slot m + (p - T - m)
  }
}

// grad_wav[n] += gpad[m - n] (1 <= n <= m), += gpad[2 (T - 1) + m - n] (T - 1 - m <= n <= T - 2); one thread per touched sample, so the two
// folds of a sample both ranges hold (T <= 2 m) are added in a fixed order
__global__ __launch_bounds__(kGThreads) void stftg_bwd_fold_kernel(const float* __restrict__ pads, int T, int m, int wav_stride,
                                                                   float* __restrict__ grad_wav) {
  const int b = blockIdx.x;
  const float* prow = pads + (size_t)b * 2 * m;
  float* wrow = grad_wav + (size_t)b * wav_stride;
  for (int i = threadIdx.x; i < 2 * m; i += kGThreads) {
    const int n = (i < m) ? 1 + i : T - 1 - m + (i - m);
    if (i >= m && n >= 1 && n <= m) continue;         // owned by the first range's thread
    float v = wrow[n];
    if (n >= 1 && n <= m) v += prow[m - n];
    if (n >= T - 1 - m && n <= T - 2) v += prow[m + (T - 2 - n)];
    wrow[n] = v;
  }
  for (int n = T + threadIdx.x; n < wav_stride; n += kGThreads) wrow[n] = 0.f;
}

}  // namespace se

extern "C" size_t se_stft_bwd_workspace_bytes(const se_plan* plan, int B, int T) {
  if (!plan || B <= 0 || !plan->g_window) return 0;
  (void)T;
  return (size_t)B * plan->n_fft * sizeof(float);
}

extern "C" int se_stft_bwd_chunk(const se_plan* plan) {
  if (!plan) return -1;
  return plan->sbwd.HB * plan->geom.hop;
}

extern "C" int se_stft_bwd_f32(const se_plan* plan, const float* grad_power, const float* grad_complx, const float* complx, int B, int F, int T,
                               float* grad_wav, int wav_stride, void* workspace, size_t workspace_bytes, void* stream) {
  SE_REQUIRE(plan && grad_wav && workspace, "se_stft_bwd_f32: null argument");
  SE_REQUIRE(grad_power || grad_complx, "se_stft_bwd_f32: at least one of grad_power and grad_complx");
  SE_REQUIRE((grad_power != nullptr) == (complx != nullptr), "se_stft_bwd_f32: complx is required iff grad_power is given");
  SE_REQUIRE(plan->g_window && plan->sbwd.HB >= 1, "se_stft_bwd_f32: the plan has no general tables");
  const int hop = plan->geom.hop, m = plan->m;
  SE_REQUIRE(B > 0 && B <= 65535, "se_stft_bwd_f32: bad B=%d", B);
  SE_REQUIRE(T > m, "se_stft_bwd_f32: T=%d must exceed n_fft/2=%d (reflect padding)", T, m);
  SE_REQUIRE(F == T / hop + 1, "se_stft_bwd_f32: F=%d is not T / hop + 1 = %d", F, T / hop + 1);
  SE_REQUIRE((long long)F * hop + 2ll * plan->n_fft < (1ll << 31), "se_stft_bwd_f32: T=%d too long", T);
  SE_REQUIRE(wav_stride >= T, "se_stft_bwd_f32: wav_stride=%d < T=%d", wav_stride, T);
  SE_REQUIRE(workspace_bytes >= se_stft_bwd_workspace_bytes(plan, B, T), "se_stft_bwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes,
             se_stft_bwd_workspace_bytes(plan, B, T));
  se::StftgBwdArgs a;
  a.F = F; a.T = T; a.hop = hop; a.m = m;
  a.HB = plan->sbwd.HB; a.halo = plan->sbwd.halo; a.FRI = plan->sbwd.FRI; a.S = plan->sbwd.S; a.bufN = plan->sbwd.bufN; a.maxov = plan->sbwd.maxov;
  a.wav_stride = wav_stride;
  a.sched = plan->sched;
  a.window = plan->g_window; a.tw = plan->g_tw; a.rtw = plan->g_rtw;
  hipStream_t st = se::as_stream(stream);
  const size_t lds = plan->sbwd.lds;
  if (lds > 64 * 1024)      // above 64 KB the dynamic LDS size has to be granted to the kernel (per device: asked for at every such launch)
    SE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(se::stftg_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // algorithmic bytes: the spectral gradients (and the spectrum) in, the gradient row out
  const double planes = (grad_power ? 3.0 : 0.0) + (grad_complx ? 2.0 : 0.0);
  se::ProfScope prof(se::kProfStft, (double)B * 4.0 * ((double)T + planes * F * (m + 1)), st);
  const int span = a.HB * hop;
  dim3 grid((T + plan->n_fft + span - 1) / span, B);
  hipLaunchKernelGGL(se::stftg_bwd_kernel, grid, dim3(se::kGThreads), lds, st, grad_power, grad_complx, complx, a, grad_wav,
                     reinterpret_cast<float*>(workspace));
  SE_LAUNCH_CHECK();
  hipLaunchKernelGGL(se::stftg_bwd_fold_kernel, dim3(B), dim3(se::kGThreads), 0, st, reinterpret_cast<const float*>(workspace), T, m, wav_stride, grad_wav);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
