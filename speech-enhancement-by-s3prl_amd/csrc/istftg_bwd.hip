// istftg_bwd.hip -- the adjoint of row A6 (OnlinePreprocessor.istft, runner.py:267) for BOTH plan kinds: d loss / d wav -> d loss / d power, with
// the phase held fixed (the decode uses the noisy phase, a constant) and linear_power = 2.  What istft.hip / istftg.hip compute is linear in
// the spectrum X = sqrt(P) (c + i s); its transpose is a forward STFT of the envelope-divided gradient:
//   gy[p]  = g[p - m] / env[p]                    m <= p < m + hop (F - 1), else 0   (ZERO padding; env with the forward's edge rule)
//   G_f    = rfft_N( w[.] gy[hop f + .] )         the sign convention of stftg.hip
//   dRe X  = (c_k / N) Re G,  dIm X = (c_k / N) Im G      c_k = 1 for k in {0, m} (where the Im term is dropped: c2r semantics), else 2
//   dP     = (dRe c + dIm s) / (2 sqrt(P))        and exactly 0 where P <= 0 (the stated subgradient; torch gives inf / nan there)
//
// Structured like stftg_kernel: a workgroup (256 threads) owns FR consecutive frames of one utterance.
//   loads  : every global load of a thread is issued up front, back to back: the gradient samples of the span the frames cover
//            ((FR - 1) hop + n_fft, at most kGFillIters per thread) and the power / phase words of the thread's output elements
//   stage  : gy of the span into LDS once (env recomputed from window^2 in LDS), in the buffer the first FFT stage overwrites afterwards
//   fill   : z[n] = (w[2n] gy[2n], w[2n+1] gy[2n+1]) per frame;  stages: fftg.h, DIR = -1;  post: G[k], G[m - k] into LDS rows of m + 1 bins
//   write  : thread <-> consecutive output element of the workgroup's ONE contiguous span of (B, F, K): coalesced stores, no loads in the loop
// No atomics, no allocation: grad_power is fully written and repeats are bit-identical.  LDS 16 bufN + 32 m bytes <= 48 KB.
#include <stdlib.h>
#include "plan.h"
#include "prof.h"
#include "fftg.h"

namespace se {

struct IstftgBwdArgs {
  int F, hop, m, FR, S, bufN, maxov, wav_stride;
  FftgSchedule sched;
  const float* window;
  const float* window_sq;
  const cf* tw;
  const cf* rtw;
};

// the unit phasor of istftg.hip's g_polar (mag = 1): same arithmetic, same word format
template <int ENC>
__device__ __forceinline__ cf gb_phasor(float h) {
  if (ENC) {
    const float s = h * h;
    const float g = __builtin_amdgcn_rcpf(1.0f + s);
    return cf_make(__uint_as_float(__float_as_uint((1.0f - s) * g) ^ (__float_as_uint(h) << 31)), (h + h) * g);
  }
  float r = h * 0.15915494309189535f;
  r -= rintf(r);
  return cf_make(__builtin_amdgcn_cosf(r), __builtin_amdgcn_sinf(r));
}

template <int ENC>
__global__ __launch_bounds__(kGThreads) void istftg_bwd_kernel(const float* __restrict__ grad_wav, const float* __restrict__ power,
                                                               const float* __restrict__ phase, IstftgBwdArgs a, float* __restrict__ grad_power) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  const int m = a.m, K = m + 1, S = a.S, F = a.F, hop = a.hop, n_fft = 2 * m;
  cf* bufA = reinterpret_cast<cf*>(g_smem);
  cf* bufB = bufA + a.bufN;
  cf* tw = bufB + a.bufN;                                  // [m]
  cf* rtw = tw + m;                                        // [m]
  float* win = reinterpret_cast<float*>(rtw + m);          // [2 m]
  float* wsq = win + n_fft;                                // [2 m]
  float* gy = reinterpret_cast<float*>(bufB);              // [span] <= 2 bufN floats; dead once the fill has read it

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * a.FR;
  const int nf = min(a.FR, F - f0);
  const int n_out = hop * (F - 1);
  const int span = (nf - 1) * hop + n_fft;                 // padded samples p0 .. p0 + span covered by the frames
  const int p0 = f0 * hop;
  const int total = nf * K;
  const size_t obase = ((size_t)b * F + f0) * K;

  // ---- every global load of the thread, back to back
  const float* grow = grad_wav + (size_t)b * a.wav_stride;
  float gv[kGFillIters], pv[kGFillIters], hv[kGFillIters];
#pragma unroll
  for (int r = 0; r < kGFillIters; ++r) {
    const int i = tid + kGThreads * r;
    const int n = p0 + i - m;
    gv[r] = (i < span && n >= 0 && n < n_out) ? grow[n] : 0.f;
  }
#pragma unroll
  for (int r = 0; r < kGFillIters; ++r) {
    const int it = tid + kGThreads * r;
    pv[r] = (it < total) ? power[obase + it] : 0.f;
    hv[r] = (it < total) ? phase[obase + it] : 0.f;
  }
  for (int i = tid; i < m; i += kGThreads) { tw[i] = a.tw[i]; rtw[i] = a.rtw[i]; }
  for (int i = tid; i < n_fft; i += kGThreads) { win[i] = a.window[i]; wsq[i] = a.window_sq[i]; }
  __syncthreads();                                          // tables visible

  // ---- stage gy = g / env (the forward's envelope: the frames f in [0, F) that contain p)
#pragma unroll
  for (int r = 0; r < kGFillIters; ++r) {
    const int i = tid + kGThreads * r;
    if (i < span) {
      const int p = p0 + i;
      const int f_last = min(p / hop, F - 1);
      float env = 0.f;
      for (int t = 0; t < a.maxov; ++t) {
        const int f = f_last - t;
        const int rr = p - f * hop;
        if (f >= 0 && rr < n_fft) env += wsq[rr];
      }
      const int n = p - m;
      gy[i] = (n >= 0 && n < n_out) ? gv[r] * __builtin_amdgcn_rcpf(env) : 0.f;
    }
  }
  __syncthreads();

  // ---- fill: frame f of the workgroup starts at gy[f hop]
  for (int it = tid; it < nf * m; it += kGThreads) {
    const int f = it / m, n = it - f * m;
    const float* x = gy + f * hop + 2 * n;
    bufA[f * S + n] = cf_make(x[0] * win[2 * n], x[1] * win[2 * n + 1]);
  }
  __syncthreads();

  // ---- stages (fftg.h, forward direction)
  cf* src = bufA;
  cf* dst = bufB;
  {
    int s = 1;
    for (int st = 0; st < a.sched.n_stages; ++st) {
      const int r = a.sched.radix[st];
      const int per = m / r;
      for (int it = tid; it < nf * per; it += kGThreads) {
        const int f = it / per, i = it - f * per;
        fftg_item<-1>(src + f * S, dst + f * S, tw, m, r, s, i);
      }
      __syncthreads();
      cf* t = src; src = dst; dst = t;
      s *= r;
    }
  }

  // ---- post: G[k], G[m - k] of every frame into rows of the buffer the spectrum is not in (row stride S > m: bin m has a slot)
  {
    const int pairs = m / 2 + 1;
    for (int it = tid; it < nf * pairs; it += kGThreads) {
      const int f = it / pairs, k = it - f * pairs;
      const cf* Z = src + f * S;
      cf X1, X2;
      fftg_post_pair(Z[k], Z[k == 0 ? 0 : m - k], rtw[k], &X1, &X2);
      dst[f * S + k] = X1;
      if (2 * k != m) dst[f * S + m - k] = X2;              // k = 0 pairs with the Nyquist bin m
    }
  }
  __syncthreads();

  // ---- write: dP = (c_k / N) (Re G c + Im G s) / (2 sqrt(P)); LDS reads and global STORES only
  const float inv_n = 1.0f / (float)n_fft;
#pragma unroll
  for (int r = 0; r < kGFillIters; ++r) {
    const int it = tid + kGThreads * r;
    if (it < total) {
      const int f = it / K, k = it - f * K;
      const cf G = dst[f * S + k];
      const cf u = gb_phasor<ENC>(hv[r]);
      const bool edge = (k == 0) || (k == m);
      const float d = edge ? 0.5f * G.x * u.x : fmaf(G.x, u.x, G.y * u.y);        // (c_k / 2) (Re G c + Im G s)
      const float P = pv[r];
      grad_power[obase + it] = (P > 0.f) ? d * inv_n * __builtin_amdgcn_rsqf(P) : 0.f;
    }
  }
}

}  // namespace se

// d loss / d wav (B, wav_stride) -> d loss / d power (B, F, K): the backward of se_istft_f32 (phase) / se_istft_tphase_f32 (tphase), linear_power = 2
extern "C" int se_istft_bwd_f32(const se_plan* plan, const float* grad_wav, int wav_stride, const float* power, const float* phase,
                                const unsigned* tphase, int B, int F, float* grad_power, void* stream) {
  SE_REQUIRE(plan && grad_wav && power && grad_power, "se_istft_bwd_f32: null argument");
  SE_REQUIRE((phase != nullptr) != (tphase != nullptr), "se_istft_bwd_f32: exactly one of phase and tphase");
  SE_REQUIRE(B > 0 && B <= 65535 && F >= 2, "se_istft_bwd_f32: bad B=%d F=%d", B, F);
  SE_REQUIRE(plan->g_window && plan->bwd.FR >= 1, "se_istft_bwd_f32: the plan has no general tables");
  const int hop = plan->geom.hop, m = plan->m;
  SE_REQUIRE((long long)hop * F + plan->n_fft < (1ll << 31), "se_istft_bwd_f32: F=%d too long", F);
  const int n_out = hop * (F - 1);
  SE_REQUIRE(wav_stride >= n_out, "se_istft_bwd_f32: wav_stride=%d < %d output samples", wav_stride, n_out);
  se::IstftgBwdArgs a;
  a.F = F; a.hop = hop; a.m = m; a.FR = plan->bwd.FR; a.S = plan->bwd.S; a.bufN = plan->bwd.bufN; a.maxov = (plan->n_fft + hop - 1) / hop;
  a.wav_stride = wav_stride;
  a.sched = plan->sched;
  a.window = plan->g_window; a.window_sq = plan->g_window_sq; a.tw = plan->g_tw; a.rtw = plan->g_rtw;
  hipStream_t st = se::as_stream(stream);
  // algorithmic bytes: the gradient row in, power and phase in, grad_power out
  se::ProfScope prof(se::kProfIstft, (double)B * 4.0 * ((double)wav_stride + 3.0 * F * (m + 1)), st);
  dim3 grid((F + a.FR - 1) / a.FR, B);
  if (tphase)
    hipLaunchKernelGGL((se::istftg_bwd_kernel<1>), grid, dim3(se::kGThreads), plan->bwd.lds, st, grad_wav, power, reinterpret_cast<const float*>(tphase), a,
                       grad_power);
  else
    hipLaunchKernelGGL((se::istftg_bwd_kernel<0>), grid, dim3(se::kGThreads), plan->bwd.lds, st, grad_wav, power, phase, a, grad_power);
  SE_LAUNCH_CHECK();
  return SE_OK;
}

extern "C" int se_istft_bwd_chunk_frames(const se_plan* plan) {
  if (!plan) return -1;
  return plan->bwd.FR;
}
