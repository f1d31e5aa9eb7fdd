// istftg.hip -- rows A6 + D2 (reduce) for ANY supported geometry (se_plan_create_any): power + phase -> waveform (inverse n_fft-point real
// FFT, window, overlap-add, envelope division, trim) with the masked square sums of the dB normalisation.  The general counterpart of
// istft.hip / istft2.hip; same outputs, zero fill and accumulator semantics.
//
// A workgroup (256 threads) owns HB hop-blocks of output (HB hop samples) of one utterance and inverse-transforms the FRI = HB + 2 halo + 1
// frames that overlap that span (halo = floor((m - 1) / hop) on either side, recomputed by the neighbours, re-read from L2):
//   pre    : one item = the bin PAIR (k, m - k) of a frame: X' = mag (cos, sin) for both bins, mag = power^(1/linear_power) or
//            exp(x / 2) for a log-power plane, (cos, sin) from the phase or from the encoded word of se_stft_tphase_f32; then
//            Z[k], Z[m - k] (fftg.h: fftg_pre_pair) into LDS.  Im X[0] = Im X[m] = 0 (c2r semantics).  Loads only in this loop.
//   stages : fftg.h with DIR = +1, ping-pong in dynamic LDS
//   ola    : out[n] = sum_f (w / m)[p - hop f] z_f[p - hop f] / sum_f w^2[p - hop f], p = n + m, over the frames f in [0, F) that contain p
//            (the edges of the signal see fewer frames than the steady state, as in torch.istft); LDS reads and global STORES only
// The reference waveform's masked square sum (ref_sumsq_out) is read in a loop of its own before the first store.
#include <stdlib.h>
#include "plan.h"
#include "prof.h"
#include "fftg.h"

namespace se {

struct IstftgArgs {
  int F, hop, m;
  int HB, halo, FRI, S, bufN, maxov;
  int log_input, use_sqrt;
  float inv_lp;
  FftgSchedule sched;
  const float* window_inv;
  const float* window_sq;
  const cf* tw;
  const cf* rtw;
};

// ENC = 1: `phase` holds the encoded words of se_stft_tphase_f32: (cos, sin) = (+-(1 - t^2), 2 t) / (1 + t^2), bit 0 = (cos < 0)
template <int ENC>
__device__ __forceinline__ cf g_polar(float p, float h, const IstftgArgs& a) {
  const float mag = a.log_input ? __expf(0.5f * p) : (a.use_sqrt ? __builtin_amdgcn_sqrtf(p) : powf(p, a.inv_lp));
  if (ENC) {
    const float s = h * h;
    const float g = mag * __builtin_amdgcn_rcpf(1.0f + s);
    return cf_make(__uint_as_float(__float_as_uint((1.0f - s) * g) ^ (__float_as_uint(h) << 31)), (h + h) * g);
  }
  float r = h * 0.15915494309189535f;                       // revolutions, reduced to [-0.5, 0.5] for the hardware sin / cos
  r -= rintf(r);
  return cf_make(mag * __builtin_amdgcn_cosf(r), mag * __builtin_amdgcn_sinf(r));
}

template <int ENC>
__global__ __launch_bounds__(kGThreads) void istftg_kernel(
    const float* __restrict__ power, const float* __restrict__ phase, IstftgArgs a, float* __restrict__ wav, int wav_stride,
    const int64_t* __restrict__ lengths, float* __restrict__ sumsq, const float* __restrict__ ref, int ref_stride, float* __restrict__ ref_sumsq) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  __shared__ float red[2][kGThreads / 64];
  const int m = a.m, K = m + 1, S = a.S, F = a.F, hop = a.hop, n_fft = 2 * m;
  cf* bufA = reinterpret_cast<cf*>(g_smem);
  cf* bufB = bufA + a.bufN;
  cf* tw = bufB + a.bufN;                                  // [m]
  cf* rtw = tw + m;                                        // [m]
  float* winv = reinterpret_cast<float*>(rtw + m);         // [2 m]  window / m
  float* wsq = winv + n_fft;                               // [2 m]  window^2

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int span = a.HB * hop;
  const int o0 = blockIdx.x * span;                   // first output sample of this workgroup
  const int n_out = hop * (F - 1);
  const int fbase = blockIdx.x * a.HB - a.halo;       // first frame overlapping the span (may be negative)
  const int flo = max(fbase, 0);
  const int fhi = min(fbase + a.FRI, F);              // exclusive
  const int nfr = fhi - flo;
  const int len_b = lengths ? (int)min((int64_t)n_out, lengths[b]) : 0;

  for (int i = tid; i < m; i += kGThreads) { tw[i] = a.tw[i]; rtw[i] = a.rtw[i]; }
  for (int i = tid; i < n_fft; i += kGThreads) { winv[i] = a.window_inv[i]; wsq[i] = a.window_sq[i]; }

  // ---- the reference waveform of the level normalisation: its masked square sum over n < min(lengths[b], wav_stride, ref_stride); the
  //      samples past the hop (F - 1) this transform returns (T not a multiple of the hop) go to the row's last workgroup
  float sr = 0.f;
  if (ref_sumsq) {
    const float* rrow = ref + (size_t)b * ref_stride;
    for (int o = tid; o < span; o += kGThreads) {
      const int n = o0 + o;
      if (n < len_b) { const float v = rrow[n]; sr = fmaf(v, v, sr); }
    }
    if (blockIdx.x == gridDim.x - 1) {
      const int rfull = (int)min((int64_t)min(wav_stride, ref_stride), lengths[b]);
      for (int n = n_out + tid; n < rfull; n += kGThreads) { const float v = rrow[n]; sr = fmaf(v, v, sr); }
    }
  }
  __syncthreads();                                    // twiddles visible

  // ---- pre-pass: spectrum -> Z rows (frame fl of the workgroup sits in row flo - fbase + fl)
  {
    const int pairs = m / 2 + 1;
    const size_t gbase = ((size_t)b * F + flo) * K;
    cf* Z0 = bufA + (flo - fbase) * S;
#pragma unroll 4
    for (int it = tid; it < nfr * pairs; it += kGThreads) {
      const int fl = it / pairs, k = it - fl * pairs;
      const size_t g = gbase + (size_t)fl * K;
      cf xk = g_polar<ENC>(power[g + k], phase[g + k], a);
      cf xn = g_polar<ENC>(power[g + m - k], phase[g + m - k], a);
      if (k == 0) xk.y = xn.y = 0.f;
      cf zk, zn;
      fftg_pre_pair(xk, xn, rtw[k], &zk, &zn);
      cf* Z = Z0 + fl * S;
      Z[k] = zk;
      if (k != 0) Z[m - k] = zn;                      // 2 k = m pairs the bin with itself: both values agree
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

  // ---- overlap-add + envelope + masked square sum; the loop contains LDS reads and global STORES only
  const float* xs = reinterpret_cast<const float*>(src);    // row f - fbase: 2 m reals z[0 .. n_fft) at stride 2 S floats
  float ss = 0.f;
  float* wrow = wav + (size_t)b * wav_stride;
  for (int o = tid; o < span; o += kGThreads) {
    const int n = o0 + o;
    if (n >= n_out) break;
    const int p = n + m;                              // padded index
    const int f_last = min(p / hop, F - 1);
    float acc = 0.f, env = 0.f;
    for (int t = 0; t < a.maxov; ++t) {
      const int f = f_last - t;
      const int rr = p - f * hop;
      if (f >= 0 && rr < n_fft) {
        acc = fmaf(xs[(f - fbase) * 2 * S + rr], winv[rr], acc);
        env += wsq[rr];
      }
    }
    const float v = acc * __builtin_amdgcn_rcpf(env);
    wrow[n] = v;
    if (n < len_b) ss = fmaf(v, v, ss);
  }
  // right-pad region [n_out, wav_stride) -- zero-filled by the last workgroup of the row
  if (blockIdx.x == gridDim.x - 1)
    for (int n = n_out + tid; n < wav_stride; n += kGThreads) wrow[n] = 0.f;

  if (sumsq) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ss += __shfl_down(ss, off);
      sr += __shfl_down(sr, off);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ss; red[1][tid >> 6] = sr; }
    __syncthreads();
    if (tid == 0) atomicAdd(&sumsq[b], red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    if (tid == 64 && ref_sumsq) atomicAdd(&ref_sumsq[b], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

}  // namespace se

int se_istftg_launch(const se_plan* plan, const float* power, const float* phase, int enc, int log_input, float linear_power, int B, int F,
                     float* wav_out, int wav_stride, const int64_t* lengths, float* sumsq_out, const float* ref, int ref_stride,
                     float* ref_sumsq_out, void* stream) {
  SE_REQUIRE(plan->general, "se_istftg_launch: not a general plan");
  const int hop = plan->geom.hop;
  SE_REQUIRE((long long)hop * F + plan->n_fft < (1ll << 31), "iSTFT: F=%d too long", F);
  const int n_out = hop * (F - 1);
  hipStream_t st = se::as_stream(stream);
  if (sumsq_out) {      // one clearing launch for both accumulators when they sit side by side
    int zrc_;
    if (ref_sumsq_out == sumsq_out + B) zrc_ = se::zero_async(sumsq_out, sizeof(float) * 2 * B, st);
    else {
      zrc_ = se::zero_async(sumsq_out, sizeof(float) * B, st);
      if (!zrc_ && ref_sumsq_out) zrc_ = se::zero_async(ref_sumsq_out, sizeof(float) * B, st);
    }
    if (zrc_) return zrc_;
  }
  se::IstftgArgs a;
  a.F = F; a.hop = hop; a.m = plan->m;
  a.HB = plan->inv.HB; a.halo = plan->inv.halo; a.FRI = plan->inv.FRI; a.S = plan->inv.S; a.bufN = plan->inv.bufN; a.maxov = plan->inv.maxov;
  a.log_input = log_input != 0;
  a.use_sqrt = linear_power == 2.0f;
  a.inv_lp = 1.0f / linear_power;
  a.sched = plan->sched;
  a.window_inv = plan->g_window_inv; a.window_sq = plan->g_window_sq; a.tw = plan->g_tw; a.rtw = plan->g_rtw;
  const int span = a.HB * hop;
  dim3 grid((n_out + span - 1) / span, B);
  const size_t lds = plan->inv.lds;
  if (lds > 64 * 1024)      // above 64 KB the dynamic LDS size has to be granted to the kernel (per device: asked for at every such launch)
    SE_HIP(hipFuncSetAttribute(enc ? reinterpret_cast<const void*>(se::istftg_kernel<1>) : reinterpret_cast<const void*>(se::istftg_kernel<0>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  se::ProfScope prof(se::kProfIstft, (double)B * (8.0 * F * (plan->m + 1) + 4.0 * n_out), st);
  if (enc)
    hipLaunchKernelGGL((se::istftg_kernel<1>), grid, dim3(se::kGThreads), lds, st, power, phase, a, wav_out, wav_stride, lengths, sumsq_out,
                       ref_sumsq_out ? ref : nullptr, ref_stride, ref_sumsq_out);
  else
    hipLaunchKernelGGL((se::istftg_kernel<0>), grid, dim3(se::kGThreads), lds, st, power, phase, a, wav_out, wav_stride, lengths, sumsq_out,
                       ref_sumsq_out ? ref : nullptr, ref_stride, ref_sumsq_out);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
