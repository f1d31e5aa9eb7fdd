// stftg.hip -- rows A1+A2(+A3) for ANY supported geometry (se_plan_create_any): framing + window + n_fft-point real FFT -> power / phase /
// complex / raw mel.  The general counterpart of stft.hip (which stays the fast path of 400 / 160 / 201); same outputs, same layouts.
//
// One workgroup (256 threads) transforms FR consecutive frames of one (utterance, channel); blockIdx.z selects one of two channel jobs.
//   fill   : z[n] = (w[2n] x[2n], w[2n+1] x[2n+1]) with reflect padding; all of a thread's global loads are issued back to back (at most
//            kGFillIters pairs); workgroups whose frames lie inside the signal skip the reflect select
//   stages : the run-time-scheduled Stockham transform of fftg.h, ping-pong between two LDS buffers (rows of m complex at stride S)
//   post   : X[k], X[m-k] from Z[k], Z[m-k]; power and atan2 / encoded phase go into two LDS PLANES in the buffer the spectrum is not in,
//            laid out exactly like the output span (frame-major, m + 1 bins, shifted to the span's offset mod 4)
//   write  : the frames of a workgroup are ONE contiguous span of (B, F, K) in each plane: scalar head / tail, aligned 16-B body.  No global
//            load sits in an output loop (all tables, the mel bank included, are in LDS before the first store: one in-order vmcnt).
//   mel    : sparse HTK triangles (CSR: any width) over the power plane, lane <-> frame; written feature-major (B, n_mels, F)
// LDS (dynamic): 16 bufN + 24 m + 4 melN bytes <= 48 KB -> three workgroups per CU; FR from plan.h (stftg_shape).
#include <stdlib.h>
#include "plan.h"
#include "prof.h"
#include "fftg.h"

namespace se {

__device__ __forceinline__ int g_reflect(int i, int T) {
  // numpy / torch 'reflect' (no edge repeat); valid for |overshoot| < T
  if (i < 0) i = -i;
  if (i >= T) i = 2 * (T - 1) - i;
  return i;
}

// the two phase forms of stft.hip, restated (that file's kernels are specialised and stay untouched): same arithmetic, same word format
__device__ __forceinline__ float g_fast_atan2(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  float a = mn * __builtin_amdgcn_rcpf(mx);
  a = (mx == 0.f) ? 0.f : a;
  const float s = a * a;
  float p = fmaf(s, 0.00264226692f, -0.0152803790f);
  p = fmaf(s, p, 0.0414993092f);
  p = fmaf(s, p, -0.0741364285f);
  p = fmaf(s, p, 0.106052168f);
  p = fmaf(s, p, -0.141971514f);
  p = fmaf(s, p, 0.199923798f);
  p = fmaf(s, p, -0.333331168f);
  float r = fmaf(a * s, p, a);
  r = (ay > ax) ? (1.57079632679f - r) : r;
  r = (x < 0.f) ? (3.14159265359f - r) : r;
  return copysignf(r, y);
}

// t = y / (|X| + |x|) as fp32 with bit 0 = (x < 0); X == 0 -> 0
__device__ __forceinline__ float g_encode_phase(float x, float y, float q) {
  const float m = q * __builtin_amdgcn_rsqf(q);
  const float d = m + fabsf(x);
  const float t = (q > 0.f) ? y * __builtin_amdgcn_rcpf(d) : 0.f;
  return __uint_as_float((__float_as_uint(t) & ~1u) | (__float_as_uint(x) >> 31));
}

struct StftgArgs {
  int C, T, F, hop, m, n_mels;
  int FR, S, bufN, planeN, melN;
  FftgSchedule sched;
  const float* window;
  const cf* tw;
  const cf* rtw;
  const int* melcsr;
};

__global__ __launch_bounds__(kGThreads) void stftg_kernel(const float* __restrict__ wavs, StftgArgs a, se_stftg_job job0, se_stftg_job job1) {
  extern __shared__ __attribute__((aligned(16))) unsigned char g_smem[];
  const se_stftg_job job = blockIdx.z ? job1 : job0;
  float* __restrict__ power = job.power;
  float* __restrict__ phase = job.phase;
  float* __restrict__ complx = job.complx;
  float* __restrict__ mel = job.mel;
  const int m = a.m, K = m + 1, S = a.S, T = a.T, F = a.F, hop = a.hop;
  cf* bufA = reinterpret_cast<cf*>(g_smem);
  cf* bufB = bufA + a.bufN;
  cf* tw = bufB + a.bufN;                                  // [m]
  cf* rtw = tw + m;                                        // [m]
  float* win = reinterpret_cast<float*>(rtw + m);          // [2 m]
  int* melt = reinterpret_cast<int*>(win + 2 * m);         // [melN]

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * a.FR;
  const int nf = min(a.FR, F - f0);
  const float* x = wavs + ((size_t)b * a.C + job.channel) * (size_t)T;

  // ---- fill.  item = tid + 256 r -> (frame, n); the loads of all items first, then the tables, then the products into LDS
  const int items = nf * m;
  const bool interior = (f0 * hop - m >= 0) && ((f0 + nf - 1) * hop + m <= T);
  float xa[kGFillIters], xb[kGFillIters];
  if (interior) {
#pragma unroll
    for (int r = 0; r < kGFillIters; ++r) {
      const int it = tid + kGThreads * r;
      const int f = it / m, n = it - f * m;
      const int s = (f0 + f) * hop - m + 2 * n;
      xa[r] = (it < items) ? x[s] : 0.f;
      xb[r] = (it < items) ? x[s + 1] : 0.f;
    }
  } else {
#pragma unroll
    for (int r = 0; r < kGFillIters; ++r) {
      const int it = tid + kGThreads * r;
      const int f = it / m, n = it - f * m;
      const int s = (f0 + f) * hop - m + 2 * n;
      xa[r] = (it < items) ? x[g_reflect(s, T)] : 0.f;
      xb[r] = (it < items) ? x[g_reflect(s + 1, T)] : 0.f;
    }
  }
  for (int i = tid; i < m; i += kGThreads) { tw[i] = a.tw[i]; rtw[i] = a.rtw[i]; }
  for (int i = tid; i < 2 * m; i += kGThreads) win[i] = a.window[i];
  if (mel)
    for (int i = tid; i < a.melN; i += kGThreads) melt[i] = a.melcsr[i];
  __syncthreads();                                          // window table visible
#pragma unroll
  for (int r = 0; r < kGFillIters; ++r) {
    const int it = tid + kGThreads * r;
    if (it < items) {
      const int f = it / m, n = it - f * m;
      bufA[f * S + n] = cf_make(xa[r] * win[2 * n], xb[r] * win[2 * n + 1]);
    }
  }
  __syncthreads();

  // ---- stages (fftg.h), work item = (frame, i)
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

  // ---- post: pairs (k, m - k), k = 0 .. m / 2 -> (power, phase) of both bins into the planes, which live in the buffer the spectrum is NOT in
  const size_t obase = ((size_t)b * F + f0) * K;
  const int pad = (int)(obase & 3);             // LDS float index = pad + (output index - obase): same 16-B phase as the global span
  float* Pw = reinterpret_cast<float*>(dst) + pad;          // power plane: Pw[f * K + k]
  float* Ph = Pw + a.planeN;                                // phase plane
  {
    const int pairs = m / 2 + 1;
    for (int it = tid; it < nf * pairs; it += kGThreads) {
      const int f = it / pairs, k = it - f * pairs;
      const cf* Z = src + f * S;
      cf X1, X2;
      fftg_post_pair(Z[k], Z[k == 0 ? 0 : m - k], rtw[k], &X1, &X2);
      const bool two = (2 * k != m);
      const int o = f * K + k;
      if (complx) {       // rarely requested ('complx' features): direct 8-B stores (no loads in this loop)
        const size_t o1 = obase + (size_t)o;
        reinterpret_cast<float2*>(complx)[o1] = make_float2(X1.x, X1.y);
        if (two) reinterpret_cast<float2*>(complx)[o1 + (m - 2 * k)] = make_float2(X2.x, X2.y);
      }
      const float q1 = X1.x * X1.x + X1.y * X1.y, q2 = X2.x * X2.x + X2.y * X2.y;
      float h1 = 0.f, h2 = 0.f;
      if (phase) {
        if (job.enc) {
          h1 = g_encode_phase(X1.x, X1.y, q1);
          h2 = g_encode_phase(X2.x, X2.y, q2);
        } else {
          h1 = g_fast_atan2(X1.y, X1.x);
          h2 = g_fast_atan2(X2.y, X2.x);
        }
      }
      Pw[o] = q1;
      Ph[o] = h1;
      if (two) {                                            // k = 0 pairs with the Nyquist bin m
        Pw[o + (m - 2 * k)] = q2;
        Ph[o + (m - 2 * k)] = h2;
      }
    }
  }
  __syncthreads();

  // ---- write-out: the workgroup's nf x K outputs are ONE contiguous span of each plane with the LDS planes' layout and 16-B phase
  if (power || phase) {
    const int total = nf * K;
    const int head = job.vec_ok ? min(total, (4 - pad) & 3) : total;
    const int nvec = (total - head) >> 2;
    for (int i = tid; i < head; i += kGThreads) {
      if (power) power[obase + i] = Pw[i];
      if (phase) phase[obase + i] = Ph[i];
    }
    if (job.vec_ok) {
      for (int i = head + 4 * nvec + tid; i < total; i += kGThreads) {
        if (power) power[obase + i] = Pw[i];
        if (phase) phase[obase + i] = Ph[i];
      }
      for (int v4 = tid; v4 < nvec; v4 += kGThreads) {
        const int i = head + 4 * v4;
        if (power) *reinterpret_cast<float4*>(power + obase + i) = *reinterpret_cast<const float4*>(Pw + i);
        if (phase) *reinterpret_cast<float4*>(phase + obase + i) = *reinterpret_cast<const float4*>(Ph + i);
      }
    }
  }

  if (mel == nullptr) return;
  // ---- mel: CSR triangles over the power plane (already barrier-visible); lane <-> frame: power reads at stride K floats
  const int M = a.n_mels;
  const float* melw = reinterpret_cast<const float*>(melt + 2 * M + 1);
  for (int it = tid; it < M * 32; it += kGThreads) {
    const int mi = it >> 5, fl = it & 31;
    if (fl >= nf) continue;
    const int w0 = melt[mi], w1 = melt[mi + 1], st = melt[M + 1 + mi];
    const float* pr = Pw + fl * K + st;
    float acc = 0.f;
    for (int i = 0; i < w1 - w0; ++i) acc = fmaf(melw[w0 + i], pr[i], acc);
    mel[((size_t)b * M + mi) * F + f0 + fl] = acc;
  }
}

}  // namespace se

int se_stftg_launch(const se_plan* plan, const float* wavs, int B, int C, int T, const se_stftg_job* jobs, int njobs, void* stream) {
  SE_REQUIRE(plan->general, "se_stftg_launch: not a general plan");
  SE_REQUIRE(T > plan->m, "STFT: T=%d must exceed n_fft/2=%d (reflect padding)", T, plan->m);
  SE_REQUIRE(B <= 65535, "STFT: B=%d exceeds grid.y limit", B);
  const int hop = plan->geom.hop;
  const int F = T / hop + 1;
  SE_REQUIRE((long long)F * hop + plan->n_fft < (1ll << 31), "STFT: T=%d too long", T);
  se::StftgArgs a;
  a.C = C; a.T = T; a.F = F; a.hop = hop; a.m = plan->m; a.n_mels = plan->geom.n_mels;
  a.FR = plan->fwd.FR; a.S = plan->fwd.S; a.bufN = plan->fwd.bufN; a.planeN = plan->fwd.planeN; a.melN = plan->mel_words;
  a.sched = plan->sched;
  a.window = plan->g_window; a.tw = plan->g_tw; a.rtw = plan->g_rtw; a.melcsr = plan->g_mel;
  double bytes = 0.0;
  for (int j = 0; j < njobs; ++j)      // algorithmic bytes: 4 T in + 4 F K per written plane
    bytes += (double)B * (4.0 * T + 4.0 * F * (plan->m + 1) * ((jobs[j].power != nullptr) + (jobs[j].phase != nullptr) + 2 * (jobs[j].complx != nullptr)) +
                          (jobs[j].mel ? 4.0 * F * plan->geom.n_mels : 0.0));
  se::ProfScope prof(se::kProfStft, bytes, se::as_stream(stream));
  dim3 grid((F + a.FR - 1) / a.FR, B, njobs);
  hipLaunchKernelGGL(se::stftg_kernel, grid, dim3(se::kGThreads), plan->fwd.lds, se::as_stream(stream), wavs, a, jobs[0], jobs[njobs > 1 ? 1 : 0]);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
