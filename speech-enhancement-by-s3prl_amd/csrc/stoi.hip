// stoi.hip -- STOI / ESTOI of every utterance of a batch on the device (evaluation.py:28-36 applied per utterance at runner.py:586-603): no D2H of
// the waveforms, no host worker pool.  The definition is written out in stoi_tables.h and include/se_amd.h (the algorithm of pystoi.stoi; parity
// unpinned vs pystoi).  Launches of one se_stoi_f32 call, all asynchronous on `stream`, no allocation, no host sync:
//   resample  fs -> 10 kHz polyphase FIR of clean and processed, all utterances in one launch: 256 outputs per workgroup, the taps (branch-major)
//             and the signal tile staged in LDS, fp64 accumulation, zero fill past n10[b].  Skipped at 10 kHz (the later kernels read the input).
//   energy    dB energy of every windowed frame of the clean signal: one wave per four frames, fp64 from the product on
//   mask      per utterance: maximum, keep mask (e > max - 40), exclusive scan in chunks of 256 frames (any frame count), kept-index list, K
//   bands     per (utterance, four compacted frames, both signals): the compacted frame is rebuilt from its up to three windowed source frames
//             (never materialised), windowed again, zero padded to 512 and transformed by fftg.h's m = 256 complex FFT + post pass in LDS;
//             15 band sums of |X|^2 and their sqrt -> tob (2, B, 15, Fmax)
//   score     one wave per (utterance, segment): lane <-> frame of the segment, the 15 band values of both signals in registers, fp64; row
//             statistics are wave sums (xor butterflies: every lane holds the same bits), column statistics are in-lane
//   fold      per utterance the segment values are summed in a fixed order (thread-strided partial sums, fixed LDS tree) -> stoi_out
#include <math.h>
#include <vector>
#include "common.h"
#include "fftg.h"
#include "fftg_plan.h"
#include "stoi_dev.h"      // the plan, the partition constants, stoi_len, wave_sum and the workspace layout (shared with stoi_bwd.hip)

namespace se {

// out (2, B, n10max): signal 0 = clean, 1 = processed
__global__ __launch_bounds__(kStoiResOut) void stoi_resample_kernel(const float* __restrict__ clean, const float* __restrict__ processed, int ld,
                                                                    const int64_t* __restrict__ lengths, int B, int T, int p, int q, int L, int NT,
                                                                    int tileN, const float* __restrict__ taps, int n10max, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float r_smem[];
  float* tile = r_smem;                // [tileN]
  float* gp = r_smem + tileN;          // [p][NT]
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n0 = blockIdx.x * kStoiResOut;
  const int64_t len = stoi_len(lengths, b, T);
  const int n10 = (int)stoi_n10(len, p, q);
  float* o = out + ((size_t)blockIdx.z * B + b) * (size_t)n10max;
  const int n = n0 + tid;
  if (n0 >= n10) {                     // workgroup-uniform: nothing but zero fill
    if (n < n10max) o[n] = 0.f;
    return;
  }
  const float* x = (blockIdx.z ? processed : clean) + (size_t)b * ld;
  // the tile starts one sample below floor((n0 q - L) / p): every index m_hi - j of the loop below lies inside it
  const int lo_t = n0 * q - L;
  const int m_base = (lo_t >= 0 ? lo_t / p : -((-lo_t + p - 1) / p)) - 1;
  for (int i = tid; i < tileN; i += kStoiResOut) {
    const int m = m_base + i;
    tile[i] = (m >= 0 && m < len) ? x[m] : 0.f;
  }
  for (int i = tid; i < p * NT; i += kStoiResOut) gp[i] = taps[i];
  __syncthreads();
  if (n >= n10max) return;
  float v = 0.f;
  if (n < n10) {
    const int t = n * q + L;
    const int m_hi = t / p, r = t - m_hi * p;
    const int jn = (2 * L - r) / p + 1;            // taps of branch r (<= NT)
    const float* g = gp + r * NT;
    const float* s = tile + (m_hi - m_base);
    double acc = 0.0;
    for (int j = 0; j < jn; ++j) acc += (double)s[-j] * (double)g[j];
    v = (float)acc;
  }
  o[n] = v;
}

// energy (B, Fmax) fp64: 20 log10(|w x[i : i + 256]| + EPS) of the clean signal's frames
__global__ __launch_bounds__(256) void stoi_energy_kernel(const float* __restrict__ xs, size_t ldx, const int64_t* __restrict__ lengths, int T,
                                                          int p, int q, int Fmax, const double* __restrict__ w64, double* __restrict__ energy) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = (int)stoi_frames(stoi_n10(stoi_len(lengths, b, T), p, q));
  const float* x = xs + (size_t)b * ldx;
  for (int k = 0; k < kStoiEnergyFrames / 4; ++k) {
    const int f = blockIdx.x * kStoiEnergyFrames + wave * (kStoiEnergyFrames / 4) + k;
    if (f >= F) break;                              // wave-uniform
    double ss = 0.0;
#pragma unroll
    for (int r = 0; r < kStoiFrame / 64; ++r) {
      const int n = lane + 64 * r;
      const double v = w64[n] * (double)x[(size_t)f * kStoiHop + n];
      ss += v * v;
    }
    ss = wave_sum(ss);
    if (lane == 0) energy[(size_t)b * Fmax + f] = 20.0 * log10(sqrt(ss) + kStoiEps);
  }
}

// kept_idx (B, Fmax): the source frame of every kept frame, in order; kept (B): their number
__global__ __launch_bounds__(kStoiScanChunk) void stoi_mask_kernel(const double* __restrict__ energy, const int64_t* __restrict__ lengths, int T, int p,
                                                                   int q, int Fmax, int* __restrict__ kept_idx, int* __restrict__ kept,
                                                                   int32_t* __restrict__ kept_out) {
  __shared__ double s_max[4];
  __shared__ int s_cnt[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int F = (int)stoi_frames(stoi_n10(stoi_len(lengths, b, T), p, q));
  const double* e = energy + (size_t)b * Fmax;
  double mx = -INFINITY;
  for (int i = tid; i < F; i += kStoiScanChunk) mx = fmax(mx, e[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
  if (lane == 0) s_max[wave] = mx;
  __syncthreads();
  const double thr = fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3])) - kStoiDynRange;
  int base = 0;
  for (int c0 = 0; c0 < F; c0 += kStoiScanChunk) {      // F is workgroup-uniform: every thread runs every chunk
    const int i = c0 + tid;
    const bool keep = i < F && e[i] > thr;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                     // the previous chunk's s_cnt has been read
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += s_cnt[w];
    if (keep) kept_idx[(size_t)b * Fmax + off + before] = i;
    base += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  }
  if (tid == 0) {
    kept[b] = base;
    if (kept_out) kept_out[b] = base;
  }
}

// tob (2, B, 15, Fmax): third-octave envelopes of the compacted clean (0) and processed (1) signals; columns from kept[b] on are zero
__global__ __launch_bounds__(256) void stoi_bands_kernel(const float* __restrict__ xs, const float* __restrict__ ys, size_t ldx,
                                                         const int* __restrict__ kept_idx, const int* __restrict__ kept, int B, int Fmax,
                                                         const float* __restrict__ window, const cf* __restrict__ g_tw, const cf* __restrict__ g_rtw,
                                                         FftgSchedule sched, StoiBands bands, float* __restrict__ tob) {
  __shared__ __attribute__((aligned(16))) cf bufA[kStoiTr * kStoiRow];
  __shared__ __attribute__((aligned(16))) cf bufB[kStoiTr * kStoiRow];
  __shared__ cf tw[kStoiM], rtw[kStoiM];
  __shared__ float win[kStoiFrame];
  __shared__ int s_idx[kStoiFr + 2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int j0 = blockIdx.x * kStoiFr;
  const int K = kept[b];
  const int nf = min(kStoiFr, K - j0);
  const int ncol = min(kStoiFr, Fmax - j0);
  if (nf <= 0) {                                          // workgroup-uniform
    for (int it = tid; it < 2 * kStoiBands * ncol; it += 256) {
      const int f = it % ncol, rest = it / ncol, band = rest % kStoiBands, sig = rest / kStoiBands;
      tob[(((size_t)sig * B + b) * kStoiBands + band) * Fmax + j0 + f] = 0.f;
    }
    return;
  }
  if (tid < kStoiFr + 2) {
    const int kk = j0 - 1 + tid;
    s_idx[tid] = (kk >= 0 && kk < K) ? kept_idx[(size_t)b * Fmax + kk] : -1;
  }
  for (int i = tid; i < kStoiM; i += 256) { tw[i] = g_tw[i]; rtw[i] = g_rtw[i]; }
  for (int i = tid; i < kStoiFrame; i += 256) win[i] = window[i];
  __syncthreads();

  // ---- fill: transform tr = 2 f + sig; z[n] = (v[2 n], v[2 n + 1]), v = w (kept frame j + the halves of its neighbours), zero from n = 128 on
  const int ntr = 2 * nf;
  for (int it = tid; it < ntr * kStoiM; it += 256) {
    const int tr = it / kStoiM, n = it - tr * kStoiM;
    cf z = cf_make(0.f, 0.f);
    if (n < kStoiFrame / 2) {
      const int f = tr >> 1;
      const float* s = ((tr & 1) ? ys : xs) + (size_t)b * ldx;
      const int ic = s_idx[f + 1];
      const int pa = 2 * n;                               // pa, pa + 1 lie in the same half
      const bool first = pa < kStoiHop;
      const int in = first ? s_idx[f] : s_idx[f + 2];     // first half: the second half of kept frame j - 1; second half: the first half of j + 1
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
    bufA[tr * kStoiRow + n] = z;
  }
  __syncthreads();

  // ---- stages (fftg.h), work item = (transform, i)
  cf* src = bufA;
  cf* dst = bufB;
  {
    int s = 1;
    for (int st = 0; st < sched.n_stages; ++st) {
      const int r = sched.radix[st];
      const int per = kStoiM / r;
      for (int it = tid; it < ntr * per; it += 256) {
        const int tr = it / per, i = it - tr * per;
        fftg_item<-1>(src + tr * kStoiRow, dst + tr * kStoiRow, tw, kStoiM, r, s, i);
      }
      __syncthreads();
      cf* t = src; src = dst; dst = t;
      s *= r;
    }
  }

  // ---- post: |X[k]|^2, |X[256 - k]|^2 from Z[k], Z[256 - k] into a plane in the buffer the spectrum is not in
  float* Pw = reinterpret_cast<float*>(dst);             // Pw[tr * kStoiPlane + k], k <= 256
  {
    const int pairs = kStoiM / 2 + 1;
    for (int it = tid; it < ntr * pairs; it += 256) {
      const int tr = it / pairs, k = it - tr * pairs;
      const cf* Z = src + tr * kStoiRow;
      cf X1, X2;
      fftg_post_pair(Z[k], Z[k == 0 ? 0 : kStoiM - k], rtw[k], &X1, &X2);
      Pw[tr * kStoiPlane + k] = X1.x * X1.x + X1.y * X1.y;
      if (2 * k != kStoiM) Pw[tr * kStoiPlane + kStoiM - k] = X2.x * X2.x + X2.y * X2.y;
    }
  }
  __syncthreads();

  // ---- bands: sqrt of the sum over bins lo .. hi - 1; the columns of this workgroup past K are zero
  for (int it = tid; it < 2 * kStoiBands * ncol; it += 256) {
    const int f = it % ncol, rest = it / ncol, band = rest % kStoiBands, sig = rest / kStoiBands;
    float v = 0.f;
    if (f < nf) {
      const float* P = Pw + (2 * f + sig) * kStoiPlane;
      float acc = 0.f;
      for (int k = bands.lo[band]; k < bands.hi[band]; ++k) acc += P[k];
      v = sqrtf(acc);
    }
    tob[(((size_t)sig * B + b) * kStoiBands + band) * Fmax + j0 + f] = v;
  }
}

// partial (B, Fmax): the sum over the 15 x 30 block of segment m (columns [m, m + 30)) of the normalised products
__global__ __launch_bounds__(256) void stoi_score_kernel(const float* __restrict__ tob, const int* __restrict__ kept, int B, int Fmax, int extended,
                                                         double* __restrict__ partial) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = blockIdx.x * 4 + wave;
  const int J = (int)stoi_segments(kept[b]);
  if (seg >= J) return;                                   // wave-uniform
  const bool act = lane < kStoiSeg;
  double x[kStoiBands], y[kStoiBands];
#pragma unroll
  for (int r = 0; r < kStoiBands; ++r) {
    const size_t o = (size_t)r * Fmax + seg + (act ? lane : 0);
    x[r] = act ? (double)tob[((size_t)b * kStoiBands) * Fmax + o] : 0.0;
    y[r] = act ? (double)tob[(((size_t)B + b) * kStoiBands) * Fmax + o] : 0.0;
  }
  const double inv_n = 1.0 / (double)kStoiSeg;
  double acc = 0.0;
  if (!extended) {
    const double clip = 1.0 + pow(10.0, -kStoiBeta / 20.0);
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {
      const double nx = sqrt(wave_sum(x[r] * x[r])), ny = sqrt(wave_sum(y[r] * y[r]));
      const double yp = fmin(nx / (ny + kStoiEps) * y[r], x[r] * clip);
      const double mx = wave_sum(x[r]) * inv_n, my = wave_sum(yp) * inv_n;
      const double xc = act ? x[r] - mx : 0.0, yc = act ? yp - my : 0.0;
      const double nxc = sqrt(wave_sum(xc * xc)), nyc = sqrt(wave_sum(yc * yc));
      acc += (yc / (nyc + kStoiEps)) * (xc / (nxc + kStoiEps));
    }
  } else {
#pragma unroll
    for (int r = 0; r < kStoiBands; ++r) {               // rows: zero mean, unit norm over the 30 frames
      const double mx = wave_sum(x[r]) * inv_n, my = wave_sum(y[r]) * inv_n;
      const double xc = act ? x[r] - mx : 0.0, yc = act ? y[r] - my : 0.0;
      const double sx = wave_sum(xc * xc), sy = wave_sum(yc * yc);
      x[r] = sx > 0.0 ? xc / sqrt(sx) : 0.0;
      y[r] = sy > 0.0 ? yc / sqrt(sy) : 0.0;
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
    acc = (act && sx > 0.0 && sy > 0.0) ? dot / (sqrt(sx) * sqrt(sy)) : 0.0;
  }
  acc = wave_sum(acc);
  if (lane == 0) partial[(size_t)b * Fmax + seg] = acc;
}

__global__ __launch_bounds__(256) void stoi_fold_kernel(const double* __restrict__ partial, const int* __restrict__ kept, int Fmax, int extended,
                                                        float* __restrict__ out) {
  __shared__ double red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int J = (int)stoi_segments(kept[b]);
  double a = 0.0;
  for (int i = tid; i < J; i += 256) a += partial[(size_t)b * Fmax + i];
  red[tid] = a;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) out[b] = J <= 0 ? kStoiTooShort : (float)(red[0] / ((double)J * (double)(extended ? kStoiSeg : kStoiBands)));
}

__global__ void stoi_short_kernel(int B, float* __restrict__ out, int32_t* __restrict__ kept_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  out[b] = kStoiTooShort;
  if (kept_out) kept_out[b] = 0;
}

}  // namespace se

extern "C" int se_stoi_plan_create(int sample_rate, se_stoi_plan** out) {
  SE_REQUIRE(out, "se_stoi_plan_create: null argument");
  *out = nullptr;
  int p = 1, q = 1;
  if (!se::stoi_rate(sample_rate, &p, &q)) {
    se::set_error("se_stoi_plan_create: unsupported sample rate %d (the supported rates are 16000 and 10000)", sample_rate);
    return SE_ERR_UNSUPPORTED;
  }
  se_stoi_plan* pl = new se_stoi_plan();
  pl->sample_rate = sample_rate;
  pl->p = p;
  pl->q = q;
  se::stoi_band_edges(pl->lo, pl->hi);
  std::vector<float> taps;
  if (p != q) {
    std::vector<double> g;
    pl->L = se::stoi_make_taps(p, q, &g);
    pl->NT = se::stoi_branch_taps(p, pl->L);
    taps.assign((size_t)p * pl->NT, 0.f);
    for (int i = 0; i < (int)g.size(); ++i) taps[(size_t)(i % p) * pl->NT + i / p] = (float)g[i];
  }
  double w64[se::kStoiFrame];
  float w32[se::kStoiFrame];
  se::stoi_make_window(w64);
  for (int n = 0; n < se::kStoiFrame; ++n) w32[n] = (float)w64[n];
  std::vector<se::cf> tw(se::kStoiM), rtw(se::kStoiM);
  se::fftg_make_twiddles(se::kStoiM, tw.data(), rtw.data());
  if (!se::fftg_make_schedule(se::kStoiM, &pl->sched)) {
    delete pl;
    se::set_error("se_stoi_plan_create: no radix schedule for m=%d", se::kStoiM);
    return SE_ERR_UNSUPPORTED;
  }

  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    delete pl;
    se::set_error("se_stoi_plan_create: no HIP device visible (the product path has no CPU fallback)");
    return SE_ERR_NO_DEVICE;
  }
  e = hipGetDevice(&pl->device);
  if (e != hipSuccess) {
    delete pl;
    return se::hip_fail(e, "hipGetDevice", __FILE__, __LINE__);
  }
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_w64 = 0, o_w32 = o_w64 + al(sizeof(w64)), o_tw = o_w32 + al(sizeof(w32)), o_rtw = o_tw + al(8 * se::kStoiM),
               o_taps = o_rtw + al(8 * se::kStoiM), total = o_taps + al(4 * taps.size() + 4);
  e = hipMalloc(&pl->d_blob, total);
  if (e != hipSuccess) {
    delete pl;
    return se::hip_fail(e, "hipMalloc(stoi tables)", __FILE__, __LINE__);
  }
  char* base = (char*)pl->d_blob;
  pl->d_window64 = (double*)(base + o_w64);
  pl->d_window = (float*)(base + o_w32);
  pl->d_tw = (se::cf*)(base + o_tw);
  pl->d_rtw = (se::cf*)(base + o_rtw);
  pl->d_taps = taps.empty() ? nullptr : (float*)(base + o_taps);
  struct { void* dst; const void* src; size_t bytes; } copies[] = {
      {pl->d_window64, w64, sizeof(w64)}, {pl->d_window, w32, sizeof(w32)}, {pl->d_tw, tw.data(), (size_t)8 * se::kStoiM},
      {pl->d_rtw, rtw.data(), (size_t)8 * se::kStoiM}, {base + o_taps, taps.data(), 4 * taps.size()}};
  for (auto& c : copies) {
    if (c.bytes == 0) continue;
    e = hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      se_stoi_plan_destroy(pl);
      return se::hip_fail(e, "hipMemcpy(stoi tables)", __FILE__, __LINE__);
    }
  }
  *out = pl;
  return SE_OK;
}

extern "C" void se_stoi_plan_destroy(se_stoi_plan* plan) {
  if (!plan) return;
  if (plan->d_blob) (void)hipFree(plan->d_blob);
  delete plan;
}

extern "C" size_t se_stoi_workspace_bytes(const se_stoi_plan* plan, int B, int T) {
  if (!plan || B <= 0 || T <= 0) return 0;
  return se::stoi_layout(plan, B, T).total;
}

extern "C" int se_stoi_f32(const se_stoi_plan* plan, const float* clean, const float* processed, int ld, const int64_t* lengths, int B, int T,
                           int extended, float* stoi_out, int32_t* kept_out, float* tob_out, void* workspace, size_t workspace_bytes, void* stream) {
  SE_REQUIRE(plan && clean && processed && stoi_out, "se_stoi_f32: null argument");
  SE_REQUIRE(B > 0 && B <= 65535 && T > 0 && ld >= T, "se_stoi_f32: bad shape (B=%d T=%d ld=%d)", B, T, ld);
  SE_REQUIRE((long long)T * (plan->p > plan->q ? plan->p : plan->q) + 2ll * plan->L < (1ll << 31), "se_stoi_f32: T=%d too long", T);
  const se::StoiLayout l = se::stoi_layout(plan, B, T);
  SE_REQUIRE(workspace && workspace_bytes >= l.total, "se_stoi_f32: workspace of %zu bytes, %zu needed (se_stoi_workspace_bytes)", workspace_bytes,
             l.total);
  hipStream_t st = se::as_stream(stream);
  const int Fmax = l.Fmax, p = plan->p, q = plan->q;
  if (Fmax == 0) {       // T itself holds no frame: every utterance is too short
    hipLaunchKernelGGL(se::stoi_short_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, stoi_out, kept_out);
    SE_LAUNCH_CHECK();
    return SE_OK;
  }
  char* ws = (char*)workspace;
  double* energy = (double*)(ws + l.o_energy);
  double* partial = (double*)(ws + l.o_partial);
  float* xr = (float*)(ws + l.o_xr);
  float* tob = tob_out ? tob_out : (float*)(ws + l.o_tob);
  int* kept_idx = (int*)(ws + l.o_idx);
  int* kept = (int*)(ws + l.o_kept);

  const float* xs = clean;
  const float* ys = processed;
  size_t ldx = (size_t)ld;
  if (plan->d_taps) {
    const int tileN = ((se::kStoiResOut - 1) * q + 2 * plan->L) / p + 4;
    const size_t lds = sizeof(float) * ((size_t)tileN + (size_t)p * plan->NT);
    hipLaunchKernelGGL(se::stoi_resample_kernel, dim3((l.n10max + se::kStoiResOut - 1) / se::kStoiResOut, B, 2), dim3(se::kStoiResOut), lds, st, clean,
                       processed, ld, lengths, B, T, p, q, plan->L, plan->NT, tileN, plan->d_taps, l.n10max, xr);
    SE_LAUNCH_CHECK();
    xs = xr;
    ys = xr + (size_t)B * (size_t)l.n10max;
    ldx = (size_t)l.n10max;
  }
  hipLaunchKernelGGL(se::stoi_energy_kernel, dim3((Fmax + se::kStoiEnergyFrames - 1) / se::kStoiEnergyFrames, B), dim3(256), 0, st, xs, ldx, lengths, T,
                     p, q, Fmax, plan->d_window64, energy);
  SE_LAUNCH_CHECK();
  hipLaunchKernelGGL(se::stoi_mask_kernel, dim3(B), dim3(se::kStoiScanChunk), 0, st, energy, lengths, T, p, q, Fmax, kept_idx, kept, kept_out);
  SE_LAUNCH_CHECK();
  se::StoiBands bands;
  for (int i = 0; i < se::kStoiBands; ++i) { bands.lo[i] = plan->lo[i]; bands.hi[i] = plan->hi[i]; }
  hipLaunchKernelGGL(se::stoi_bands_kernel, dim3((Fmax + se::kStoiFr - 1) / se::kStoiFr, B), dim3(256), 0, st, xs, ys, ldx, kept_idx, kept, B, Fmax,
                     plan->d_window, plan->d_tw, plan->d_rtw, plan->sched, bands, tob);
  SE_LAUNCH_CHECK();
  if (Fmax >= se::kStoiSeg) {
    const int Jmax = Fmax - se::kStoiSeg + 1;
    hipLaunchKernelGGL(se::stoi_score_kernel, dim3((Jmax + 3) / 4, B), dim3(256), 0, st, tob, kept, B, Fmax, extended, partial);
    SE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(se::stoi_fold_kernel, dim3(B), dim3(256), 0, st, partial, kept, Fmax, extended, stoi_out);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
