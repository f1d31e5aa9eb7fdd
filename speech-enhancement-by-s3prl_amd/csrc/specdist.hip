// specdist.hip -- one resolution of the multi-resolution STFT criterion (Yamamoto et al. 2020: spectral convergence + log-magnitude L1) on two
// power planes, per utterance, with its gradient wrt the predicted plane.  |X| = sqrt(max(P_pred, clamp)), |Y| = sqrt(max(P_tar, clamp));
// over the bins k < K of the frames f < frames_b = lengths[b] / hop + 1 (runner.py:455; 0 for lengths[b] <= 0):
//   a = sum (|Y| - |X|)^2,  c = sum |Y|^2,  l = sum |log|Y| - log|X||,  n = frames_b K
//   loss_b = sqrt(a) / (sqrt(c) + 1e-12) + l / max(n, 1)
// The shape of objectives.hip: per-utterance fp64 partial sums into their own slots of a slab (no atomics, fixed order), closed-form
// coefficients per utterance, one elementwise pass that writes the gradient:
//   d loss_b / d P = [ (|X| - |Y|) / (sqrt(a) (sqrt(c) + 1e-12)) - sign(log|Y| - log|X|) / (n |X|) ] / (2 |X|)
// exactly 0 where P_pred <= clamp, on frames >= frames_b, in the first term when a == 0; sign(0) = 0.
#include <math.h>
#include <algorithm>
#include "common.h"

namespace se {

constexpr double kSpecdistEps = 1e-12;

__device__ __forceinline__ int specdist_frames(const int64_t* __restrict__ lengths, int b, int hop, int F) {
  const int64_t wl = lengths[b];
  if (wl <= 0) return 0;
  return (int)min((int64_t)F, wl / hop + 1);
}

__global__ __launch_bounds__(256) void specdist_slab_kernel(const float* __restrict__ pred, const float* __restrict__ tar,
                                                            const int64_t* __restrict__ lengths, int hop, int F, int K, float clamp,
                                                            double* __restrict__ slab) {
  __shared__ double red[3][4];
  const int b = blockIdx.y;
  const int64_t L = (int64_t)specdist_frames(lengths, b, hop, F) * K;
  const float* p = pred + (size_t)b * F * K;
  const float* t = tar + (size_t)b * F * K;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  for (; i + 3 * stride < L; i += 4 * stride) {      // eight loads in flight per thread
    float pv[4], tv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { pv[u] = p[i + u * stride]; tv[u] = t[i + u * stride]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float qx = fmaxf(pv[u], clamp), qy = fmaxf(tv[u], clamp);
      const float x = sqrtf(qx), y = sqrtf(qy);
      a0 += (double)(y - x) * (double)(y - x);
      a1 += (double)qy;
      a2 += (double)fabsf(0.5f * (logf(qy) - logf(qx)));
    }
  }
  for (; i < L; i += stride) {
    const float qx = fmaxf(p[i], clamp), qy = fmaxf(t[i], clamp);
    const float x = sqrtf(qx), y = sqrtf(qy);
    a0 += (double)(y - x) * (double)(y - x);
    a1 += (double)qy;
    a2 += (double)fabsf(0.5f * (logf(qy) - logf(qx)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a0 += __shfl_xor(a0, off);
    a1 += __shfl_xor(a1, off);
    a2 += __shfl_xor(a2, off);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a0;
    red[1][threadIdx.x >> 6] = a1;
    red[2][threadIdx.x >> 6] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3)
    slab[((size_t)b * gridDim.x + blockIdx.x) * 3 + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// loss_b and coef[b] = { 1 / (sqrt(a) (sqrt(c) + eps)) or 0 for a == 0,  1 / max(n, 1) } from utterance b's `chunks` slots, in slot order
__global__ void specdist_final_kernel(const double* __restrict__ slab, int chunks, const int64_t* __restrict__ lengths, int hop, int F, int K, int B,
                                      float* __restrict__ loss_b, double* __restrict__ coef) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double a = 0.0, c = 0.0, l = 0.0;
  const double* r = slab + (size_t)b * chunks * 3;
  for (int j = 0; j < chunks; ++j) { a += r[3 * j]; c += r[3 * j + 1]; l += r[3 * j + 2]; }
  const double n = (double)specdist_frames(lengths, b, hop, F) * (double)K;
  const double den = sqrt(c) + kSpecdistEps;
  const double inv_n = 1.0 / fmax(n, 1.0);
  loss_b[b] = (float)(sqrt(a) / den + l * inv_n);
  coef[2 * b] = a > 0.0 ? 1.0 / (sqrt(a) * den) : 0.0;
  coef[2 * b + 1] = inv_n;
}

__global__ __launch_bounds__(256) void specdist_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tar,
                                                            const int64_t* __restrict__ lengths, int hop, int F, int K, float clamp,
                                                            const double* __restrict__ coef, float scale, float* __restrict__ grad) {
  const int b = blockIdx.y;
  const int64_t L = (int64_t)specdist_frames(lengths, b, hop, F) * K, tot = (int64_t)F * K;
  const float csc = (float)coef[2 * b] * scale, cn = (float)coef[2 * b + 1] * scale;
  const float* p = pred + (size_t)b * F * K;
  const float* t = tar + (size_t)b * F * K;
  float* g = grad + (size_t)b * F * K;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
    float v = 0.f;
    if (i < L) {
      const float pv = p[i];
      if (pv > clamp) {
        const float qy = fmaxf(t[i], clamp);
        const float x = sqrtf(pv), y = sqrtf(qy);
        const float sgn = (qy > pv) ? 1.f : (qy < pv) ? -1.f : 0.f;      // sign(log|Y| - log|X|): the logarithm and the root are monotone
        const float rx = 1.0f / x;
        v = 0.5f * rx * ((x - y) * csc - sgn * cn * rx);
      }
    }
    g[i] = v;
  }
}

}  // namespace se

// slots per utterance: enough workgroups to fill the chip, no more (the final launch walks them)
static int specdist_chunks(int B, int F, int K) {
  const int64_t by_size = ((int64_t)F * K + 8191) / 8192;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(64, by_size), std::max(1, 2048 / B)));
}

extern "C" size_t se_specdist_scratch_doubles(int B, int F, int K) {
  if (B <= 0 || F <= 0 || K <= 0) return 0;
  return (size_t)B * specdist_chunks(B, F, K) * 3 + 2 * (size_t)B;
}

static int specdist_check(const char* what, const float* pp, const float* pt, const int64_t* lengths, int hop, int B, int F, int K, float clamp,
                          const double* scratch) {
  SE_REQUIRE(pp && pt && lengths && scratch, "%s: null argument", what);
  SE_REQUIRE(B > 0 && B <= 65535 && F > 0 && K > 0 && hop > 0, "%s: bad shape B=%d F=%d K=%d hop=%d", what, B, F, K, hop);
  SE_REQUIRE(clamp > 0.f, "%s: clamp must be positive", what);
  return SE_OK;
}

extern "C" int se_specdist_loss_f32(const float* power_pred, const float* power_tar, const int64_t* lengths, int hop, int B, int F, int K, float clamp,
                                    double* scratch, float* loss_b, void* stream) {
  const int rc = specdist_check("se_specdist_loss_f32", power_pred, power_tar, lengths, hop, B, F, K, clamp, scratch);
  if (rc) return rc;
  SE_REQUIRE(loss_b, "se_specdist_loss_f32: null argument");
  hipStream_t st = se::as_stream(stream);
  const int chunks = specdist_chunks(B, F, K);
  hipLaunchKernelGGL(se::specdist_slab_kernel, dim3(chunks, B), dim3(256), 0, st, power_pred, power_tar, lengths, hop, F, K, clamp, scratch);
  SE_LAUNCH_CHECK();
  hipLaunchKernelGGL(se::specdist_final_kernel, dim3((B + 255) / 256), dim3(256), 0, st, scratch, chunks, lengths, hop, F, K, B, loss_b,
                     scratch + (size_t)B * chunks * 3);
  SE_LAUNCH_CHECK();
  return SE_OK;
}

extern "C" int se_specdist_grad_f32(const float* power_pred, const float* power_tar, const int64_t* lengths, int hop, int B, int F, int K, float clamp,
                                    const double* scratch, float grad_scale, float* grad_power_pred, void* stream) {
  const int rc = specdist_check("se_specdist_grad_f32", power_pred, power_tar, lengths, hop, B, F, K, clamp, scratch);
  if (rc) return rc;
  SE_REQUIRE(grad_power_pred, "se_specdist_grad_f32: null argument");
  const int chunks = specdist_chunks(B, F, K);
  hipLaunchKernelGGL(se::specdist_grad_kernel, dim3(chunks, B), dim3(256), 0, se::as_stream(stream), power_pred, power_tar, lengths, hop, F, K, clamp,
                     scratch + (size_t)B * chunks * 3, grad_scale, grad_power_pred);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
