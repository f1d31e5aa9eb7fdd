// stoi_dev.h -- what the STOI / ESTOI forward (stoi.hip) and its backward (stoi_bwd.hip) share on the device side: the plan, the partition
// constants of the kernels, the two device helpers and the workspace layout of one se_stoi_f32 call.  The host-only tables and counting rules
// stay in stoi_tables.h.
#pragma once
#include <stdint.h>
#include "common.h"
#include "fftg.h"
#include "stoi_tables.h"

struct se_stoi_plan {
  int sample_rate = 0, device = 0;
  int p = 1, q = 1, L = 0, NT = 0;      // resampler: p / q, half length, taps per branch
  int lo[se::kStoiBands], hi[se::kStoiBands];
  se::FftgSchedule sched = {};
  void* d_blob = nullptr;
  float* d_taps = nullptr;              // [p][NT] branch-major, zero padded (NULL at 10 kHz)
  float* d_window = nullptr;            // [256]
  double* d_window64 = nullptr;         // [256]
  se::cf* d_tw = nullptr;               // [256] stage twiddles
  se::cf* d_rtw = nullptr;              // [256] recombination twiddles
};

namespace se {

constexpr int kStoiM = kStoiNfft / 2;                  // 256: complex FFT size
constexpr int kStoiFr = 4;                             // compacted frames per workgroup of the band kernel
constexpr int kStoiTr = 2 * kStoiFr;                   // transforms per workgroup (clean + processed)
constexpr int kStoiRow = (kStoiM + 9) | 1;             // 265: row stride of the FFT buffers (fftg_row_stride)
constexpr int kStoiPlane = kStoiM + 4;                 // row stride of the power plane (bins 0 .. 256)
constexpr int kStoiScanChunk = 256;                    // frames per step of the mask kernel's scan
constexpr int kStoiEnergyFrames = 16;                  // frames per workgroup of the energy kernel
constexpr int kStoiResOut = 256;                       // outputs per workgroup of the resampler

struct StoiBands { int lo[kStoiBands], hi[kStoiBands]; };

__device__ __forceinline__ int64_t stoi_len(const int64_t* lengths, int b, int T) {
  if (!lengths) return T;
  const int64_t l = lengths[b];
  return l < 0 ? 0 : (l > T ? T : l);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct StoiLayout {
  int n10max, Fmax;
  size_t o_energy, o_partial, o_xr, o_tob, o_idx, o_kept, total;
};

inline StoiLayout stoi_layout(const se_stoi_plan* plan, int B, int T) {
  StoiLayout l;
  l.n10max = (int)stoi_n10(T, plan->p, plan->q);
  l.Fmax = (int)stoi_frames(l.n10max);
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t BF = (size_t)B * (size_t)l.Fmax;
  l.o_energy = 0;
  l.o_partial = l.o_energy + al(8 * BF);
  l.o_xr = l.o_partial + al(8 * BF);
  l.o_tob = l.o_xr + (plan->d_taps ? al((size_t)8 * B * (size_t)l.n10max) : 0);
  l.o_idx = l.o_tob + al((size_t)8 * kStoiBands * BF);
  l.o_kept = l.o_idx + al(4 * BF);
  l.total = l.o_kept + al((size_t)4 * B);
  return l;
}

}  // namespace se
