// plan.h -- preprocessor plan: geometry + device tables (window, twiddles, sparse mel bank).
#pragma once
#include <vector>
#include "common.h"
#include "fftg_plan.h"

namespace se {
constexpr int kNfft = 400;
constexpr int kHalf = 200;      // complex FFT size
constexpr int kBins = 201;
constexpr int kHop = 160;
constexpr int kMelMaxW = 32;    // max bins under one mel triangle
constexpr int kMelMax = 128;     // 40 (the reference's configs) ... 128 (the MFCC branch's own mel bank, torchaudio's default)

// ---- launch shapes of the general kernels (stftg.hip, istftg.hip), fixed per plan.  Rows of the ping-pong FFT buffers hold m complex values
// at a stride of S = an odd number >= m + 9: frames then start on different banks, and the buffer that is not holding the spectrum has
// room for the two output planes (FR x (m + 1) floats each, shifted by up to 3 floats to the output's 16-B phase).
constexpr int kGThreads = 256;
constexpr int kGFillIters = 16;                 // fill loads a thread keeps in flight: FR m <= 256 x 16
constexpr size_t kGFwdLds = 48 * 1024;          // forward transform: three workgroups per CU
constexpr size_t kGInvLdsSmall = 64 * 1024;     // inverse transform: two or more workgroups per CU when the halo leaves that efficient,
constexpr size_t kGInvLdsLarge = 159 * 1024;    // else one workgroup on (almost) the whole 160 KiB

inline int fftg_row_stride(int m) { return (m + 9) | 1; }

struct StftgShape {
  int FR;            // frames per workgroup
  int S;             // row stride of the FFT buffers (complex)
  int bufN;          // complex values per FFT buffer (even: 16-B aligned sections)
  int planeN;        // floats per output plane in LDS (a multiple of 4)
  int melN;          // words of the CSR mel table in LDS
  size_t lds;        // dynamic LDS bytes
};

inline StftgShape stftg_shape_for(int m, int melN, int FR) {
  StftgShape s;
  s.FR = FR;
  s.S = fftg_row_stride(m);
  s.bufN = (FR * s.S + 1) & ~1;
  s.planeN = (FR * (m + 1) + 3 + 3) & ~3;
  s.melN = (melN + 3) & ~3;
  s.lds = (size_t)16 * s.bufN + (size_t)24 * m + (size_t)4 * s.melN;      // two buffers, stage + recombination twiddles, window, mel table
  return s;
}

inline StftgShape stftg_shape(int m, int melN) {
  int FR = std::min(32, kGThreads * kGFillIters / m);
  while (FR > 1 && stftg_shape_for(m, melN, FR).lds > kGFwdLds) --FR;
  return stftg_shape_for(m, melN, FR);
}

struct IstftgShape {
  int HB;            // hop-blocks of output per workgroup
  int halo;          // frames before the span's first hop-block that reach into it (as many follow its last one, plus that block's own second frame)
  int FRI;           // frames transformed per workgroup = HB + 2 halo + 1
  int S, bufN;
  int maxov;         // frames that overlap one sample: ceil(n_fft / hop)
  size_t lds;
};

inline IstftgShape istftg_shape(int m, int hop) {
  IstftgShape s;
  s.S = fftg_row_stride(m);
  s.halo = (m - 1) / hop;
  s.maxov = (2 * m + hop - 1) / hop;
  const int extra = 2 * s.halo + 1;
  const size_t tables = (size_t)32 * m;                                     // two twiddle tables, window / m, window^2
  auto frames = [&](size_t budget) { return (int)((budget - tables) / ((size_t)16 * s.S)); };
  int FRI = frames(kGInvLdsSmall);
  if (FRI < 3 * extra) FRI = frames(kGInvLdsLarge);
  FRI = std::min(FRI, 64 + extra);
  s.FRI = FRI;
  s.HB = FRI - extra;
  s.bufN = (FRI * s.S + 1) & ~1;
  s.lds = (size_t)16 * s.bufN + tables;
  return s;
}

// the adjoint of the inverse transform (istftg_bwd.hip): FR frames per workgroup; their output elements (FR (m + 1)) and the gradient samples
// they cover ((FR - 1) hop + n_fft) both fit kGFillIters register slots per thread, and the LDS stays within the forward's 48 KB
struct IstftgBwdShape {
  int FR, S, bufN;
  size_t lds;
};

inline IstftgBwdShape istftg_bwd_shape(int m, int hop) {
  const int cap = kGThreads * kGFillIters;
  IstftgBwdShape s;
  s.S = fftg_row_stride(m);
  auto lds = [&](int FR) { return (size_t)16 * ((FR * s.S + 1) & ~1) + (size_t)32 * m; };      // two buffers; twiddles, window, window^2
  int FR = std::min(32, cap / (m + 1));
  while (FR > 1 && ((FR - 1) * hop + 2 * m > cap || lds(FR) > kGFwdLds)) --FR;
  s.FR = FR;
  s.bufN = (FR * s.S + 1) & ~1;
  s.lds = lds(FR);
  return s;
}

// the adjoint of the forward transform (stftg_bwd.hip): a workgroup owns HB hop-blocks of the PADDED gradient (HB hop samples of T + n_fft) and
// inverse-transforms the FRI = HB + halo frames that reach into that span (halo = floor((n_fft - 1) / hop) frames start before it).  Within
// the forward's 48 KB where the halo leaves that efficient (HB >= 2 halo), else one workgroup on (almost) the whole LDS, as istftg_shape
struct StftgBwdShape {
  int HB, halo, FRI, S, bufN, maxov;
  size_t lds;
};

inline StftgBwdShape stftg_bwd_shape(int m, int hop) {
  StftgBwdShape s;
  s.S = fftg_row_stride(m);
  s.halo = (2 * m - 1) / hop;
  s.maxov = (2 * m + hop - 1) / hop;
  const size_t tables = (size_t)24 * m;                                     // two twiddle tables, window
  auto frames = [&](size_t budget) { return (int)((budget - tables) / ((size_t)16 * s.S)); };
  int FRI = frames(kGFwdLds);
  if (FRI < 3 * s.halo) FRI = frames(kGInvLdsLarge);
  FRI = std::min(FRI, 64 + s.halo);
  s.FRI = FRI;
  s.HB = FRI - s.halo;
  s.bufN = (FRI * s.S + 1) & ~1;
  s.lds = (size_t)16 * s.bufN + tables;
  return s;
}
}  // namespace se

struct se_plan {
  se_geometry geom;
  int device;
  // host copies
  std::vector<float> h_window;   // n_fft (win centred, zero padded)
  std::vector<float> h_melfb;    // (n_freq, n_mels)
  // device tables (one allocation)
  void* d_blob;
  float* d_window;      // [400]   forward window
  float* d_window_inv;  // [400]   window / 200 (inverse transform scale folded in)
  float* d_window_sq;   // [400]   window^2
  float2* d_tw200;      // [200]   (cos, sin)(2 pi t / 200)
  float2* d_tw400;      // [200]   (cos, sin)(2 pi k / 400), k < 200 (also serves W200^t = tw400[2t] / -tw400[2t-200])
  int* d_mel_start;     // [kMelMax]
  int* d_mel_len;       // [kMelMax]
  float* d_mel_w;       // [kMelMax][kMelMaxW]

  // ---- a GENERAL plan (se_plan_create_any): none of the 400-sized tables above exists; the entry points dispatch on `general`
  bool general = false;
  int m = 0, n_fft = 0;            // n_fft = 2 m = 2 (n_freq - 1)
  se::FftgSchedule sched = {};
  se::StftgShape fwd = {};
  se::IstftgShape inv = {};
  // ---- the adjoint iSTFT (se_istft_bwd_f32) runs on the general tables for BOTH plan kinds: a plan of se_plan_create builds m, n_fft, sched,
  //      g_window, g_window_sq, g_tw and g_rtw for its geometry in a blob of their own (d_blob_g) at creation and stays `general == false`
  se::IstftgBwdShape bwd = {};
  se::StftgBwdShape sbwd = {};     // the adjoint STFT (se_stft_bwd_f32), on the same tables
  void* d_blob_g = nullptr;
  float* g_window = nullptr;       // [n_fft]  forward window
  float* g_window_inv = nullptr;   // [n_fft]  window / m (the inverse transform's scale folded in)
  float* g_window_sq = nullptr;    // [n_fft]  window^2
  se::cf* g_tw = nullptr;          // [m]      (cos, sin)(2 pi t / m): stage twiddles
  se::cf* g_rtw = nullptr;         // [m]      (cos, sin)(2 pi k / n_fft): recombination twiddles
  int* g_mel = nullptr;            // CSR mel bank: [n_mels + 1] offsets into the weights, [n_mels] first bins, [nnz] weights (as float bits)
  int mel_words = 0;
};

// the general kernels behind the entry points of stft.hip / istft.hip (stftg.hip, istftg.hip); job layout as se::StftOut
struct se_stftg_job { float* power; float* phase; float* complx; float* mel; int channel; int vec_ok; int enc; };
int se_stftg_launch(const se_plan* plan, const float* wavs, int B, int C, int T, const se_stftg_job* jobs, int njobs, void* stream);
int se_istftg_launch(const se_plan* plan, const float* power, const float* phase, int enc, int log_input, float linear_power, int B, int F,
                     float* wav_out, int wav_stride, const int64_t* lengths, float* sumsq_out, const float* ref, int ref_stride,
                     float* ref_sumsq_out, void* stream);
