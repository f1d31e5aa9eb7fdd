// mhsa_route.h -- which kernel runs an attention forward call: one pure function of the call's shape facts.
//
// Host-only and free of HIP (a plain C++ compiler takes it: tests/test_mhsa_route.py walks it under the sanitizers).  One predicate per
// route says what that kernel CAN run; mhsa_route() alone holds the order of preference and the measured threshold.  The launch site
// (mhsa.hip) and the 8-wave launcher (mhsa8.hip) re-check the predicate and fail the call otherwise: there is no silent fall-back.
#pragma once
#include <stddef.h>
#include <stdlib.h>

namespace se {

// A call that passed the entries' argument checks: 0 < B <= 65535, T > 0, 0 < heads <= 65535.
struct MhsaCall {
  int B, T, heads;
  bool prescaled;     // se_mhsa_fwd_prescaled_bf16 / se_mhsa_fwd_prescaled_variant_bf16: queries carry log2(e) / sqrt(64), inference
  bool dropout;       // make_dropout(p, seed).thr16 != 0 (training forward with attention dropout)
};

enum class MhsaRoute {
  Wave4,              // mhsa.hip mhsa_fwd_kernel<3, 0, 0>: training and plain forward
  Wave4Dropout,       // mhsa.hip mhsa_fwd_kernel<2, 1, 0>: training forward with dropout
  Wave4Prescaled,     // mhsa.hip mhsa_fwd_kernel<3, 0, 1>: prescaled inference, 4 waves (variant 0)
  Wave8Prescaled,     // mhsa8.hip mhsa_wave8_fwd_kernel: prescaled inference, 8 waves on one LDS-DMA staged tile (variant 10)
};

// The switches that survive (A/B tools and tests set them), read once by mhsa_tuning().
struct MhsaTuning {
  int force_variant = -1;       // SE_AMD_MHSA_PIPE: >= 0 forces one variant of the prescaled entry (0 or 10)
  int wave8_min_wgs = 768;      // SE_AMD_MHSA8_MIN_WGS: 8-wave workgroups from which on the 8-wave kernel is the default
  int speculate = 1;            // SE_AMD_MHSA_SPEC: 0 = always the exact online-softmax tile (A/B)
};

inline MhsaTuning mhsa_tuning_from_env() {
  MhsaTuning t;
  auto env = [](const char* name, int& v) { if (const char* e = getenv(name)) v = atoi(e); };
  env("SE_AMD_MHSA_PIPE", t.force_variant);
  env("SE_AMD_MHSA8_MIN_WGS", t.wave8_min_wgs);
  env("SE_AMD_MHSA_SPEC", t.speculate);
  return t;
}

inline const MhsaTuning& mhsa_tuning() {
  static const MhsaTuning t = mhsa_tuning_from_env();
  return t;
}

// ---- launch geometry

struct MhsaGrid {
  int rows;           // query rows per workgroup (32 per wave)
  int threads;        // threads per workgroup
};

constexpr int kMhsaWave4Rows = 128, kMhsaWave8Rows = 256;

inline MhsaGrid mhsa_grid(MhsaRoute r) {
  return r == MhsaRoute::Wave8Prescaled ? MhsaGrid{kMhsaWave8Rows, 512} : MhsaGrid{kMhsaWave4Rows, 256};
}

// ---- what each kernel can run

inline bool mhsa_wave4_ok(const MhsaCall&) { return true; }                // 64-bit addressing throughout: any validated call
inline bool mhsa_wave4_prescaled_ok(const MhsaCall&) { return true; }
// the pair index of the counter-based mask, (row, key / 2) over B * heads * T rows, is a 32-bit counter
inline bool mhsa_wave4_dropout_ok(const MhsaCall& c) { return (double)c.B * c.heads * c.T * ((c.T + 1) / 2) < 4294967296.0; }
// the 32-bit lane offsets of the LDS-DMA address one (utterance, head) block of the fused rows: T * 3 H * 2 bytes, H = 64 heads
inline double mhsa_wave8_block_bytes(const MhsaCall& c) { return (double)c.T * 3.0 * (c.heads * 64) * 2.0; }
inline bool mhsa_wave8_prescaled_ok(const MhsaCall& c) { return mhsa_wave8_block_bytes(c) < 2147483648.0; }

inline bool mhsa_route_ok(MhsaRoute r, const MhsaCall& c) {
  switch (r) {
    case MhsaRoute::Wave4: return mhsa_wave4_ok(c);
    case MhsaRoute::Wave4Dropout: return mhsa_wave4_dropout_ok(c);
    case MhsaRoute::Wave4Prescaled: return mhsa_wave4_prescaled_ok(c);
    case MhsaRoute::Wave8Prescaled: return mhsa_wave8_prescaled_ok(c);
  }
  return false;
}

// the variant numbers of se_mhsa_fwd_prescaled_variant_bf16 (and SE_AMD_MHSA_PIPE) that name a kernel of the library
inline bool mhsa_variant_ok(int variant) { return variant == 0 || variant == 10; }

// ---- the order of preference and the threshold (a forced variant must have passed mhsa_variant_ok)

inline MhsaRoute mhsa_route(const MhsaCall& c, const MhsaTuning& t) {
  if (!c.prescaled) return c.dropout ? MhsaRoute::Wave4Dropout : MhsaRoute::Wave4;
  if (t.force_variant >= 0) return t.force_variant == 10 ? MhsaRoute::Wave8Prescaled : MhsaRoute::Wave4Prescaled;
  // round 4: 8-wave workgroups on one LDS-DMA staged K / V tile, two per CU, half of each SIMD's waves half a tile behind (107 vs 118 us
  // at B = 32) from 768 such workgroups (1.5 per CU slot pair) on -- B >= 16 at T = 1001; below that the 4-wave workgroups (three per CU,
  // twice as many of them) cover the CUs better (profiles/r04_mhsa_bsweep.txt).  A call past the 8-wave kernel's 31-bit limit is NOT sent
  // to the 4-wave kernel: the launcher fails it.
  const long wgs8 = (long)((c.T + kMhsaWave8Rows - 1) / kMhsaWave8Rows) * c.heads * c.B;
  return wgs8 >= t.wave8_min_wgs ? MhsaRoute::Wave8Prescaled : MhsaRoute::Wave4Prescaled;
}

}  // namespace se
