// mhsa8.hip -- row B2 core, inference form (pre-scaled queries): the flash attention forward as an 8-wave workgroup on one LDS-DMA staged
// K / V tile.  The default of se_mhsa_fwd_prescaled_bf16 from 768 workgroups on (mhsa_route.h: Wave8Prescaled, variant 10); bit-identical to
// mhsa.hip's 4-wave kernel.  profiles/ record it under its earlier name, mhsaN_fwd_kernel<8, 4, 1>.
//
// Built in round 4 after the in-kernel stamps of mhsa.hip (tools/mhsa_stamps.py, profiles/r04_mhsa_stamps.txt) showed where that kernel's waves
// wait: a wave ALONE on its SIMD needs ~2 200 cycles per 64-key tile for 512 cycles of MFMA and ~430 of softmax issue -- the K fragment reads in
// front of QK^T (~300 exposed), the matrix results in front of the first exponential (~250), the V^T fragment reads inside PV (~160), the
// global -> register -> LDS staging and its barrier (~200; the round-3 ablation put the staging at 27 % of the launch at 128 queries per staged
// tile).  The softmax of a 64-key tile is ~520 issue cycles of ONE wave (a single wave issues a vector instruction every ~5 cycles, a SIMD with
// 3-4 waves one every ~2) against 512 matrix cycles, so a strict two-wave alternation leaves the matrix pipe idle for half of every load segment.
//
// Workgroup = 8 waves = 256 query rows of one (utterance, head); wave = 32 query rows; the waves SHARE the staged tile and otherwise run FREE
// (one barrier per tile, no segment hand-shake).  The register allocation is held to 4 waves per SIMD (128 registers), so TWO workgroups are
// resident per CU: two independent barrier domains.  Per tile a wave issues two 1-KiB LDS-DMA pieces (8 rows x 128 B of K and of V; inline asm:
// through the builtin the compiler orders every later ds_read behind the DMA with vmcnt(0)) and nothing else for the staging: no global loads
// into registers, no ds_write, half of mhsa.hip's L2 -> LDS bytes per query.  Tile t + 2 is issued at the top of tile t, the wave's own pieces
// of tile t + 1 are awaited (counted vmcnt) in front of the tile's one barrier.
// Stagger: the waves with (wave & 4) != 0 -- one half of every SIMD's residents -- take the tile's barrier in the MIDDLE of their tile (between
// the softmax and the PV products) instead of at its end: a per-tile barrier otherwise re-aligns all waves of a SIMD at every tile top (they
// then queue for the matrix pipe together and exponentiate together); with the shifted barrier the two halves run half a tile apart
// (MI355X_MICROARCH.md, "Two waves per SIMD", item 9).  Hence a FOUR-slot ring: a late wave still reads V of tile t - 1 after the barrier that
// lets the early ones start tile t.
// Tile layout, swizzle and fragment addressing are mhsa.hip's (mhsa_tile.h: kv_off), as are the speculative / exact softmax tiles.
#include "clkprobe.h"
#include "common.h"
#include "prof.h"
#include "bf16.h"
#include "mhsa_tile.h"
#include "mhsa_route.h"

// developer ablation (timing only, results are wrong): -DSE_MHSAN_ABL=<mask>: 1 no LDS-DMA staging (and no waits for it),
// 2 no tile barrier, 4 no LDS fragment reads (the MFMAs take the query fragments), 8 no exponentials
#ifndef SE_MHSAN_ABL
#define SE_MHSAN_ABL 0
#endif

SE_CLKPROBE_DECL(clkprobe_mhsa)
namespace se {

constexpr int k8Q = 256;        // query rows per workgroup
constexpr int k8Slot = 16384;   // one ring slot: K tile (8 KiB) + V tile (8 KiB)
constexpr int k8Ring = 4;
static_assert(k8Q == kMhsaWave8Rows, "mhsa_route.h: query rows per workgroup of this file's kernel");

#define SE8_BAR()                                   \
  do {                                              \
    __builtin_amdgcn_sched_barrier(0);              \
    asm volatile("s_barrier" ::: "memory");         \
    __builtin_amdgcn_sched_barrier(0);              \
  } while (0)

__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void mhsa_wave8_fwd_kernel(
    const uint16_t* __restrict__ qkv, const int32_t* __restrict__ lengths, int T, int H, uint16_t* __restrict__ ctx, float dscale) {
  __shared__ __attribute__((aligned(16))) char smem[k8Ring * k8Slot];
  SE_CLKPROBE_BEGIN();
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hh = lane >> 5;
  // XCD-aware work mapping (as mhsa.hip): all query tiles of one (utterance, head) on ONE XCD, consecutive in its dispatch order
  int b, head, qt;
  {
    const int nqt = gridDim.x, pairs = gridDim.y * gridDim.z;
    const int lin = blockIdx.x + nqt * (blockIdx.y + gridDim.y * blockIdx.z);
    if ((pairs & 7) == 0) {
      const int xcd = lin & 7, i = lin >> 3;
      const int pair = 8 * (i / nqt) + xcd;
      qt = i % nqt;
      head = pair % gridDim.y;
      b = pair / gridDim.y;
    } else {
      qt = blockIdx.x; head = blockIdx.y; b = blockIdx.z;
    }
  }
  const int q0 = qt * k8Q + wave * 32;
  const int ld = 3 * H;
  const int len = (lengths && lengths[b] > 0) ? min(lengths[b], T) : T;      // 0 or less: no frame is valid, nothing is masked (the reference's -10000 on every key cancels in the softmax)
  const int nkt = (len + kAK - 1) / kAK;
  const uint16_t* base = qkv + (size_t)b * T * ld + head * kHD;

  // LDS-DMA pieces (8 rows x 128 B = 1 KiB): wave w brings K piece w and V piece w; lane l writes slot l & 7 of row l >> 3 of the piece, so it
  // FETCHES chunk (l & 7) ^ f(row)   (kv_off: slot = chunk ^ f)
  typedef __attribute__((address_space(3))) char* lds_c_t;
  const int piece = wave & 7;
  const int drow = piece * 8 + (lane >> 3);
  const uint32_t dch = (uint32_t)(((lane & 7) ^ (kv_off(drow, 0) >> 4 & 7)) * 16);
  const uint32_t dpk = (uint32_t)drow | (dch << 8);          // one register for both lane constants of the DMA address (unpacked per issue, opaquely:
                                                              // hoisted copies spilled, and a spill reload waits vmcnt(0) in front of the DMA)
  const uint32_t lds_piece = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(lds_c_t)smem + piece * 1024);
  const char* gbase = reinterpret_cast<const char*>(base);
#define SE8_DMA(kt, slot)                                                                                                     \
  do {                                                                                                                        \
    uint32_t dp_ = dpk;                                                                                                       \
    asm volatile("" : "+v"(dp_));                                                                                             \
    const uint32_t row_ = (uint32_t)(min((kt) * kAK + (int)(dp_ & 0xffu), T - 1) * ld);                                       \
    const uint32_t ok_ = (row_ + (uint32_t)H) * 2u + (dp_ >> 8);                                                              \
    uint32_t keep_;                                                                                                           \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"      \
                 : "=&s"(keep_) : "v"(ok_), "s"(gbase), "s"(lds_piece + (uint32_t)((slot) * k8Slot)) : "memory");             \
    const uint32_t ov_ = (row_ + 2u * (uint32_t)H) * 2u + (dp_ >> 8);                                                         \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"      \
                 : "=&s"(keep_) : "v"(ov_), "s"(gbase), "s"(lds_piece + (uint32_t)((slot) * k8Slot + 8192)) : "memory");      \
  } while (0)

  if (!(SE_MHSAN_ABL & 1)) {
  SE8_DMA(0, 0);
  if (nkt > 1) SE8_DMA(1, 1);
  }

  // ---- Q fragments (B operand of S^T = K Q^T): lane -> query row q0 + l31, d = 16 s + 8 hh .. +7
  bf16x8 qf[4];
  {
    const int q = min(q0 + l31, T - 1);
    const uint16_t* qp = base + (size_t)q * ld + 8 * hh;
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
  }
  const f32x16 kZero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x16 o0, o1;                      // O^T d-blocks 0 / 1: col = query (lane & 31), row = d
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = 0.f, l_run = 0.f;
  bool slow = dscale < 0.f;           // wave-uniform: the speculative (no row maximum) path failed once; dscale < 0: never speculate (A/B switch)
  constexpr float kDefer = 8.f;
  // K fragment address of k-step s = kv_off(l31, 2 s + hh) = koff0 ^ (s << 5): 2 s and hh occupy disjoint bits of the chunk index, so the XOR with
  // the swizzle term commutes -- ONE address register instead of four (128 registers per lane)
  const int koff0 = kv_off(l31, hh);
  const int tq = (lane & 15) >> 2, tp = lane & 3, g1 = (lane >> 4) & 1;
  int voff[2][2];                     // [dblk][lo / hi]
#pragma unroll
  for (int dblk = 0; dblk < 2; ++dblk) {
    const int dcol = dblk * 32 + 16 * g1 + 4 * tp;
    voff[dblk][0] = 8192 + kv_off(4 * hh + tq, dcol >> 3) + (dcol & 7) * 2;
    voff[dblk][1] = 8192 + kv_off(4 * hh + tq + 8, dcol >> 3) + (dcol & 7) * 2;
  }

  // tile 0 landed (this wave's two pieces; tile 1's may still fly) -> publish
  if (nkt > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  SE8_BAR();

  const bool late = (wave & 4) != 0;
  // the tile's barrier: own pieces of tile kt + 1 (issued one tile ago) are in LDS once all but the two just issued have completed
#define SE8_SYNC()                                                                                                            \
  do {                                                                                                                        \
    if (!(SE_MHSAN_ABL & 1)) {                                                                                                \
      if (kt + 2 < nkt) asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    }                                                                                                                         \
    if (!(SE_MHSAN_ABL & 2)) SE8_BAR();                                                                                       \
  } while (0)
  int slot = 0;
  for (int kt = 0; kt < nkt; ++kt) {
    const char* t_s = smem + slot * k8Slot;
    const int slot1 = slot == k8Ring - 1 ? 0 : slot + 1, slot2 = slot1 == k8Ring - 1 ? 0 : slot1 + 1;      // (slot + 1), (slot + 2) mod ring
    if (kt + 2 < nkt && !(SE_MHSAN_ABL & 1)) SE8_DMA(kt + 2, slot2);       // the slot of tile kt - 2: every wave left it before the barrier that ended tile kt - 1
    // S^T = K Q^T of this tile + the key mask of a ragged last tile
    f32x16 s0, s1;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bf16x8 ka = (SE_MHSAN_ABL & 4) ? qf[s] : *reinterpret_cast<const bf16x8*>(t_s + (koff0 ^ (s << 5)));
      const bf16x8 kb_ = (SE_MHSAN_ABL & 4) ? qf[3 - s] : *reinterpret_cast<const bf16x8*>(t_s + (koff0 ^ (s << 5)) + 4096);
      s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, qf[s], s == 0 ? kZero16 : s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kb_, qf[s], s == 0 ? kZero16 : s1, 0, 0, 0);
    }
    if ((kt + 1) * kAK > len) {
      const int kbase = kt * kAK + 4 * hh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kbase + (r & 3) + 8 * (r >> 2);
        if (key >= len) s0[r] = -INFINITY;
        if (key + 32 >= len) s1[r] = -INFINITY;
      }
    }
    bf16x8 pf[2][2];
    bool spec_ok = false;
    if (!slow) {
      // SPECULATIVE tile (mhsa.hip): probabilities against the initial reference 0, no row maximum; the row sums tell whether it held
      float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float a0 = (SE_MHSAN_ABL & 8) ? s0[8 * s + j] * 0.5f + 1.0f : __builtin_amdgcn_exp2f(s0[8 * s + j]);
          const float a1 = (SE_MHSAN_ABL & 8) ? s1[8 * s + j] * 0.5f + 1.0f : __builtin_amdgcn_exp2f(s1[8 * s + j]);
          rs0 += a0;
          rs1 += a1;
          pf[0][s][j] = (__bf16)a0;
          pf[1][s][j] = (__bf16)a1;
        }
      const float rs = rs0 + rs1;
      const bool bad = !(rs < 0x1p60f) || (kt == 0 && rs < 0x1p-60f);
      if (!__any(bad)) {
        l_run += rs;
        spec_ok = true;
      } else {
        slow = true;
      }
    }
    if (!spec_ok) {
      float mx = fmaxf(s0[0], s1[0]);
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(fmaxf(mx, s0[r]), s1[r]);       /* v_max3_f32 */
      {
        const auto sw_ = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw_[0]), __uint_as_float(sw_[1]));
      }
      float m_new = ((mx - m_run) > kDefer) ? mx : m_run;
      if (kt == 0 && mx < -64.f) m_new = mx;        /* a first tile far below the initial reference 0 (later tiles cannot matter) */
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      const float mc = -m_new;
      float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float a0 = __builtin_amdgcn_exp2f(s0[r] + mc);
        const float a1 = __builtin_amdgcn_exp2f(s1[r] + mc);
        rs0 += a0;
        rs1 += a1;
        s0[r] = a0; s1[r] = a1;
      }
      l_run = fmaf(l_run, alpha, rs0 + rs1);
      m_run = m_new;
      if (__any(alpha != 1.0f)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          pf[0][s][j] = (__bf16)s0[8 * s + j];
          pf[1][s][j] = (__bf16)s1[8 * s + j];
        }
    }
    if (late) SE8_SYNC();             // the late half of every SIMD's waves: the barrier between the softmax and the PV products
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dblk = 0; dblk < 2; ++dblk) {
          const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) bf16x4*)(t_s + voff[dblk][0] + kb * 4096 + s * 2048));
          const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
              (__attribute__((address_space(3))) bf16x4*)(t_s + voff[dblk][1] + kb * 4096 + s * 2048));
          bf16x8 va = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          if (SE_MHSAN_ABL & 4) va = qf[2 * kb + s];
          if (dblk == 0) o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pf[kb][s], o0, 0, 0, 0);
          else o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, pf[kb][s], o1, 0, 0, 0);
        }
    if (!late) SE8_SYNC();            // the early half: at the tile's end
    slot = slot1;
  }
#undef SE8_SYNC
#undef SE8_DMA

  SE_CLKPROBE_END(clkprobe_mhsa);
  // ---- epilogue: O / l ; lane holds query q0 + l31, d = 32 dblk + (r&3) + 8 (r>>2) + 4 hh
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = 1.0f / l_tot;
  const int q = q0 + l31;
  if (q < T) {
    uint16_t* op = ctx + ((size_t)b * T + q) * H + head * kHD + 4 * hh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      uint2 w0 = make_uint2(pack_bf16x2(o0[4 * g] * inv, o0[4 * g + 1] * inv), pack_bf16x2(o0[4 * g + 2] * inv, o0[4 * g + 3] * inv));
      uint2 w1 = make_uint2(pack_bf16x2(o1[4 * g] * inv, o1[4 * g + 1] * inv), pack_bf16x2(o1[4 * g + 2] * inv, o1[4 * g + 3] * inv));
      *reinterpret_cast<uint2*>(op + 8 * g) = w0;
      *reinterpret_cast<uint2*>(op + 32 + 8 * g) = w1;
    }
  }
}

}  // namespace se

// mhsa.hip's launch site hands over the route's grid; the predicate is re-checked here: a call past the 31-bit limit fails, it is not re-routed
int se_mhsa_wave8_fwd_launch(const se::MhsaCall& call, dim3 grid, dim3 block, const uint16_t* qkv, const int32_t* lengths, uint16_t* ctx, float dscale,
                             hipStream_t st) {
  SE_REQUIRE(se::mhsa_wave8_prescaled_ok(call), "se_mhsaN: T * 3 H * 2 = %.0f bytes exceeds the 31-bit DMA offset", se::mhsa_wave8_block_bytes(call));
  hipLaunchKernelGGL(se::mhsa_wave8_fwd_kernel, grid, block, 0, st, qkv, lengths, call.T, call.heads * se::kHD, ctx, dscale);
  SE_LAUNCH_CHECK();
  return SE_OK;
}
