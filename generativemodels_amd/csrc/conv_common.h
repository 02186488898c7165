// Shared pieces of the implicit-GEMM convolution kernels (conv.hip: generic geometry; conv_fast.hip: the stride-1 hot path).
#pragma once
#include "gm_common.h"

// ---- host predicates shared by the eligibility tests of the LDS-DMA kernels ---------------------------------------------------------------------------------
// the statistics form of a GroupNorm prologue (GmConvDesc.pre_stats / GmGnTables): one or two 16-byte aligned sources of 1 .. GM_GN_SHORT_MAX_ROWS rows whose
// channels add up to cin; no second source, no second channel count.  (Each consumer adds the bounds of its own LDS tables.)
static inline bool gm_gn_stats_form_ok(const double* const stats[2], const int S[2], const int C[2], int cin) {
  return stats[0] != nullptr && S[0] >= 1 && S[0] <= GM_GN_SHORT_MAX_ROWS && C[0] > 0 &&
         ((stats[1] == nullptr && C[1] == 0 && C[0] == cin) || (stats[1] != nullptr && S[1] >= 1 && S[1] <= GM_GN_SHORT_MAX_ROWS && C[1] > 0 && C[0] + C[1] == cin)) &&
         gm_aligned16(stats[0]) && gm_aligned16(stats[1]);
}
// the second input source of a virtual channel concatenation: same geometry, chunk-aligned split inside C_in, vector-aligned pitch and base
static inline bool gm_conv_second_source_ok(const GmConvDesc* d, int bk, int vecw) {
  return d->x2 == nullptr || (d->cin_split > 0 && d->cin_split < d->Cin && d->cin_split % bk == 0 && d->x2_ld % vecw == 0 && gm_aligned16(d->x2));
}
// the fused 1x1 shortcut: packed weights and one or two sources of whole K chunks with vector-aligned pitch and base
static inline bool gm_conv_shortcut_ok(const GmConvDesc* d, int bk, int vecw) {
  if (!d->skip_x[0]) return true;
  for (int i = 0; i < 2; ++i)
    if (d->skip_x[i] && !(d->skip_cin[i] > 0 && d->skip_cin[i] % bk == 0 && d->skip_ld[i] % vecw == 0 && gm_aligned16(d->skip_x[i]))) return false;
  return d->skip_w != nullptr;
}

// slot count of the zero-initialised, atomically accumulated statistic tables the BACKWARD kernels still use ([GM_STAT_SLOTS][N][C][2];
// gm_gn_bwd_stats, gm_layernorm_bwd).  The forward tables (convolution epilogues, gm_gn_channel_stats) hold one partial per tile instead.
#define GM_STAT_SLOTS 64

#define CONV_ROWB 80  // LDS row pitch in bytes: 64 B of operands + 16 B pad

template <typename T> struct ConvTraits;
template <> struct ConvTraits<bf16_raw> { static constexpr int BK = 32; static constexpr int VECW = 8; };
template <> struct ConvTraits<float> { static constexpr int BK = 16; static constexpr int VECW = 4; };

__device__ __forceinline__ float conv_act(float v, int act, bool precise) {
  switch (act) {
    case 1: return precise ? gm_silu_precise(v) : gm_silu(v);
    case 2: return fmaxf(v, 0.f);
    default: return v;
  }
}
// The activation of a whole register vector with the (wave-uniform, run-time) kind tested ONCE.  `for i: v[i] = conv_act(v[i], act, ..)` made
// hipcc emit the switch PER ELEMENT: every element became its own basic block -- s_cmp / s_cbranch, then the fully dependent chain v_mul ->
// v_exp -> v_add -> v_rcp -> v_mul with the transcendental latencies exposed and nothing to interleave (round-3 ISA read: the out head's fused
// GroupNorm + SiLU prologue cost 0.15 of its 0.26 ms, the in-LDS prologue of the LDS-DMA convolution as much as a separate pass over HBM).  Here
// the N chains of a vector sit in one straight-line block and the scheduler interleaves them.
template <int N>
__device__ __forceinline__ void conv_act_vec(float (&v)[N], int act, bool precise) {
  if (act == 1) {
    if (precise) {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = gm_silu_precise(v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = gm_silu(v[i]);
    }
  } else if (act == 2) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = fmaxf(v[i], 0.f);
  }
}
__device__ __forceinline__ float conv_post_act(float v, int act) {
  switch (act) {
    case 1: return fmaxf(v, 0.f);
    case 2: return tanhf(v);
    case 3: return 1.0f / (1.0f + expf(-v));
    case 4: return gm_silu_precise(v);
    case 5: return v > 0.f ? v : 0.01f * v;
    case 6: return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));  // nn.GELU() (exact), MONAI MLPBlock
    default: return v;
  }
}

template <typename T> struct Mma;
template <> struct Mma<bf16_raw> {
  static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mma<float> {
  static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
  }
};

