// Device helpers of the fp32-MFMA flash backward kernels (attention_bwd.hip, with and without the causal mask): 4-element loads / stores in either storage
// dtype, the staging of a 32-row streamed tile as fp32 into LDS, and the two MFMA contractions over it (tile rows x own rows, tile columns
// accumulated into own rows).  The work-group's OWN rows are MFMA columns, one per lane (attention_bwd.hip's header comment).
#pragma once
#include "attn_common.h"

template <typename T> __device__ __forceinline__ float4 ab_load4(const T* p);
template <> __device__ __forceinline__ float4 ab_load4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
template <> __device__ __forceinline__ float4 ab_load4<bf16_raw>(const bf16_raw* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void ab_store4(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void ab_store4<float>(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }
template <> __device__ __forceinline__ void ab_store4<bf16_raw>(bf16_raw* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}

#define AB_ROWS 32  // rows of a streamed tile (two 16-row fragments)
#define AB_OWN 64   // own rows of a work-group (4 waves x 16 MFMA columns)

// stage `AB_ROWS` rows [row0, row0 + AB_ROWS) of a [L][ld] operand (channels [0, DH)) as fp32 into lds[row][DH + 4]; rows >= L are zero
template <typename T, int DH>
__device__ __forceinline__ void ab_stage(const T* base, long long ld, int row0, int L, float* lds, int tid) {
  constexpr int PITCH = DH + 4;
  for (int it = tid; it < AB_ROWS * (DH / 4); it += (int)blockDim.x) {
    const int row = it / (DH / 4), c4 = it % (DH / 4);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row0 + row < L) v = ab_load4<T>(base + (long long)(row0 + row) * ld + c4 * 4);
    *reinterpret_cast<float4*>(lds + row * PITCH + c4 * 4) = v;
  }
}

// acc[f][r] (f = 16-row fragment of the tile, r) += sum_c tile[f*16 + l15][c] * own[c]: A = tile rows, B = own-row fragments
template <int DH>
__device__ __forceinline__ void ab_rows_dot(const float* lds, const float4 (&own)[DH / 16], f32x4_t (&acc)[2], int l15, int qg) {
  constexpr int PITCH = DH + 4;
#pragma unroll
  for (int s = 0; s < DH / 16; ++s)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float4 a = *reinterpret_cast<const float4*>(lds + (f * 16 + l15) * PITCH + s * 16 + qg * 4);
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, own[s].x, acc[f], 0, 0, 0);
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, own[s].y, acc[f], 0, 0, 0);
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, own[s].z, acc[f], 0, 0, 0);
      acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, own[s].w, acc[f], 0, 0, 0);
    }
}

// out[d][r] (channel c0 + d*16 + 4qg + r of this lane's own row) += sum_rows tile[row][c0 + d*16 + l15] * w[row]: A = tile^T read element-wise
// from the natural tile, B = the per-row weights held in the accumulator layout (w[f][i] belongs to tile row f*16 + 4qg + i)
template <int DH, int DF>
__device__ __forceinline__ void ab_cols_acc(const float* lds, const f32x4_t (&w)[2], f32x4_t (&out)[DF], int c0, int l15, int qg) {
  constexpr int PITCH = DH + 4;
#pragma unroll
  for (int d = 0; d < DF; ++d)
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = lds[(f * 16 + qg * 4 + i) * PITCH + c0 + d * 16 + l15];
        out[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[f][i], out[d], 0, 0, 0);
      }
}

template <typename T, int DH>
__device__ __forceinline__ void ab_load_own(const T* row, bool ok, float4 (&own)[DH / 16], int qg) {
#pragma unroll
  for (int s = 0; s < DH / 16; ++s) own[s] = ok ? ab_load4<T>(row + s * 16 + qg * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
