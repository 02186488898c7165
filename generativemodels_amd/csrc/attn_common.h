// Pieces shared by the attention kernels (GmAttnDesc / GmAttnBwdDesc themselves: include/gm_amd.h): attention.hip (register-staged, any dtype / head dim),
// attention_dma.hip (bf16, LDS-DMA), attention_wide.hip, the backward files and the decode step's kernels in decode_attention.hip and rows_gemm.hip.
#pragma once
#include "gm_common.h"

// key ranges of the split-KV single-query attention of the decode step (decode_attention.hip; the merge code of decode_common.h unrolls over it)
#define GM_DECODE_KV_SPLITS 16
// widest head the register-staged kernels serve in one pass (attention.hip), and the widest the sliced kernel serves (attention_wide.hip)
#define GM_ATTN_MAX_DH 256
#define GM_ATTN_WIDE_MAX_DH 1024

#ifdef __HIPCC__
// 256 < dh <= GM_ATTN_WIDE_MAX_DH, fp32 / bf16, after gm_attention_forward's descriptor checks (attention_wide.hip); 0 = launched
int gm_attn_wide_dispatch(const GmAttnDesc& d, hipStream_t st);
// The four lanes l15 + 16 * {0, 1, 2, 3} of a wave hold partial results of one MFMA column: max / sum over them by gfx950's lane-swap VALU
// instructions (v_permlane32_swap exchanges the wave's halves, v_permlane16_swap the odd and even 16-lane rows) instead of two ds_bpermute
// round trips through the LDS pipeline.  Every lane receives the same value, operands combined in a fixed order.
__device__ __forceinline__ float attn_quad_max(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float m = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float attn_quad_sum(float x) {
  auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  const float m = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(m), __float_as_uint(m), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// one 1 KB LDS-DMA piece: every lane's 16 bytes at gsrc land at lds_dst + 16 * lane (M0 saved and restored around the request)
__device__ __forceinline__ void attn_dma16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
// ... the same piece from a wave-uniform base (SGPR pair) + this lane's 32-bit byte offset: per-tile address arithmetic on the scalar unit
__device__ __forceinline__ void attn_dma16_s(const void* sbase, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_dst)
               : "memory");
}
// rows [L][ld] (channels [h * dh, (h + 1) * dh) per head) -> image[b * H + h][channel][position], zero beyond L, position order inside each
// 32-block = the order a 16x16x32 MFMA consumes two 16-row accumulator fragments (attention_dma.hip: vt_pack_kernel); dh a multiple of 64
void gm_attn_pack_transposed(const bf16_raw* rows, long long ld, bf16_raw* image, int B, int H, int L, int L_pad, int dh, hipStream_t st);
// ... three tensors in one launch (3 * B * H <= 65535)
void gm_attn_pack_transposed3(const bf16_raw* const rows[3], const long long ld[3], bf16_raw* const image[3], const int L[3], const int L_pad[3], int B, int H, int dh,
                              hipStream_t st);
#endif
