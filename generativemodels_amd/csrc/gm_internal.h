// Cross-file helpers of libgmamd.so that are NOT part of the public interface (include/gm_amd.h), each declared once, grouped by the file that defines
// them.  gm_common.h includes this header, so the defining file sees its own declaration and the compiler holds definition, declaration and every caller to
// one signature: these are extern "C" (no mangling), and a disagreement would otherwise link cleanly.  A helper gm_amd.h declares gets no line here.
#pragma once
#include "gm_amd.h"

extern "C" {

// ---- capi.cpp
void gm_set_error(const char* where, int code, const char* msg);

// ---- conv_fast.hip: the stride-1 register-staged kernels (cfg 5 .. 10; variant = cfg - 4)
long long gm_conv_fast_lds_bytes(const GmConvDesc* d, int bn);
long long gm_conv_fast_max_patch(int variant);
int gm_conv_fast_variant_geometry(int variant, int* voxels, int* channels, int* threads);
int gm_conv_fast_launch(const GmConvDesc* dp, int variant, unsigned nblocks, void* stream);

// ---- conv_dma.hip: the LDS-DMA kernels (cfg 11, 14 .. 19); launch_part<k> = the instantiations of the translation unit built with GM_DMA_PART = k
long long gm_conv_dma_lds_bytes(int variant);
int gm_conv_dma_variant(int cfg);
int gm_conv_dma_eligible(const GmConvDesc* d);
int gm_conv_dma_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_dma_launch_part0(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_dma_launch_part1(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_dma_launch_part2(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_dma_launch_part3(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_dma_launch_part4(const GmConvDesc* dp, unsigned nblocks, void* stream);

// ---- conv_sk.hip: the K slices of a split cfg 11 launch
int gm_conv_sk_eligible(const GmConvDesc* d);
int gm_conv_sk_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);

// ---- conv_sn.hip: small volumes and images, K-complete (cfg 24 / 25)
int gm_conv_sn_eligible(const GmConvDesc* d);
long long gm_conv_sn_lds_bytes(int cfg);
int gm_conv_sn_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);

// ---- conv_edge.hip: the HBM-bound end convolutions (cfg 12: C_in <= 4; cfg 13 / 20: C_out == 1)
int gm_conv_cin_eligible(const GmConvDesc* d);
long long gm_conv_cin_lds_bytes(const GmConvDesc* d);
int gm_conv_cin_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_cout1_eligible(const GmConvDesc* d);
long long gm_conv_cout1_lds_bytes(void);
int gm_conv_cout1_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);
int gm_conv_cout1m_eligible(const GmConvDesc* d);
long long gm_conv_cout1m_lds_bytes(const GmConvDesc* d);
int gm_conv_cout1m_launch(const GmConvDesc* dp, unsigned nblocks, void* stream);

// ---- attention_dma.hip: 0 = the LDS-DMA kernel took the launch
int gm_attention_dma_try(const GmAttnDesc* dp, void* stream);

// ---- transformer_ops.hip: gm_embed_tokens with the position read from device memory (pos_dev != NULL)
int gm_embed_tokens_dev(const long long* indices, const void* token_weight, const void* position_weight, void* out, long long batch, int seq_len, int C,
                        int pos0, int num_tokens, int max_positions, int dtype, const int* pos_dev, void* stream);

// ---- rows_gemm.hip: the row GEMMs with the decode step's fused prologues and epilogues (decode_step.hip), and the fused MLP
int gm_linear_rows_takes_ksplit(int rows, int cin, int dtype);
// What the decode step adds to a plain GmRowsDesc (whose x is NULL with a partial source); every group is off when its first member is 0 / null.
struct GmRowsFused {
  const float* ln_g; const float* ln_b; float ln_eps;  // x <- LayerNorm(x) * g + b before the GEMM
  void* y1; void* y2; long long y12_ld; int split;     // cout = 3 * split: channels [split, 2 split) -> y1, [2 split, 3 split) -> y2 (row pitch y12_ld) ...
  const int* off_dev; long long off_mul;               // ... advanced by (*off_dev) * off_mul elements at run time (KV-cache row = position)
  const float* kv_ws; int kv_ns, kv_dh;                // x = the merge of the split-KV attention partials (gm_attention_decode_split, merge 0): kv_ns ranges, head size kv_dh
  const float* mlp_p; int mlp_nj; const void* mlp_x1; const float* mlp_b2; void* mlp_x0;  // x = x1 + b2 + sum_j P[j] over gm_mlp_rows's nj partials, stored to mlp_x0 when given
};
// gm_rows_gemm with those extras (f NULL: none).  The two partial sources exist in the K-split kernel only: a geometry outside it is an error.
int gm_rows_gemm_fused(const GmRowsDesc* d, const GmRowsFused* f, void* stream);
// The decode step's MLP as one launch leaving (M / 64) * rows * C fp32 K-slice partials in P for GmRowsFused.mlp_p; fusable: 1 when both kernels take the geometry.
int gm_mlp_rows_fusable(int rows, int C, int M, int dtype);
int gm_mlp_rows(const void* x, const float* ln_g, const float* ln_b, float ln_eps, const void* w1, const float* b1, const void* w2, float* P, int rows,
                int C, int M, int act, int dtype, void* stream);

// ---- decode_attention.hip: one query per (batch, head) over a KV cache -- single launch, split over key ranges, or fused behind the q | k | v projection
int gm_attention_decode_try(const GmAttnDesc* dp, void* stream);
int gm_attention_decode_dev(const GmAttnDesc* dp, const int* lk_dev, void* stream);
int gm_attention_decode_split(const GmAttnDesc* dp, const int* lk_dev, float* ws, int nsplit, int merge, int cap, void* stream);
// LayerNorm + q | k | v + one key range of the single-query attention in one launch (qkv_attn_rows_kernel, which takes the struct by value)
struct QkvAttnArgs {
  const void* x0;                                                       // [B][C] rows, or null with the partial source below
  const float* mlp_p; int mlp_nj; const void* mlp_x1; const float* mlp_b2; void* x0_out;
  const float* ln_g; const float* ln_b; float ln_eps;
  const void* w; const float* bias;                                     // packed [chunk][3C pad 16][BK]; fp32 [3C] or null
  void* kcache; void* vcache;                                           // [B][cap][C]
  int B, H, C, dh, cap, pos; const int* pos_dev;
  float scale; float* ws; int chunk, sc_elems;
};
int gm_qkv_attn_rows(const QkvAttnArgs* ap, int dtype, void* stream);
int gm_qkv_attn_rows_plan(const QkvAttnArgs* ap, int dtype, int* ng, int* um);  // which instantiation would take it; launches nothing
// LayerNorm + one head's q projection + the 1 x Lc attention over projected context keys / values in one launch (cross_attn_rows_kernel, by value)
struct CrossAttnArgs {
  const void* x;                                                        // [B][C] residual-stream rows
  const float* ln_g; const float* ln_b; float ln_eps;
  const void* w; const float* bias;                                     // packed [chunk][C pad 16][BK]; fp32 [C] or null
  const void* ck; const void* cv;                                       // [B][Lc][C]
  void* o;                                                              // [B][C] attention output (before the out-projection)
  int B, H, C, dh, Lc;
  float scale; int sc_elems;
};
int gm_cross_attn_rows(const CrossAttnArgs* ap, int dtype, void* stream);        // 1 = launched, 0 = not this kernel's case, < 0 = error
int gm_cross_attn_rows_plan(const CrossAttnArgs* ap, int dtype, int* ng, int* um);  // 1 and the instantiation that would take it, or 0; launches nothing

}  // extern "C"
