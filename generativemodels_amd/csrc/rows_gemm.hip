// The row GEMMs: y[rows][cout] = post(pre(x)[rows][cin] W^T + b) (+ res) without the tiled convolution's K-chunk loop over LDS (two barriers per
// chunk: 10-30 us on a few rows, 20 us per launch on a few thousand tokens).  Every 1x1 convolution over tokens, every nn.Linear, the timestep MLP
// and the decode step's projections (reference: nn.Linear in transformer blocks, time_embed / time_emb_proj, diffusion_model_unet.py:1758-1760).
//   linear_rows_kernel         one wave per 16 rows x 16 output channels streams its weight rows global -> registers -> MFMA (no LDS, no barrier)
//   token_gemm_wide_kernel     many token rows: a wave owns 16 rows x NB * 16 channels; the GroupNorm prologue from (scale, shift) or statistic tables
//   linear_rows_ksplit_kernel  at most 16 rows and a long K: the K chunks dealt to the four waves; prologues that merge the producer's partials
//   mlp_rows_kernel            the decode step's MLP in one launch, leaving K-slice partials for the K-split kernel's prologue
// then the host side: one validation, one route decision (gm_rows_gemm_route), one launcher behind gm_rows_gemm / gm_rows_gemm_fused.
#include <cstdlib>
#include "conv_common.h"
#include "decode_common.h"

// optional extras of the small-row GEMM: a LayerNorm over the input row as its prologue (transformer pre-norm blocks) and a split of
// the output channels over three destinations (the stacked q | k | v projection writing k and v straight into the KV caches)
struct LinearRowsExtra {
  const float* ln_g; const float* ln_b; float ln_eps;  // ln_g != null: x <- LayerNorm(x) * g + b before the GEMM
  void* y1; void* y2; long long y12_ld; int split;     // split > 0: channels [split, 2*split) -> y1, [2*split, 3*split) -> y2 (row pitch y12_ld)
  const int* off_dev; long long off_mul;               // y1 / y2 are advanced by (*off_dev) * off_mul elements at run time (KV-cache row = position)
  const float* kv_ws; int kv_dh;                       // K-split kernel STAGE 1: x = merge of the split-KV attention partials (head size kv_dh)
  const float* mlp_p; int mlp_nj; const void* mlp_x1; const float* mlp_b2; void* mlp_x0;  // K-split kernel STAGE 2: x = x1 + b2 + sum_j P[j]
  const float* pre_scale; const float* pre_shift; long long ss_ld; int rows_per_sample;   // linear_rows_kernel: x <- x * scale[n][c] + shift[n][c], n = row / rows_per_sample
  // linear_rows_kernel, stacked q | k | v projection of an attention block: output channels >= vt_c0 (the V columns) are ALSO stored into the
  // transposed, key-permuted image VT[sample * H + head][channel][position] the LDS-DMA attention kernel consumes (attention_dma.hip:
  // vt_pack_kernel's layout; rows_per_sample = tokens per sample = the image's row pitch, a multiple of 64): no separate pack launch
  void* vt; int vt_c0; int vt_dh;
  // token_gemm_wide_kernel<.., GN = true>: the per-sample GroupNorm of x given as the statistic tables of its producer(s) -- finalised in the kernel's prologue
  // (GmRowsDesc.gn; the shared short-table order of gm_common.h: bit-identical to gm_gn_finalize_channels + the (scale, shift) form)
  const double* gn_stats[2]; int gn_S[2]; int gn_C[2]; const float* gn_gamma; const float* gn_beta; float gn_eps; int gn_groups; int gn_N;
};

template <typename T>
__global__ __launch_bounds__(256) void linear_rows_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ w,
                                                         const float* __restrict__ bias, const T* __restrict__ res, long long res_ld,
                                                         T* __restrict__ y, long long y_ld, int rows, int cin, int cout, int pre_act,
                                                         int post_act, LinearRowsExtra ex) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW;
  constexpr bool PRECISE = sizeof(T) == 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int cout_pad = (cout + 15) & ~15;
  const int co0 = (blockIdx.x * 4 + wave) * 16;
  if (co0 >= cout_pad) return;  // wave-uniform
  const int r0 = blockIdx.y * 16;
  const int row = r0 + l15;
  const bool row_ok = row < rows;
  const int nchunks = (cin + BK - 1) / BK;
  const T* wrow = w + ((long long)(co0 + l15)) * BK + q * VECW;      // + chunk * cout_pad * BK
  const T* xrow = x + (long long)(row_ok ? row : 0) * x_ld + q * VECW;  // + chunk * BK; only dereferenced under its `ok` guard
  // ---- LayerNorm statistics of this lane's row: the 4 lanes sharing l15 cover the row between them (two passes: mean, then the
  //      centred second moment, like the reference's fp32 computation) ------------------------------------------------------------
  float mean = 0.f, rstd = 1.f;
  if (ex.ln_g) {
    float sum = 0.f;
    for (int c = 0; c < nchunks; ++c) {
      if (c * BK + q * VECW + VECW <= cin) {
        float v[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(xrow + c * BK), v);
#pragma unroll
        for (int i = 0; i < VECW; ++i) sum += v[i];
      }
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    mean = sum / (float)cin;
    float sq = 0.f;
    for (int c = 0; c < nchunks; ++c) {
      if (c * BK + q * VECW + VECW <= cin) {
        float v[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(xrow + c * BK), v);
#pragma unroll
        for (int i = 0; i < VECW; ++i) sq += (v[i] - mean) * (v[i] - mean);
      }
    }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    rstd = 1.0f / sqrtf(sq / (float)cin + ex.ln_eps);
  }
  // bias and residual of this lane's outputs: requested up front through substitute addresses (round 3: a conditional load is a branch + a wait)
  float bia[4], rsd[4];
  {
    const float* bsrc = bias ? bias : reinterpret_cast<const float*>(w);
    const T* rsrc = res ? res + (long long)(row_ok ? row : 0) * res_ld : w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + 4 * q + i;
      bia[i] = bsrc[bias ? (co < cout ? co : cout - 1) : 0];
      rsd[i] = ElemIO<T>::ld(rsrc + (res ? (co < cout ? co : cout - 1) : 0));
    }
  }
  f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  constexpr int U = 4;
  for (int c0 = 0; c0 < nchunks; c0 += U) {
    uint4 wf[U], xf[U];
    float asc[U][VECW], ash[U][VECW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u < nchunks ? c0 + u : nchunks - 1;  // clamped: the duplicate is discarded below
      wf[u] = *reinterpret_cast<const uint4*>(wrow + (long long)c * cout_pad * BK);
      const bool ok = row_ok & (c * BK + q * VECW + VECW <= cin);  // host: cin % VECW == 0
      // masked lanes read the first vector of the tensor: xrow + 0 is q * VECW elements into the row, which lies beyond a row (and, in
      // the last row, beyond the allocation) whenever cin < 4 * VECW -- a faulting read even though its value is discarded
      const uint4 v = *reinterpret_cast<const uint4*>(ok ? xrow + c * BK : x);
      xf[u] = make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
      if (ex.pre_scale) {  // (uniform) per-sample GroupNorm affine of this lane's channels: vector loads at a clamped offset, values selected below
        const int cb = c * BK + q * VECW + VECW <= cin ? c * BK + q * VECW : 0;
        const long long off = (long long)((row_ok ? row : 0) / ex.rows_per_sample) * ex.ss_ld + cb;
#pragma unroll
        for (int i = 0; i < VECW; i += 4) {
          const float4 a = *reinterpret_cast<const float4*>(ex.pre_scale + off + i), b2 = *reinterpret_cast<const float4*>(ex.pre_shift + off + i);
          asc[u][i] = a.x; asc[u][i + 1] = a.y; asc[u][i + 2] = a.z; asc[u][i + 3] = a.w;
          ash[u][i] = b2.x; ash[u][i + 1] = b2.y; ash[u][i + 2] = b2.z; ash[u][i + 3] = b2.w;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c0 + u >= nchunks) break;
      uint4 b = xf[u];
      if (pre_act || ex.ln_g || ex.pre_scale) {
        float v[VECW];
        Vec16<T>::unpack(b, v);
        if (ex.pre_scale) {
          const bool okc = row_ok & ((c0 + u) * BK + q * VECW + VECW <= cin);
#pragma unroll
          for (int i = 0; i < VECW; ++i) v[i] = okc ? v[i] * asc[u][i] + ash[u][i] : 0.f;
        }
        if (ex.ln_g) {
          const int cbase = (c0 + u) * BK + q * VECW;
          const bool ok = row_ok & (cbase + VECW <= cin);
#pragma unroll
          for (int i = 0; i < VECW; ++i) v[i] = ok ? (v[i] - mean) * rstd * ex.ln_g[cbase + i] + (ex.ln_b ? ex.ln_b[cbase + i] : 0.f) : 0.f;
        }
        if (pre_act) {
          conv_act_vec(v, pre_act, PRECISE);
        }
        b = Vec16<T>::pack(v);
      }
      Mma<T>::run(wf[u], b, acc);
    }
  }
  // D layout: column = row l15, rows = output channels co0 + 4q + i
  if (!row_ok) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co0 + 4 * q + i;
    if (co < cout) {
      float v = acc[i] + (bias ? bia[i] : 0.f);
      v = conv_post_act(v, post_act);
      if (res) v += rsd[i];
      if (ex.split > 0 && co >= ex.split) {
        T* dst = reinterpret_cast<T*>(co < 2 * ex.split ? ex.y1 : ex.y2) + (ex.off_dev ? (long long)(*ex.off_dev) * ex.off_mul : 0);
        ElemIO<T>::st(dst + (long long)row * ex.y12_ld + (co - (co < 2 * ex.split ? ex.split : 2 * ex.split)), v);
      } else {
        ElemIO<T>::st(y + (long long)row * y_ld + co, v);
        if (ex.vt && co >= ex.vt_c0) {
          const int cch = co - ex.vt_c0, L = ex.rows_per_sample;
          const int smp = row / L, key = row - smp * L;
          const int pos = (key & ~31) + ((key & 15) >> 2) * 8 + ((key >> 4) & 1) * 4 + (key & 3);  // key = blk*32 + half*16 + qq*4 + r -> blk*32 + qq*8 + half*4 + r
          const int heads = (cout - ex.vt_c0) / ex.vt_dh;
          ElemIO<T>::st(reinterpret_cast<T*>(ex.vt) + ((long long)(smp * heads + cch / ex.vt_dh) * ex.vt_dh + cch % ex.vt_dh) * L + pos, v);
        }
      }
    }
  }
}

// The same GEMM for MANY token rows (round 6): y = post_act(act(x * scale[n] + shift[n]) W^T + b) (+ res) with a wave owning 16 rows x NB * 16 output channels.
// linear_rows_kernel gives every 16-channel block of a row group its own wave: each re-reads the group's x rows (and re-applies the GroupNorm affine) and
// stores its results two bytes at a time.  At 16 384 rows (the q | k | v projections of BASELINE configs[0]'s attention blocks: 16 x 32 x 32 tokens, 64 -> 192)
// that is 12 passes over x and 3 072 work-groups for 0.4 GFLOP.  Here the x fragment of a K chunk is loaded and transformed ONCE per NB blocks, the four waves
// of a work-group take four consecutive row groups (the weight fragments they share meet in the CU's L1), and a lane stores its four consecutive channels as
// one vector.  Same accumulation order per output (K chunks in order, one MFMA each) as linear_rows_kernel: bit-identical results.  C_in a multiple of the MFMA
// K step; affine prologue, pre-/post-activation, residual and the V^T image as there.
template <typename T, int NB, bool GN>
__global__ __launch_bounds__(256) void token_gemm_wide_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ w, const float* __restrict__ bias,
                                                             const T* __restrict__ res, long long res_ld, T* __restrict__ y, long long y_ld, int rows, int cin,
                                                             int cout, int pre_act, int post_act, LinearRowsExtra ex) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW;
  constexpr bool PRECISE = sizeof(T) == 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int cout_pad = (cout + 15) & ~15;
  const int co0 = blockIdx.x * (16 * NB);
  const int r0 = (blockIdx.y * 4 + wave) * 16;
  // ---- GN: (scale | shift) of the work-group's sample over all input channels, from the statistic tables (every thread takes part: before any wave leaves) -----
  extern __shared__ __attribute__((aligned(16))) char gn_smem[];  // [scale[cin] | shift[cin]] fp32, [cin] fp64 (sum, sum of squares)
  if constexpr (GN) {
    float* tab = reinterpret_cast<float*>(gn_smem);
    double* csum = reinterpret_cast<double*>(gn_smem + 2 * (size_t)cin * 4);
    const int n = (blockIdx.y * 64) / ex.rows_per_sample;  // host: rows_per_sample % 64 == 0 -- one sample per work-group
    gn_short_table<256>(tab, cin, csum, 0, cin, 0, cin, cin / ex.gn_groups, ex.gn_stats[0], ex.gn_S[0], ex.gn_C[0], ex.gn_stats[1], ex.gn_S[1], ex.gn_C[1], ex.gn_N, n,
                        (long long)ex.rows_per_sample, ex.gn_eps, ex.gn_gamma, ex.gn_beta, threadIdx.x);
  }
  if (r0 >= rows) return;  // wave-uniform
  const int row = r0 + l15;
  const bool row_ok = row < rows;
  const int rowc = row_ok ? row : rows - 1;
  const int nchunks = cin / BK;  // host: cin % BK == 0
  const T* xrow = x + (long long)rowc * x_ld + q * VECW;
  // block nb of this wave: channels co0 + 16 nb .. + 15; blocks beyond the padded panel re-read the last one and are dropped at the store
  int wblk[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) wblk[nb] = co0 + 16 * nb < cout_pad ? co0 + 16 * nb : cout_pad - 16;
  const T* wrow = w + (long long)l15 * BK + q * VECW;  // + (chunk * cout_pad + block channel) * BK
  const long long aoff = ex.pre_scale ? (long long)(rowc / ex.rows_per_sample) * ex.ss_ld + q * VECW : 0;
  // bias / residual of this lane's outputs, requested up front at clamped addresses
  float bia[NB][4];
  uint2 rsd[NB];
  const bool vec4 = (cout & 3) == 0 && (y_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & (4 * sizeof(T) - 1)) == 0 &&
                    (!res || ((res_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(res) & (4 * sizeof(T) - 1)) == 0));
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = wblk[nb] + 4 * q + i;
      bia[nb][i] = bias ? bias[co < cout ? co : cout - 1] : 0.f;
    }
    rsd[nb] = make_uint2(0u, 0u);
    if (sizeof(T) == 2 && res && vec4) {
      const int co = wblk[nb] + 4 * q;
      rsd[nb] = *reinterpret_cast<const uint2*>(res + (long long)rowc * res_ld + (co + 3 < cout ? co : 0));
    }
  }
  f32x4_t acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  constexpr int U = 2;
  for (int c0 = 0; c0 < nchunks; c0 += U) {
    uint4 wf[U][NB], xf[U];
    float asc[U][VECW], ash[U][VECW];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u < nchunks ? c0 + u : nchunks - 1;  // clamped: the duplicate is discarded below
      xf[u] = *reinterpret_cast<const uint4*>(xrow + c * BK);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wf[u][nb] = *reinterpret_cast<const uint4*>(wrow + ((long long)c * cout_pad + wblk[nb]) * BK);
      if (GN) {
        const float* tab = reinterpret_cast<const float*>(gn_smem) + c * BK + q * VECW;
#pragma unroll
        for (int i = 0; i < VECW; i += 4) {
          const float4 a = *reinterpret_cast<const float4*>(tab + i), b2 = *reinterpret_cast<const float4*>(tab + cin + i);
          asc[u][i] = a.x; asc[u][i + 1] = a.y; asc[u][i + 2] = a.z; asc[u][i + 3] = a.w;
          ash[u][i] = b2.x; ash[u][i + 1] = b2.y; ash[u][i + 2] = b2.z; ash[u][i + 3] = b2.w;
        }
      } else if (ex.pre_scale) {  // (uniform)
#pragma unroll
        for (int i = 0; i < VECW; i += 4) {
          const float4 a = *reinterpret_cast<const float4*>(ex.pre_scale + aoff + c * BK + i), b2 = *reinterpret_cast<const float4*>(ex.pre_shift + aoff + c * BK + i);
          asc[u][i] = a.x; asc[u][i + 1] = a.y; asc[u][i + 2] = a.z; asc[u][i + 3] = a.w;
          ash[u][i] = b2.x; ash[u][i + 1] = b2.y; ash[u][i + 2] = b2.z; ash[u][i + 3] = b2.w;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c0 + u >= nchunks) break;
      uint4 b = row_ok ? xf[u] : make_uint4(0u, 0u, 0u, 0u);
      if (pre_act || ex.pre_scale || GN) {
        float v[VECW];
        Vec16<T>::unpack(b, v);
        if (ex.pre_scale || GN) {
#pragma unroll
          for (int i = 0; i < VECW; ++i) v[i] = row_ok ? v[i] * asc[u][i] + ash[u][i] : 0.f;
        }
        if (pre_act) conv_act_vec(v, pre_act, PRECISE);
        b = Vec16<T>::pack(v);
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) Mma<T>::run(wf[u][nb], b, acc[nb]);
    }
  }
  if (!row_ok) return;
  // D layout: column = row l15, rows = output channels block + 4q + i
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (co0 + 16 * nb >= cout_pad) break;  // (uniform)
    const int cob = co0 + 16 * nb + 4 * q;
    float o[4];
    float rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (res) {
      if (sizeof(T) == 2 && vec4) {
        rs[0] = __uint_as_float(rsd[nb].x << 16); rs[1] = __uint_as_float(rsd[nb].x & 0xffff0000u);
        rs[2] = __uint_as_float(rsd[nb].y << 16); rs[3] = __uint_as_float(rsd[nb].y & 0xffff0000u);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[i] = cob + i < cout ? ElemIO<T>::ld(res + (long long)row * res_ld + cob + i) : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[nb][i] + (bias ? bia[nb][i] : 0.f);
      v = conv_post_act(v, post_act);
      if (res) v += rs[i];
      o[i] = v;
    }
    if (vec4) {
      if (cob < cout) {
        if (sizeof(T) == 2) *reinterpret_cast<uint2*>(y + (long long)row * y_ld + cob) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        else *reinterpret_cast<float4*>(y + (long long)row * y_ld + cob) = make_float4(o[0], o[1], o[2], o[3]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (cob + i < cout) ElemIO<T>::st(y + (long long)row * y_ld + cob + i, o[i]);
    }
    if (ex.vt && cob + 3 >= ex.vt_c0) {
      const int L = ex.rows_per_sample, smp = row / L, key = row - smp * L;
      const int pos = (key & ~31) + ((key & 15) >> 2) * 8 + ((key >> 4) & 1) * 4 + (key & 3);  // key = blk*32 + half*16 + qq*4 + r -> blk*32 + qq*8 + half*4 + r
      const int heads = (cout - ex.vt_c0) / ex.vt_dh;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cch = cob + i - ex.vt_c0;
        if (cch >= 0 && cob + i < cout)
          ElemIO<T>::st(reinterpret_cast<T*>(ex.vt) + ((long long)(smp * heads + cch / ex.vt_dh) * ex.vt_dh + cch % ex.vt_dh) * L + pos, o[i]);
      }
    }
  }
}

// rows from which the wide form takes the affine token GEMMs (0 = never), and its blocks per wave: tools / tests pin them, the defaults are the measured ones
// (nb 0 = by row count: 4 blocks per wave from 8 192 rows, 2 below -- MI355X, profiles/r06_token_gemm_wide_ab.txt: 16 384 x 64 -> 192 runs best at 3-4, 4 096 x 128 -> 384 at 2)
static int gm_token_gemm_wide_rows = 2048, gm_token_gemm_wide_nb = 0;
extern "C" void gm_token_gemm_set_wide(int min_rows, int nb) {
  gm_token_gemm_wide_rows = min_rows < 0 ? 2048 : min_rows;
  gm_token_gemm_wide_nb = (nb == 2 || nb == 3 || nb == 4) ? nb : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Round 3: the decode step's GEMMs re-built around ONE rule -- every global load of a launch is issued before the first wait.  A launch of
// these kernels is a handful of work-groups on an idle chip; its duration is the ~4.3 us every launch costs on this stack plus one L2 round
// trip (0.2-0.5 us at the clocks such a load runs at) per DEPENDENT load.  The round-2 kernel above spends 17-25 round trips per launch:
// hipcc branches around every conditional load (`ok ? p[i] : 0`, `bias ? bias[co] : 0`, the per-element LayerNorm gamma / beta) and waits
// at each join, and the LayerNorm statistics loops wait for each chunk in turn (rocprofv3: 8.7 us with the LayerNorm prologue, 5.3 without).
// Here: loads go to clamped / substitute addresses unconditionally and the VALUE is selected; the x rows are staged in LDS once per
// work-group (LayerNorm / activation applied there by one wave per row, not re-done by every wave); the first batch of weight fragments, the
// bias and the residual are requested at kernel entry, ahead of the staging.
//
// linear_rows_ksplit_kernel: the K chunks of one 16-channel output group are dealt to the FOUR waves of a work-group (the M -> C projection
// of the MLP, K = 1024, was eight dependent batches on 16 waves of the whole chip); the four partial accumulators meet in LDS in a fixed order.
// STAGE selects where the x rows come from.  0: global memory.  1 / 2: assembled in LDS from the partial results of the producing launch,
// which takes that producer's merge launch off the token's dependent chain:
//   1  x = merge of the split-KV single-query attention partials (kv_merge_one; out-projection of the decode step);
//   2  x = x1 + b2 + sum_j P[j]  -- the residual stream after the MLP whose down-projection left NJ K-slice partials (mlp_rows_kernel);
//      work-group 0 also stores the assembled rows (the out-projection two launches later reads them as its residual).
// The assembled rows are rounded to T, exactly what the un-fused chain stores and re-reads.  XF: 0 = rows used as they are (STAGE 0: straight
// from global memory, no LDS), 1 = LayerNorm and / or pre-activation applied to the staged rows.
// ---------------------------------------------------------------------------------------------------------------------------------
#define GM_ROWS_KCH 4  // 16-byte vectors per lane and row in the staging pass: cin <= 64 * VECW * GM_ROWS_KCH (2048 bf16 / 1024 fp32)

// rows [rows][cin] -> xs (LDS, as T), one wave per row: optional LayerNorm (two-pass statistics from registers, like the reference's fp32
// computation) and optional pre-activation.  SRC_LDS: the rows already sit in xs (assembled there), otherwise they come from global memory.
template <typename T, bool SRC_LDS>
__device__ __forceinline__ void stage_rows(const T* __restrict__ x, long long x_ld, T* xs, int rows, int cin, const float* __restrict__ ln_g,
                                           const float* __restrict__ ln_b, float ln_eps, int pre_act) {
  constexpr int VECW = ConvTraits<T>::VECW;
  constexpr bool PRECISE = sizeof(T) == 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* gsrc = ln_g ? ln_g : reinterpret_cast<const float*>(x ? (const void*)x : (const void*)xs);  // never dereferenced without ln_g
  const float* bsrc = ln_b ? ln_b : gsrc;
  const float bmul = ln_b ? 1.f : 0.f;
  for (int r = wave; r < rows; r += 4) {
    float v[GM_ROWS_KCH][VECW], g[GM_ROWS_KCH][VECW], bb[GM_ROWS_KCH][VECW];
    bool ok[GM_ROWS_KCH];
#pragma unroll
    for (int k = 0; k < GM_ROWS_KCH; ++k) {
      const int ch = (k * 64 + lane) * VECW;
      ok[k] = ch + VECW <= cin;
      const int c = ok[k] ? ch : 0;
      const uint4 raw = SRC_LDS ? *reinterpret_cast<const uint4*>(xs + (long long)r * cin + c) : *reinterpret_cast<const uint4*>(x + (long long)r * x_ld + c);
      Vec16<T>::unpack(raw, v[k]);
      if (ln_g) {  // (uniform; the loads inside are unconditional per lane)
#pragma unroll
        for (int i = 0; i < VECW; i += 4) {
          const float4 tg = *reinterpret_cast<const float4*>(gsrc + c + i), tb = *reinterpret_cast<const float4*>(bsrc + c + i);
          g[k][i] = tg.x; g[k][i + 1] = tg.y; g[k][i + 2] = tg.z; g[k][i + 3] = tg.w;
          bb[k][i] = tb.x; bb[k][i + 1] = tb.y; bb[k][i + 2] = tb.z; bb[k][i + 3] = tb.w;
        }
      }
    }
    if (ln_g) {
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < GM_ROWS_KCH; ++k)
#pragma unroll
        for (int i = 0; i < VECW; ++i) sum += ok[k] ? v[k][i] : 0.f;
      const float mean = wave_sum(sum) / (float)cin;
      float sq = 0.f;
#pragma unroll
      for (int k = 0; k < GM_ROWS_KCH; ++k)
#pragma unroll
        for (int i = 0; i < VECW; ++i) sq += ok[k] ? (v[k][i] - mean) * (v[k][i] - mean) : 0.f;
      const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)cin + ln_eps);
#pragma unroll
      for (int k = 0; k < GM_ROWS_KCH; ++k)
#pragma unroll
        for (int i = 0; i < VECW; ++i) v[k][i] = (v[k][i] - mean) * rstd * g[k][i] + bb[k][i] * bmul;
    }
#pragma unroll
    for (int k = 0; k < GM_ROWS_KCH; ++k) {
      if (pre_act) conv_act_vec(v[k], pre_act, PRECISE);
      if (ok[k]) *reinterpret_cast<uint4*>(xs + (long long)r * cin + (k * 64 + lane) * VECW) = Vec16<T>::pack(v[k]);
    }
  }
}

template <typename T, int STAGE, int XF>
__global__ __launch_bounds__(256) void linear_rows_ksplit_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ w,
                                                                const float* __restrict__ bias, const T* __restrict__ res, long long res_ld,
                                                                T* __restrict__ y, long long y_ld, int rows, int cin, int cout, int pre_act,
                                                                int post_act, LinearRowsExtra ex) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW;
  constexpr bool STAGED = STAGE != 0 || XF != 0;
  __shared__ float part[3][64][4];
  extern __shared__ __attribute__((aligned(16))) char staged_raw[];
  T* xs = reinterpret_cast<T*>(staged_raw);  // STAGED: [rows][cin]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int cout_pad = (cout + 15) & ~15;
  const int co0 = blockIdx.x * 16;
  const int row = l15;  // one row block (host: rows <= 16)
  const bool row_ok = row < rows;
  const int nchunks = (cin + BK - 1) / BK;
  const T* wrow = w + ((long long)(co0 + l15)) * BK + q * VECW;
  constexpr int U = 4;
  uint4 wf[U], xf[U];
  // ---- requested at entry: this wave's first batch of weight fragments (chunks wave, wave + 4, ...), bias and residual of its outputs ----------
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int cc = wave + 4 * u;
    wf[u] = *reinterpret_cast<const uint4*>(wrow + (long long)(cc < nchunks ? cc : nchunks - 1) * cout_pad * BK);
  }
  float bia[4], rsd[4];
  {
    const float* bsrc = bias ? bias : reinterpret_cast<const float*>(w);
    const T* rsrc = res ? res + (long long)(row_ok ? row : 0) * res_ld : w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = co0 + 4 * q + i;
      bia[i] = bsrc[bias ? (co < cout ? co : cout - 1) : 0];
      rsd[i] = ElemIO<T>::ld(rsrc + (res ? (co < cout ? co : cout - 1) : 0));
    }
  }
  // this lane's 16-byte vector of chunk c (zero beyond the row / the last channel)
  auto xvec = [&](int c) __attribute__((always_inline)) -> uint4 {
    const bool ok = row_ok & (c * BK + q * VECW + VECW <= cin);
    const uint4 v = STAGED ? *reinterpret_cast<const uint4*>(xs + (ok ? (long long)row * cin + c * BK + q * VECW : 0))
                           : *reinterpret_cast<const uint4*>(ok ? x + (long long)row * x_ld + q * VECW + c * BK : x);
    return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
  };
  if (!STAGED) {
#pragma unroll
    for (int u = 0; u < U; ++u) xf[u] = xvec(wave + 4 * u < nchunks ? wave + 4 * u : nchunks - 1);
  }
  // ---- the x rows into LDS ---------------------------------------------------------------------------------------------------------------
  if (STAGE == 1) {
    const int H = cin / ex.kv_dh;
    for (int idx = threadIdx.x; idx < rows * cin; idx += 256) {
      const int r = idx / cin, ch = idx - r * cin;
      ElemIO<T>::st(xs + idx, kv_merge_one(ex.kv_ws, rows * H, ex.kv_dh, r * H + ch / ex.kv_dh, ch % ex.kv_dh));
    }
  } else if (STAGE == 2) {
    const float* b2 = ex.mlp_b2 ? ex.mlp_b2 : ex.mlp_p;
    const float b2mul = ex.mlp_b2 ? 1.f : 0.f;
    for (int idx = threadIdx.x; idx < rows * cin; idx += 256) {
      const int ch = idx % cin;
      constexpr int PB = 8;  // partials in flight per batch
      float v = ElemIO<T>::ld(reinterpret_cast<const T*>(ex.mlp_x1) + idx) + b2[ex.mlp_b2 ? ch : 0] * b2mul;
      const float* pp = ex.mlp_p + idx;
      const long long pstride = (long long)rows * cin;
      for (int j0 = 0; j0 < ex.mlp_nj; j0 += PB) {
        float t[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) t[j] = pp[(j0 + j < ex.mlp_nj ? j0 + j : j0) * pstride];
#pragma unroll
        for (int j = 0; j < PB; ++j) v += j0 + j < ex.mlp_nj ? t[j] : 0.f;  // slice order
      }
      ElemIO<T>::st(xs + idx, v);
      if (blockIdx.x == 0 && ex.mlp_x0) reinterpret_cast<T*>(ex.mlp_x0)[idx] = xs[idx];
    }
  }
  if (STAGE != 0 && XF != 0) __syncthreads();
  if (XF != 0) {
    if (STAGE == 0) stage_rows<T, false>(x, x_ld, xs, rows, cin, ex.ln_g, ex.ln_b, ex.ln_eps, pre_act);
    else stage_rows<T, true>(nullptr, 0, xs, rows, cin, ex.ln_g, ex.ln_b, ex.ln_eps, pre_act);
  }
  if (STAGED) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; ++u) xf[u] = xvec(wave + 4 * u < nchunks ? wave + 4 * u : nchunks - 1);
  }
  // ---- GEMM over this wave's chunks ---------------------------------------------------------------------------------------------------------
  f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int c0 = wave; c0 < nchunks; c0 += 4 * U) {
    if (c0 != wave) {  // (the first batch was requested at entry)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = c0 + 4 * u < nchunks ? c0 + 4 * u : nchunks - 1;
        wf[u] = *reinterpret_cast<const uint4*>(wrow + (long long)c * cout_pad * BK);
        xf[u] = xvec(c);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + 4 * u < nchunks) Mma<T>::run(wf[u], xf[u], acc);
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) part[wave - 1][lane][i] = acc[i];
  }
  __syncthreads();
  if (wave > 0 || !row_ok) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = ((acc[i] + part[0][lane][i]) + part[1][lane][i]) + part[2][lane][i];  // fixed order: waves 0, 1, 2, 3
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int co = co0 + 4 * q + i;
    if (co < cout) {
      float v = acc[i] + (bias ? bia[i] : 0.f);
      v = conv_post_act(v, post_act);
      if (res) v += rsd[i];
      if (ex.split > 0 && co >= ex.split) {
        T* dst = reinterpret_cast<T*>(co < 2 * ex.split ? ex.y1 : ex.y2) + (ex.off_dev ? (long long)(*ex.off_dev) * ex.off_mul : 0);
        ElemIO<T>::st(dst + (long long)row * ex.y12_ld + (co - (co < 2 * ex.split ? ex.split : 2 * ex.split)), v);
      } else {
        ElemIO<T>::st(y + (long long)row * y_ld + co, v);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The MLP of a decode step in ONE launch (round 3): LayerNorm -> up-projection [C -> M] -> GELU -> down-projection [M -> C].  Work-group j
// owns the hidden slice [64 j, 64 j + 64): the LayerNorm'ed rows are staged in LDS once (stage_rows), its four waves each compute 16 hidden
// channels over all of K = C, the activated slice goes to LDS as T, and the work-group multiplies it with ITS 64-row K-slice of the
// down-projection: a [rows][C] fp32 partial P[j] -- no bias, no residual.  The M / 64 partials are summed (slice order) with the residual row
// and the bias by the consumer's prologue (linear_rows_ksplit_kernel STAGE 2).  Both projections' weight fragments are requested at kernel
// entry (C <= 256 bf16: all of them), so the launch has one exposed round trip.  One launch instead of two on the token's dependent chain,
// and the M -> C product runs on M / 64 work-groups.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mlp_rows_kernel(const T* __restrict__ x, const float* __restrict__ ln_g, const float* __restrict__ ln_b,
                                                      float ln_eps, const T* __restrict__ w1, const float* __restrict__ b1,
                                                      const T* __restrict__ w2, float* __restrict__ P, int rows, int C, int M, int act) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW;
  constexpr int HC = 64 / BK;      // K chunks of the down-projection per hidden slice
  constexpr int GMAX = 8;          // output groups of the down-projection per wave held in registers: C <= 4 * 16 * GMAX = 512
  constexpr int U = 8;             // up-projection chunks in flight
  __shared__ __attribute__((aligned(16))) T hs[16][64 + VECW];  // activated hidden slice, [row][hidden]; + VECW: rows on different banks
  extern __shared__ __attribute__((aligned(16))) char staged_raw[];
  T* xs = reinterpret_cast<T*>(staged_raw);  // [rows][C] LayerNorm'ed rows
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, q = lane >> 4;
  const int j = blockIdx.x;
  const int row = l15;
  const bool row_ok = row < rows;
  const int nchunks = (C + BK - 1) / BK;
  const int cpad = (C + 15) & ~15, mpad = (M + 15) & ~15;
  const int ngroups = cpad / 16;
  const int hc0 = j * 64 + wave * 16;  // this wave's hidden channels
  const T* w1row = w1 + ((long long)(hc0 + l15)) * BK + q * VECW;
  // ---- requested at entry: the up-projection's first U chunks, the bias of this lane's hidden channels, the down-projection fragments of this
  //      wave's output groups (wave, wave + 4, ...) for the slice's HC chunks -------------------------------------------------------------------
  uint4 wf[U];
#pragma unroll
  for (int u = 0; u < U; ++u) wf[u] = *reinterpret_cast<const uint4*>(w1row + (long long)(u < nchunks ? u : nchunks - 1) * mpad * BK);
  float b1v[4];
  {
    const float* bsrc = b1 ? b1 : reinterpret_cast<const float*>(w1);
#pragma unroll
    for (int i = 0; i < 4; ++i) b1v[i] = bsrc[b1 ? hc0 + 4 * q + i : 0];
  }
  uint4 w2f[GMAX][HC];
#pragma unroll
  for (int g = 0; g < GMAX; ++g) {
    const int grp = wave + 4 * g < ngroups ? wave + 4 * g : ngroups - 1;
#pragma unroll
    for (int c = 0; c < HC; ++c) w2f[g][c] = *reinterpret_cast<const uint4*>(w2 + ((long long)(j * HC + c) * cpad + grp * 16 + l15) * BK + q * VECW);
  }
  // ---- LayerNorm'ed rows into LDS ------------------------------------------------------------------------------------------------------------
  stage_rows<T, false>(x, C, xs, rows, C, ln_g, ln_b, ln_eps, 0);
  __syncthreads();
  auto xvec = [&](int c) __attribute__((always_inline)) -> uint4 {
    const bool ok = row_ok & (c * BK + q * VECW + VECW <= C);
    const uint4 v = *reinterpret_cast<const uint4*>(xs + (ok ? (long long)row * C + c * BK + q * VECW : 0));
    return make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u);
  };
  // ---- phase 1: up-projection of hidden channels 64 j + 16 wave .. + 16, GELU ---------------------------------------------------------------
  f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < nchunks; c0 += U) {
    if (c0 != 0) {
#pragma unroll
      for (int u = 0; u < U; ++u) wf[u] = *reinterpret_cast<const uint4*>(w1row + (long long)(c0 + u < nchunks ? c0 + u : nchunks - 1) * mpad * BK);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (c0 + u < nchunks) Mma<T>::run(wf[u], xvec(c0 + u), acc);
  }
  // D layout: column = row l15, rows = hidden channels hc0 + 4 q + i  ->  hs[row][16 wave + 4 q + i] (rows beyond `rows` hold zeros)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = acc[i] + (b1 ? b1v[i] : 0.f);
    v = conv_post_act(v, act);
    ElemIO<T>::st(&hs[l15][wave * 16 + 4 * q + i], row_ok ? v : 0.f);
  }
  __syncthreads();
  // ---- phase 2: P[j][row][co] = sum over the slice's 64 hidden channels -------------------------------------------------------------------
  uint4 hf[HC];
#pragma unroll
  for (int c = 0; c < HC; ++c) hf[c] = *reinterpret_cast<const uint4*>(&hs[l15][c * BK + q * VECW]);
  float* Pj = P + (long long)j * rows * C;
#pragma unroll
  for (int g = 0; g < GMAX; ++g) {
    const int grp = wave + 4 * g;
    if (grp < ngroups) {
      f32x4_t a2 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < HC; ++c) Mma<T>::run(w2f[g][c], hf[c], a2);
      if (row_ok) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int co = grp * 16 + 4 * q + i;
          if (co < C) Pj[(long long)row * C + co] = a2[i];
        }
      }
    }
  }
}

// one row block and a long K: the K chunks of an output group are dealt to the four waves of a work-group
static bool linear_rows_takes_ksplit(int rows, int cin, int dtype) {
  static const bool ksplit = !(getenv("GM_LINEAR_KSPLIT") && getenv("GM_LINEAR_KSPLIT")[0] == '0');  // bench switch (tools/diag_c5.py)
  const int bk = dtype == GM_F32 ? 16 : 32, vecw = dtype == GM_F32 ? 4 : 8;
  // (its staging pass holds GM_ROWS_KCH vectors per lane and row, and the staged rows live in <= 48 KiB of LDS)
  return ksplit && (cin + bk - 1) / bk >= 8 && rows <= 16 && cin <= 64 * vecw * GM_ROWS_KCH && (long long)rows * cin * (dtype == GM_F32 ? 4 : 2) <= 48 * 1024;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Host side.  A call is (GmRowsDesc, GmRowsFused or null): gm_rows_gemm_check holds every requirement once, gm_rows_gemm_route_of the one
// decision between the three kernels (gm_rows_gemm_route exports it), rows_extra the one place LinearRowsExtra is filled.
// ---------------------------------------------------------------------------------------------------------------------------------
static int gm_rows_gemm_check(const GmRowsDesc* dp, const GmRowsFused* f) {
  GM_REQUIRE(dp, "null descriptor");
  const GmRowsDesc& d = *dp;
  GM_REQUIRE((d.pre_scale == nullptr) == (d.pre_shift == nullptr), "scale and shift come together");
  GM_REQUIRE(!d.pre_scale || (d.rows_per_sample > 0 && d.ss_ld % 4 == 0 && gm_aligned16(d.pre_scale) && gm_aligned16(d.pre_shift)),
             "the affine tables are 16-byte aligned fp32 rows");
  if (d.gn) {
    const GmGnTables& t = *d.gn;
    GM_REQUIRE(!d.pre_scale, "the GroupNorm comes as statistic tables or as (scale, shift) tables, not both");
    GM_REQUIRE(t.stats[0] && t.groups > 0 && d.cin % t.groups == 0 && d.cin <= GM_GN_TABLE_MAX_CHANNELS, "GroupNorm tables: whole groups, at most 384 channels");
    const int gn_C[2] = {t.C[0], t.stats[1] ? t.C[1] : 0};  // (C[1] is not read without a second source)
    GM_REQUIRE(gm_gn_stats_form_ok(t.stats, t.S, gn_C, d.cin), "short, 16-byte aligned statistic tables covering the input channels");
    GM_REQUIRE(d.n_samples > 0 && d.rows_per_sample > 0 && d.rows_per_sample % 64 == 0 && d.rows == d.n_samples * d.rows_per_sample, "whole 64-row groups per sample");
  }
  if (d.vt) {
    GM_REQUIRE(d.dtype == GM_BF16 && d.rows_per_sample > 0 && d.rows_per_sample % 64 == 0 && d.rows % d.rows_per_sample == 0,
               "the V^T image needs bf16 and whole 64-key blocks per sample");
    GM_REQUIRE(d.vt_dh > 0 && d.vt_c0 >= 0 && d.vt_c0 < d.cout && (d.cout - d.vt_c0) % d.vt_dh == 0, "the V columns are whole heads");
    GM_REQUIRE(!d.res && d.post_act == 0, "the V^T image: no residual, no output activation");
  }
  GM_REQUIRE((d.x || (f && (f->kv_ws || f->mlp_p))) && d.w && d.y, "null pointer");
  GM_REQUIRE(d.rows >= 0 && d.cin > 0 && d.cout > 0, "bad geometry");
  if (d.rows == 0) return 0;  // nothing is launched
  const int vecw = d.dtype == GM_F32 ? 4 : 8;
  GM_REQUIRE(d.cin % vecw == 0 && d.x_ld % vecw == 0 && gm_aligned16(d.x), "x rows must be 16-byte vectors");
  if (f) {
    GM_REQUIRE(!f->mlp_p || (f->mlp_x1 && f->mlp_nj > 0), "null pointer");
    GM_REQUIRE(!f->kv_ws || (f->kv_ns == GM_DECODE_KV_SPLITS && f->kv_dh > 0 && d.cin % f->kv_dh == 0),
               "the partial-merging prologues live in the K-split kernel: GM_DECODE_KV_SPLITS key ranges of whole heads");
    GM_REQUIRE(f->split == 0 || (f->y1 && f->y2 && d.cout == 3 * f->split), "split output needs two extra destinations and cout = 3 * split");
  }
  if (d.dtype != GM_F32 && d.dtype != GM_BF16) GM_FAIL(-2, "unsupported dtype");
  return 0;
}

// GM_ROWS_ROUTE_* for a call, or a negative error
static int gm_rows_gemm_route_of(const GmRowsDesc* dp, const GmRowsFused* f) {
  if (const int rc = gm_rows_gemm_check(dp, f)) return rc;
  const GmRowsDesc& d = *dp;
  const bool partials = f && (f->kv_ws || f->mlp_p);
  const bool extras = partials || (f && (f->ln_g || f->split != 0 || f->off_dev));
  const int bk = d.dtype == GM_F32 ? 16 : 32, cout_pad = (d.cout + 15) & ~15;
  int route = GM_ROWS_ROUTE_ROWS;
  if (linear_rows_takes_ksplit(d.rows, d.cin, d.dtype) && !d.pre_scale) route = GM_ROWS_ROUTE_KSPLIT;
  else if ((d.gn || (gm_token_gemm_wide_rows > 0 && d.rows >= gm_token_gemm_wide_rows)) && d.cin % bk == 0 && cout_pad >= 32 && !extras) route = GM_ROWS_ROUTE_WIDE;
  GM_REQUIRE(!partials || route == GM_ROWS_ROUTE_KSPLIT, "the partial-merging prologues live in the K-split kernel");
  GM_REQUIRE(!d.gn || route == GM_ROWS_ROUTE_WIDE,
             "the statistics form of the token GEMM's GroupNorm needs the wide kernel's geometry (cin a multiple of the MFMA K step, cout >= 32)");
  return route;
}
extern "C" int gm_rows_gemm_route(const GmRowsDesc* d) { return gm_rows_gemm_route_of(d, nullptr); }

static LinearRowsExtra rows_extra(const GmRowsDesc& d, const GmRowsFused* f) {
  LinearRowsExtra ex = {};
  ex.pre_scale = d.pre_scale; ex.pre_shift = d.pre_shift; ex.ss_ld = d.ss_ld; ex.rows_per_sample = d.rows_per_sample;
  ex.vt = d.vt; ex.vt_c0 = d.vt_c0; ex.vt_dh = d.vt_dh;
  if (d.gn) {
    const GmGnTables& t = *d.gn;
    ex.gn_stats[0] = t.stats[0]; ex.gn_stats[1] = t.stats[1]; ex.gn_S[0] = t.S[0]; ex.gn_S[1] = t.stats[1] ? t.S[1] : 0;
    ex.gn_C[0] = t.C[0]; ex.gn_C[1] = t.stats[1] ? t.C[1] : 0;
    ex.gn_gamma = t.gamma; ex.gn_beta = t.beta; ex.gn_eps = t.eps; ex.gn_groups = t.groups; ex.gn_N = d.n_samples;
  }
  if (f) {
    ex.ln_g = f->ln_g; ex.ln_b = f->ln_b; ex.ln_eps = f->ln_eps;
    ex.y1 = f->y1; ex.y2 = f->y2; ex.y12_ld = f->y12_ld; ex.split = f->split;
    ex.off_dev = f->off_dev; ex.off_mul = f->off_mul;
    ex.kv_ws = f->kv_ws; ex.kv_dh = f->kv_dh;
    ex.mlp_p = f->mlp_p; ex.mlp_nj = f->mlp_nj; ex.mlp_x1 = f->mlp_x1; ex.mlp_b2 = f->mlp_b2; ex.mlp_x0 = f->mlp_x0;
  }
  return ex;
}

extern "C" int gm_rows_gemm_fused(const GmRowsDesc* dp, const GmRowsFused* f, void* stream) {
  const int route = gm_rows_gemm_route_of(dp, f);
  if (route < 0) return route;
  const GmRowsDesc& d = *dp;
  if (d.rows == 0) return 0;
  const LinearRowsExtra ex = rows_extra(d, f);
  hipStream_t st = (hipStream_t)stream;
  const int cout_pad = (d.cout + 15) & ~15;
  const bool f32 = d.dtype == GM_F32;
#define GM_ROWS_ARGS(T) (const T*)d.x, d.x_ld, (const T*)d.w, d.bias, (const T*)d.res, d.res_ld, (T*)d.y, d.y_ld, d.rows, d.cin, d.cout, d.pre_act, d.post_act, ex
  if (route == GM_ROWS_ROUTE_KSPLIT) {
    dim3 gk(cout_pad / 16, 1);
    const int stage = ex.kv_ws ? 1 : ex.mlp_p ? 2 : 0;
    const int xf = (ex.ln_g || d.pre_act) ? 1 : 0;
    const size_t smem = (stage || xf) ? (size_t)d.rows * d.cin * (f32 ? 4 : 2) : 0;  // the staged rows
#define GM_KSPLIT_LAUNCH(T, STAGE, XF) linear_rows_ksplit_kernel<T, STAGE, XF><<<gk, 256, smem, st>>>(GM_ROWS_ARGS(T))
#define GM_KSPLIT_DISPATCH(T)                                                         \
  do {                                                                                \
    if (stage == 0) { if (xf) GM_KSPLIT_LAUNCH(T, 0, 1); else GM_KSPLIT_LAUNCH(T, 0, 0); } \
    else if (stage == 1) { if (xf) GM_KSPLIT_LAUNCH(T, 1, 1); else GM_KSPLIT_LAUNCH(T, 1, 0); } \
    else { if (xf) GM_KSPLIT_LAUNCH(T, 2, 1); else GM_KSPLIT_LAUNCH(T, 2, 0); }       \
  } while (0)
    if (f32) GM_KSPLIT_DISPATCH(float);
    else GM_KSPLIT_DISPATCH(bf16_raw);
#undef GM_KSPLIT_DISPATCH
#undef GM_KSPLIT_LAUNCH
  } else if (route == GM_ROWS_ROUTE_WIDE) {
    const int nb = gm_token_gemm_wide_nb ? gm_token_gemm_wide_nb : (d.rows >= 8192 ? 4 : 2);
    dim3 gw((cout_pad + 16 * nb - 1) / (16 * nb), (d.rows + 63) / 64);
    const size_t gsm = d.gn ? (size_t)d.cin * (2 * 4 + 16) : 0;
#define GM_WIDE_LAUNCH(T, NBV)                                                                    \
  do {                                                                                            \
    if (d.gn) token_gemm_wide_kernel<T, NBV, true><<<gw, 256, gsm, st>>>(GM_ROWS_ARGS(T));        \
    else token_gemm_wide_kernel<T, NBV, false><<<gw, 256, 0, st>>>(GM_ROWS_ARGS(T));              \
  } while (0)
    if (f32) { if (nb == 2) GM_WIDE_LAUNCH(float, 2); else if (nb == 3) GM_WIDE_LAUNCH(float, 3); else GM_WIDE_LAUNCH(float, 4); }
    else { if (nb == 2) GM_WIDE_LAUNCH(bf16_raw, 2); else if (nb == 3) GM_WIDE_LAUNCH(bf16_raw, 3); else GM_WIDE_LAUNCH(bf16_raw, 4); }
#undef GM_WIDE_LAUNCH
  } else {
    dim3 grid((cout_pad / 16 + 3) / 4, (d.rows + 15) / 16);
    if (f32) linear_rows_kernel<float><<<grid, 256, 0, st>>>(GM_ROWS_ARGS(float));
    else linear_rows_kernel<bf16_raw><<<grid, 256, 0, st>>>(GM_ROWS_ARGS(bf16_raw));
  }
#undef GM_ROWS_ARGS
  GM_LAUNCH_CHECK();
}
extern "C" int gm_rows_gemm(const GmRowsDesc* d, void* stream) { return gm_rows_gemm_fused(d, nullptr, stream); }

// The decode step's MLP as one launch leaving K-slice partials, and the consumer form of the small-row GEMM that sums them (see mlp_rows_kernel).
// gm_mlp_rows_fusable: 1 when both kernels take this geometry.  P holds (M / 64) * rows * C floats.
extern "C" int gm_mlp_rows_fusable(int rows, int C, int M, int dtype) {
  static const bool on = !(getenv("GM_DECODE_MLP_FUSE") && getenv("GM_DECODE_MLP_FUSE")[0] == '0');  // bench switch (tools/diag_c5.py)
  const int vecw = dtype == GM_F32 ? 4 : 8;
  return on && (dtype == GM_F32 || dtype == GM_BF16) && rows >= 1 && rows <= 16 && C % vecw == 0 && C <= 512 && M % 64 == 0 &&
         linear_rows_takes_ksplit(rows, C, dtype);
}
extern "C" int gm_mlp_rows(const void* x, const float* ln_g, const float* ln_b, float ln_eps, const void* w1, const float* b1, const void* w2,
                           float* P, int rows, int C, int M, int act, int dtype, void* stream) {
  GM_REQUIRE(x && w1 && w2 && P && ln_g, "null pointer");
  GM_REQUIRE(gm_mlp_rows_fusable(rows, C, M, dtype), "geometry outside the fused MLP kernel");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == GM_F32)
    mlp_rows_kernel<float><<<M / 64, 256, (size_t)rows * C * 4, st>>>((const float*)x, ln_g, ln_b, ln_eps, (const float*)w1, b1, (const float*)w2, P, rows, C, M, act);
  else
    mlp_rows_kernel<bf16_raw><<<M / 64, 256, (size_t)rows * C * 2, st>>>((const bf16_raw*)x, ln_g, ln_b, ln_eps, (const bf16_raw*)w1, b1, (const bf16_raw*)w2, P, rows, C, M, act);
  GM_LAUNCH_CHECK();
}
extern "C" int gm_linear_rows_takes_ksplit(int rows, int cin, int dtype) { return linear_rows_takes_ksplit(rows, cin, dtype) ? 1 : 0; }
