// The single-query attention of an autoregressive decode step: softmax(scale q K^T) V for ONE query per (batch, head) over a KV cache
// (reference: blocks/selfattention.py:117-147 evaluated for the last position only).
//   attn_decode_kernel           one work-group per (batch, head): keys spread over the 256 threads, scores through LDS, the PV sum parallel over
//                                (channel, key slice); behind gm_attention_forward for Lq = 1, and with the key count read on the device
//   attn_decode_split_kernel     long windows: the keys cut into GM_DECODE_KV_SPLITS ranges, one work-group each (attn_range_body), partials to a workspace
//   attn_decode_combine_kernel   ... merged in range order (kv_merge_one; the out-projection's prologue in rows_gemm.hip can merge them instead)
//   qkv_attn_rows_kernel         LayerNorm + q | k | v projection + one key range in ONE launch, with its select / plan / launch functions
//   cross_attn_rows_kernel       cross attention: LayerNorm + one head's q projection + all keys of the projected context in ONE launch, likewise
#include <cstdlib>
#include "conv_common.h"
#include "decode_common.h"

// ---------------------------------------------------------------------------------------------------------------------------------
// one query per (batch, head)
// ---------------------------------------------------------------------------------------------------------------------------------
#define DEC_MAX_KEYS 15360  // scores live in LDS (fp32): 60 KiB + query + scratch stay under the default 64 KiB dynamic limit

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_kernel(GmAttnDesc p, const int* __restrict__ lk_dev) {
  const int lds_keys = p.Lk;       // the launch sized the score buffer for this many keys
  if (lk_dev) p.Lk = *lk_dev + 1;  // decode-graph replay: keys 0 .. position (LDS was sized for the descriptor's Lk = the cache length)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = reinterpret_cast<float*>(smem);            // [Lk] scores, then probabilities
  float* qs = sc + ((((lk_dev ? lds_keys : p.Lk) > 2048 ? (lk_dev ? lds_keys : p.Lk) : 2048) + 3) & ~3);  // [dh] query (fp32); the score region doubles as the [KL][dh] partial table
  float* red = qs + p.dh;                                 // [256] reduction scratch / [slices][dh] partial outputs
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
  const int dh = p.dh;
  const T* Q = reinterpret_cast<const T*>(p.q) + (long long)b * p.q_ld + h * dh;  // Lq == 1
  const T* K = reinterpret_cast<const T*>(p.k) + (long long)b * (p.k_bs ? p.k_bs : (long long)p.Lk * p.k_ld) + h * dh;
  const T* V = reinterpret_cast<const T*>(p.v) + (long long)b * (p.v_bs ? p.v_bs : (long long)p.Lk * p.v_ld) + h * dh;
  for (int c = tid; c < dh; c += 256) qs[c] = ElemIO<T>::ld(Q + c) * p.scale;
  __syncthreads();
  // ---- scores: thread <-> key -------------------------------------------------------------------------------------------------
  float mx = -INFINITY;
  constexpr int VECW = 16 / (int)sizeof(T);
  const bool kvec = (dh % VECW == 0) && (p.k_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0);
  for (int j = tid; j < p.Lk; j += 256) {
    const T* kr = K + (long long)j * p.k_ld;
    float s = 0.f;
    if (kvec) {
      for (int c = 0; c < dh; c += VECW) {
        float kv[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(kr + c), kv);
#pragma unroll
        for (int i = 0; i < VECW; ++i) s += qs[c + i] * kv[i];
      }
    } else {
      for (int c = 0; c < dh; ++c) s += qs[c] * ElemIO<T>::ld(kr + c);
    }
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < p.Lk; j += 256) {
    const float e = expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  const float inv = 1.0f / (red[0] + red[1] + red[2] + red[3]);
  __syncthreads();
  // ---- output: thread <-> (key lane, 16-byte channel vector): KL keys per iteration, 4 iterations of independent loads in flight
  //      (one 2-byte load per thread per key, accumulated serially, cost ~1 us of latency per key: 125 us per call at 3500 keys) -----
  const bool vvec = (dh % VECW == 0) && (p.v_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(V) & 15) == 0);
  float o[VECW];
#pragma unroll
  for (int i = 0; i < VECW; ++i) o[i] = 0.f;
  const int nv = vvec ? dh / VECW : dh;             // channel vectors (or single channels) per key
  const int KL = 256 / nv > 0 ? 256 / nv : 1;       // key lanes
  const int cv = tid % nv, kl = tid / nv;
  if (kl < KL) {
    if (vvec) {
      int j = kl;
      for (; j + 3 * KL < p.Lk; j += 4 * KL) {
        uint4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const uint4*>(V + (long long)(j + u * KL) * p.v_ld + cv * VECW);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float vv[VECW];
          Vec16<T>::unpack(r[u], vv);
          const float pj = sc[j + u * KL];
#pragma unroll
          for (int i = 0; i < VECW; ++i) o[i] += pj * vv[i];
        }
      }
      for (; j < p.Lk; j += KL) {
        float vv[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(V + (long long)j * p.v_ld + cv * VECW), vv);
        const float pj = sc[j];
#pragma unroll
        for (int i = 0; i < VECW; ++i) o[i] += pj * vv[i];
      }
    } else {
      for (int j = kl; j < p.Lk; j += KL) o[0] += sc[j] * ElemIO<T>::ld(V + (long long)j * p.v_ld + cv);
    }
  }
  __syncthreads();  // everyone is done reading the probabilities: the score buffer becomes the [KL][dh] partial-sum table
  const int per = vvec ? VECW : 1;
  if (kl < KL)
    for (int i = 0; i < per; ++i) sc[kl * dh + cv * per + i] = o[i];
  __syncthreads();
  if (tid < dh) {
    float tot = 0.f;
    for (int s2 = 0; s2 < KL; ++s2) tot += sc[s2 * dh + tid];
    float out = tot * inv;
    if (p.res) out += ElemIO<T>::ld(reinterpret_cast<const T*>(p.res) + (long long)b * p.res_ld + h * dh + tid);
    ElemIO<T>::st(reinterpret_cast<T*>(p.o) + (long long)b * p.o_ld + h * dh + tid, out);
  }
}

// returns 1 if launched, 0 if the geometry is not a single-query decode this kernel covers.  lk_dev != null: attend keys
// 0 .. *lk_dev (read on the device at run time); d.Lk is then the upper bound the LDS buffer is sized for.
extern "C" int gm_attention_decode_dev(const GmAttnDesc* dp, const int* lk_dev, void* stream) {
  const GmAttnDesc& d = *dp;
  if (d.Lq != 1 || d.Lk > DEC_MAX_KEYS || d.dh > 256 || d.Lk < 1) return 0;
  if (d.dtype != GM_F32 && d.dtype != GM_BF16) return 0;
  hipStream_t st = (hipStream_t)stream;
  const size_t smem = (size_t)((((d.Lk > 2048 ? d.Lk : 2048) + 3) & ~3) + d.dh + 256) * sizeof(float);
  if (d.dtype == GM_F32) attn_decode_kernel<float><<<d.B * d.H, 256, smem, st>>>(d, lk_dev);
  else attn_decode_kernel<bf16_raw><<<d.B * d.H, 256, smem, st>>>(d, lk_dev);
  return 1;
}

extern "C" int gm_attention_decode_try(const GmAttnDesc* dp, void* stream) { return gm_attention_decode_dev(dp, nullptr, stream); }

// ---------------------------------------------------------------------------------------------------------------------------------
// Split-KV form of the single-query attention (round 3).  `attn_decode_kernel` gives one (batch, head) to ONE work-group: at 4096 cached
// keys each thread walks 16 keys one dependent L2 round trip after the other and then 16 value rows -- 20-25 us per layer on 8 of the
// chip's 256 CUs.  Here the keys of a (batch, head) are cut into NS contiguous ranges (a multiple of 64 keys each, so a range is one key
// per thread at NS = 16 and 4096 keys); work-group (bh, s) writes its range's (running max m, sum l of exp(score - m), un-normalised
// output sum_j exp(score_j - m) v_j) to the workspace and the consumer -- `attn_decode_combine_kernel`, or the out-projection GEMM's
// prologue (`kv_merge_one`, decode_common.h) -- merges the NS partials in range order:
//     M = max_s m_s,   out = (sum_s e^{m_s - M} o_s) / (sum_s e^{m_s - M} l_s)   (+ residual).
// The partition depends on the key count only (host value, or `*lk_dev + 1` under graph replay), every sum has a fixed order: the eager
// and the replayed step give identical bits.  Workspace: B * H * NS * (dh + 2) floats.
// ---------------------------------------------------------------------------------------------------------------------------------
// One key range of the single-query attention: scores over keys K[0 .. n), softmax state, un-normalised output -> the range's partial
// (shared by attn_decode_split_kernel and the fused q|k|v + attention kernel below).  qs: the scaled query in LDS (published by the caller);
// sc: LDS scores / probabilities, later the [KL][dh] partial table; red: 4 floats.  K, V point at the range's first key.
template <typename T>
__device__ __forceinline__ void attn_range_body(const T* __restrict__ K, long long k_ld, const T* __restrict__ V, long long v_ld, int n, int dh,
                                                const float* qs, float* sc, float* red, float* wsp, float* wm, float* wl, int tid) {
  struct { long long k_ld, v_ld; } p = {k_ld, v_ld};
  float mx = -INFINITY;
  constexpr int VECW = 16 / (int)sizeof(T);
  const bool kvec = (dh % VECW == 0) && (p.k_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(K) & 15) == 0);
  for (int j = tid; j < n; j += 256) {
    const T* kr = K + (long long)j * p.k_ld;
    float s = 0.f;
    if (kvec) {
      for (int c = 0; c < dh; c += VECW) {
        float kv[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(kr + c), kv);
#pragma unroll
        for (int i = 0; i < VECW; ++i) s += qs[c + i] * kv[i];
      }
    } else {
      for (int c = 0; c < dh; ++c) s += qs[c] * ElemIO<T>::ld(kr + c);
    }
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float sum = 0.f;
  for (int j = tid; j < n; j += 256) {
    const float e = expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  const float tot_l = ((red[0] + red[1]) + red[2]) + red[3];
  const bool vvec = (dh % VECW == 0) && (p.v_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(V) & 15) == 0);
  float o[VECW];
#pragma unroll
  for (int i = 0; i < VECW; ++i) o[i] = 0.f;
  const int nv = vvec ? dh / VECW : dh;
  const int KL = 256 / nv > 0 ? 256 / nv : 1;
  const int cv = tid % nv, kl = tid / nv;
  if (kl < KL) {
    if (vvec) {
      int j = kl;
      for (; j + 3 * KL < n; j += 4 * KL) {
        uint4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = *reinterpret_cast<const uint4*>(V + (long long)(j + u * KL) * p.v_ld + cv * VECW);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float vv[VECW];
          Vec16<T>::unpack(r[u], vv);
          const float pj = sc[j + u * KL];
#pragma unroll
          for (int i = 0; i < VECW; ++i) o[i] += pj * vv[i];
        }
      }
      for (; j < n; j += KL) {
        float vv[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(V + (long long)j * p.v_ld + cv * VECW), vv);
        const float pj = sc[j];
#pragma unroll
        for (int i = 0; i < VECW; ++i) o[i] += pj * vv[i];
      }
    } else {
      for (int j = kl; j < n; j += KL) o[0] += sc[j] * ElemIO<T>::ld(V + (long long)j * p.v_ld + cv);
    }
  }
  __syncthreads();
  const int per = vvec ? VECW : 1;
  if (kl < KL)
    for (int i = 0; i < per; ++i) sc[kl * dh + cv * per + i] = o[i];
  __syncthreads();
  if (tid < dh) {
    float tot = 0.f;
    for (int s2 = 0; s2 < KL; ++s2) tot += sc[s2 * dh + tid];
    wsp[tid] = tot;
  }
  if (tid == 0) { *wm = mx; *wl = tot_l; }
}

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_split_kernel(GmAttnDesc p, const int* __restrict__ lk_dev, float* __restrict__ ws, int NS,
                                                               int sc_elems, int chunk, int cap) {
  if (!p.k_bs) p.k_bs = (long long)cap * p.k_ld;  // dense caches: `cap` rows per batch entry
  if (!p.v_bs) p.v_bs = (long long)cap * p.v_ld;
  if (lk_dev) p.Lk = *lk_dev + 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sc = reinterpret_cast<float*>(smem);  // [chunk] scores, then probabilities; later the [KL][dh] partial table
  float* qs = sc + sc_elems;                   // [dh]
  float* red = qs + p.dh;                      // [4]
  const int tid = threadIdx.x;
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, sp = blockIdx.y;
  const int dh = p.dh;
  const int k0 = sp * chunk, k1 = min(p.Lk, k0 + chunk);
  const long long BH = (long long)gridDim.x;
  float* wsp = ws + ((long long)bh * NS + sp) * dh;              // o[BH][NS][dh]
  float* wm = ws + BH * NS * dh + (long long)bh * NS + sp;       // m[BH][NS]
  float* wl = wm + BH * NS;                                      // l[BH][NS]
  if (k0 >= p.Lk) {  // an empty range: weight zero in the merge
    if (tid < dh) wsp[tid] = 0.f;
    if (tid == 0) { *wm = -INFINITY; *wl = 0.f; }
    return;
  }
  const int n = k1 - k0;
  const T* Q = reinterpret_cast<const T*>(p.q) + (long long)b * p.q_ld + h * dh;
  const T* K = reinterpret_cast<const T*>(p.k) + (long long)b * (p.k_bs ? p.k_bs : (long long)p.Lk * p.k_ld) + h * dh + (long long)k0 * p.k_ld;
  const T* V = reinterpret_cast<const T*>(p.v) + (long long)b * (p.v_bs ? p.v_bs : (long long)p.Lk * p.v_ld) + h * dh + (long long)k0 * p.v_ld;
  for (int c = tid; c < dh; c += 256) qs[c] = ElemIO<T>::ld(Q + c) * p.scale;
  __syncthreads();
  attn_range_body<T>(K, p.k_ld, V, p.v_ld, n, dh, qs, sc, red, wsp, wm, wl, tid);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// LayerNorm + q | k | v projection + one key range of the single-query attention in ONE launch (round 3): work-group (b * H + h, range) assembles
// the residual-stream row of sample b (plain, or x1 + b2 + sum_j P[j] behind a fused MLP -- work-group (h = 0, range 0) also stores it for the
// out-projection's residual), normalises it, and multiplies it with head h's 3 * dh rows of the stacked projection: the K chunks are dealt to the
// four waves, the partial sums meet in LDS in wave order.  q stays in LDS (scaled, rounded through T like the stored q of the two-launch form);
// the work-group whose range holds the position stores the new k / v rows into the caches and -- after a fence and a barrier -- reads them back
// with the rest of its range; the others never touch that row.  Every work-group recomputes q (3 * dh x C MACs: nothing) and requests ALL its
// weight fragments at entry; what the fusion buys is one ~4.5 us launch per block of the token's dependent chain.
// NG = 3 * dh / 16 output groups, UM = K chunks per wave (host: C % BK == 0, ceil(C / BK / 4) <= UM).
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int NG, int UM>
__global__ __launch_bounds__(256) void qkv_attn_rows_kernel(QkvAttnArgs a) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW, NS = GM_DECODE_KV_SPLITS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int C = a.C, dh = a.dh;
  float* sc = reinterpret_cast<float*>(smem);      // [sc_elems]
  float* qs = sc + a.sc_elems;                     // [dh]
  float* red = qs + dh;                            // [8]
  float* xrow = red + 8;                           // [C] the assembled row (values already rounded through T)
  float* part = xrow + C;                          // [4][3 dh]
  T* xn = reinterpret_cast<T*>(part + 4 * 3 * dh); // [C] LayerNorm'ed row (16-byte aligned: every count above is a multiple of 4 floats)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H, sp = blockIdx.y;
  const int nchunks = C / BK, cout_pad = (3 * C + 15) & ~15;
  constexpr int GPH = NG / 3;  // output groups per head part (dh / 16)
  // ---- requested at entry: the position, every weight fragment of this wave, this thread's bias -------------------------------------------
  const int pos = a.pos_dev ? *a.pos_dev : a.pos;
  const T* W = reinterpret_cast<const T*>(a.w);
  uint4 wfr[NG][UM];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int co = (g / GPH) * C + h * dh + (g % GPH) * 16 + l15;
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const int c = wave + 4 * u < nchunks ? wave + 4 * u : nchunks - 1;
      wfr[g][u] = *reinterpret_cast<const uint4*>(W + ((long long)c * cout_pad + co) * BK + q4 * VECW);
    }
  }
  const int tt = tid < 3 * dh ? tid : 0;
  const float bval = (a.bias ? a.bias : reinterpret_cast<const float*>(a.w))[a.bias ? (tt / dh) * C + h * dh + tt % dh : 0];
  const int Lk = pos + 1;
  const int k0 = sp * a.chunk, k1 = min(Lk, k0 + a.chunk);
  const long long BH = (long long)gridDim.x;
  float* wsp = a.ws + ((long long)bh * NS + sp) * dh;
  float* wm = a.ws + BH * NS * dh + (long long)bh * NS + sp;
  float* wl = wm + BH * NS;
  if (k0 >= Lk) {  // an empty range (never range 0, never the position's range): weight zero in the merge
    if (tid < dh) wsp[tid] = 0.f;
    if (tid == 0) { *wm = -INFINITY; *wl = 0.f; }
    return;
  }
  const bool owner = pos >= k0 && pos < k0 + a.chunk;
  // ---- the residual-stream row of sample b ------------------------------------------------------------------------------------------------
  for (int idx = tid; idx < C; idx += 256) {
    float v;
    if (a.mlp_p) {
      const float* b2 = a.mlp_b2 ? a.mlp_b2 : a.mlp_p;
      v = ElemIO<T>::ld(reinterpret_cast<const T*>(a.mlp_x1) + (long long)b * C + idx) + b2[a.mlp_b2 ? idx : 0] * (a.mlp_b2 ? 1.f : 0.f);
      const float* pp = a.mlp_p + (long long)b * C + idx;
      const long long pstride = (long long)a.B * C;
      constexpr int PB = 8;
      for (int j0 = 0; j0 < a.mlp_nj; j0 += PB) {
        float t[PB];
#pragma unroll
        for (int j = 0; j < PB; ++j) t[j] = pp[(j0 + j < a.mlp_nj ? j0 + j : j0) * pstride];
#pragma unroll
        for (int j = 0; j < PB; ++j) v += j0 + j < a.mlp_nj ? t[j] : 0.f;  // slice order
      }
    } else {
      v = ElemIO<T>::ld(reinterpret_cast<const T*>(a.x0) + (long long)b * C + idx);
    }
    T r;
    ElemIO<T>::st(&r, v);
    xrow[idx] = ElemIO<T>::ld(&r);
    if (a.mlp_p && a.x0_out && h == 0 && sp == 0) reinterpret_cast<T*>(a.x0_out)[(long long)b * C + idx] = r;
  }
  __syncthreads();
  // ---- LayerNorm (two-pass statistics, like the reference's fp32 computation) -------------------------------------------------------------
  float part_s = 0.f;
  for (int idx = tid; idx < C; idx += 256) part_s += xrow[idx];
  part_s = wave_sum(part_s);
  if (lane == 0) red[wave] = part_s;
  __syncthreads();
  const float mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)C;
  float part_q = 0.f;
  for (int idx = tid; idx < C; idx += 256) part_q += (xrow[idx] - mean) * (xrow[idx] - mean);
  part_q = wave_sum(part_q);
  if (lane == 0) red[4 + wave] = part_q;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((((red[4] + red[5]) + red[6]) + red[7]) / (float)C + a.ln_eps);
  for (int idx = tid; idx < C; idx += 256)
    ElemIO<T>::st(xn + idx, (xrow[idx] - mean) * rstd * a.ln_g[idx] + (a.ln_b ? a.ln_b[idx] : 0.f));
  __syncthreads();
  // ---- q | k | v of head h: this wave's K chunks, then the four waves' partial sums in wave order ---------------------------------------------
  f32x4_t acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) acc[g] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < UM; ++u) {
    const int c = wave + 4 * u;
    if (c < nchunks) {  // (wave-uniform)
      const uint4 xv = *reinterpret_cast<const uint4*>(xn + c * BK + q4 * VECW);
      const uint4 xf = make_uint4(l15 == 0 ? xv.x : 0u, l15 == 0 ? xv.y : 0u, l15 == 0 ? xv.z : 0u, l15 == 0 ? xv.w : 0u);  // MFMA column 0 = the row
#pragma unroll
      for (int g = 0; g < NG; ++g) Mma<T>::run(wfr[g][u], xf, acc[g]);
    }
  }
  if (l15 == 0) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[wave * 3 * dh + g * 16 + 4 * q4 + i] = acc[g][i];
  }
  __syncthreads();
  if (tid < 3 * dh) {
    const float val = (((part[tid] + part[3 * dh + tid]) + part[6 * dh + tid]) + part[9 * dh + tid]) + (a.bias ? bval : 0.f);
    T r;
    ElemIO<T>::st(&r, val);
    const int which = tid / dh, c = tid - which * dh;
    if (which == 0) {
      qs[c] = ElemIO<T>::ld(&r) * a.scale;
    } else if (owner) {
      T* dst = reinterpret_cast<T*>(which == 1 ? a.kcache : a.vcache) + ((long long)b * a.cap + pos) * C + h * dh + c;
      *dst = r;
    }
  }
  if (owner) __threadfence();  // the new rows are in L2 before any wave of this work-group reads its range
  __syncthreads();
  const T* K = reinterpret_cast<const T*>(a.kcache) + ((long long)b * a.cap + k0) * C + h * dh;
  const T* V = reinterpret_cast<const T*>(a.vcache) + ((long long)b * a.cap + k0) * C + h * dh;
  attn_range_body<T>(K, C, V, C, k1 - k0, dh, qs, sc, red, wsp, wm, wl, tid);
}

// Which instantiation takes this geometry: 1 and (*ng, *um) = its template arguments (and the launch geometry in *chunk, *sc_elems, *smem when
// given), 0 = none.  The one decision both the launch below and the decode step's plan (decode_step.hip) consult.
static int qkv_attn_rows_select(const QkvAttnArgs& a, int dtype, int* ng_out, int* um_out, int* chunk_out, int* sc_out, size_t* smem_out) {
  static const bool on = !(getenv("GM_DECODE_QKV_FUSE") && getenv("GM_DECODE_QKV_FUSE")[0] == '0');  // bench switch (tools/diag_c5.py)
  if (!on || (dtype != GM_F32 && dtype != GM_BF16)) return 0;
  const int bk = dtype == GM_F32 ? 16 : 32, vecw = dtype == GM_F32 ? 4 : 8;
  if (!a.ln_g || !a.w || !a.kcache || !a.vcache || !a.ws || (!a.x0 && !a.mlp_p)) return 0;
  if (a.dh % 16 || a.C % bk || a.C != a.H * a.dh || a.C % vecw) return 0;
  const int ng = 3 * a.dh / 16, nchunks = a.C / bk, um = (nchunks + 3) / 4;
  const int chunk = ((a.cap + GM_DECODE_KV_SPLITS - 1) / GM_DECODE_KV_SPLITS + 63) & ~63;
  const int sc_elems = chunk > 256 * vecw ? chunk : 256 * vecw;
  if (sc_elems > 32768 || (long long)a.B * a.H > 65535) return 0;
  const size_t smem = (size_t)(sc_elems + a.dh + 8 + a.C + 12 * a.dh) * sizeof(float) + (size_t)a.C * (dtype == GM_F32 ? 4 : 2);
  if (smem > 160 * 1024) return 0;
  int sel_ng = 0, sel_um = 0;  // (the same table for both dtypes; first match wins)
  if (ng == 6 && um <= 2) { sel_ng = 6; sel_um = 2; }
  else if (ng == 6 && um <= 4) { sel_ng = 6; sel_um = 4; }
  else if (ng == 12 && um <= 2) { sel_ng = 12; sel_um = 2; }
  else return 0;
  if (ng_out) *ng_out = sel_ng;
  if (um_out) *um_out = sel_um;
  if (chunk_out) *chunk_out = chunk;
  if (sc_out) *sc_out = sc_elems;
  if (smem_out) *smem_out = smem;
  return 1;
}
// the non-launching query beside gm_qkv_attn_rows: 1 and the instantiation (NG, UM) that would take `ap`, or 0
extern "C" int gm_qkv_attn_rows_plan(const QkvAttnArgs* ap, int dtype, int* ng, int* um) {
  return qkv_attn_rows_select(*ap, dtype, ng, um, nullptr, nullptr, nullptr);
}

// 1 = launched, 0 = not this kernel's case (the caller issues the LayerNorm + q|k|v GEMM and gm_attention_decode_split), < 0 = error.
extern "C" int gm_qkv_attn_rows(const QkvAttnArgs* ap, int dtype, void* stream) {
  const QkvAttnArgs& a = *ap;
  int ng = 0, um = 0, chunk = 0, sc_elems = 0;
  size_t smem = 0;
  if (!qkv_attn_rows_select(a, dtype, &ng, &um, &chunk, &sc_elems, &smem)) return 0;
  QkvAttnArgs k = a;
  k.chunk = chunk; k.sc_elems = sc_elems;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(a.B * a.H, GM_DECODE_KV_SPLITS);
#define GM_QKV_LAUNCH(T, NG, UM)                                                                                          \
  do {                                                                                                                    \
    static bool attr = false;                                                                                             \
    if (!attr) {                                                                                                          \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(qkv_attn_rows_kernel<T, NG, UM>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      attr = true;                                                                                                        \
    }                                                                                                                     \
    qkv_attn_rows_kernel<T, NG, UM><<<grid, 256, smem, st>>>(k);                                                           \
    return hipGetLastError() == hipSuccess ? 1 : -1;                                                                      \
  } while (0)
  if (dtype == GM_BF16) {
    if (ng == 6 && um == 2) GM_QKV_LAUNCH(bf16_raw, 6, 2);
    if (ng == 6 && um == 4) GM_QKV_LAUNCH(bf16_raw, 6, 4);
    if (ng == 12 && um == 2) GM_QKV_LAUNCH(bf16_raw, 12, 2);
  } else {
    if (ng == 6 && um == 2) GM_QKV_LAUNCH(float, 6, 2);
    if (ng == 6 && um == 4) GM_QKV_LAUNCH(float, 6, 4);
    if (ng == 12 && um == 2) GM_QKV_LAUNCH(float, 12, 2);
  }
#undef GM_QKV_LAUNCH
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Cross attention of the decode step: LayerNorm2 + head h's q projection + the 1 x Lc attention over the projected context in ONE launch, built like
// qkv_attn_rows_kernel above: work-group b * H + h normalises the residual-stream row of sample b, multiplies it with head h's dh rows of to_q (K chunks
// dealt to the four waves, every weight fragment requested at entry, the partial sums met in LDS in wave order), keeps q in LDS (scaled, rounded through T
// like the stored q of the composed form) and runs attn_range_body over ALL Lc keys of ck / cv (read only).  The context is short (tens of keys: one
// range) and does not grow, so there is no key split and no merge: the work-group normalises its own output and stores it for the out-projection GEMM.
// NG = dh / 16 output groups, UM = K chunks per wave (host: C % BK == 0, ceil(C / BK / 4) <= UM).  Fixed summation order, no atomics.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int NG, int UM>
__global__ __launch_bounds__(256) void cross_attn_rows_kernel(CrossAttnArgs a) {
  constexpr int BK = ConvTraits<T>::BK, VECW = ConvTraits<T>::VECW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int C = a.C, dh = a.dh;
  float* sc = reinterpret_cast<float*>(smem);    // [sc_elems] scores, then probabilities; later the [KL][dh] partial table
  float* qs = sc + a.sc_elems;                   // [dh]
  float* red = qs + dh;                          // [8]
  float* outp = red + 8;                         // [dh] un-normalised output
  float* ml = outp + dh;                         // [4] softmax maximum, denominator
  float* xrow = ml + 4;                          // [C]
  float* part = xrow + C;                        // [4][dh]
  T* xn = reinterpret_cast<T*>(part + 4 * dh);   // [C] LayerNorm'ed row (16-byte aligned: every count above is a multiple of 4 floats)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, q4 = lane >> 4;
  const int bh = blockIdx.x, b = bh / a.H, h = bh % a.H;
  const int nchunks = C / BK, cout_pad = (C + 15) & ~15;
  // ---- requested at entry: every weight fragment of this wave, this thread's bias ------------------------------------------------------------
  const T* W = reinterpret_cast<const T*>(a.w);
  uint4 wfr[NG][UM];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int co = h * dh + g * 16 + l15;
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const int c = wave + 4 * u < nchunks ? wave + 4 * u : nchunks - 1;
      wfr[g][u] = *reinterpret_cast<const uint4*>(W + ((long long)c * cout_pad + co) * BK + q4 * VECW);
    }
  }
  const int tt = tid < dh ? tid : 0;
  const float bval = (a.bias ? a.bias : reinterpret_cast<const float*>(a.w))[a.bias ? h * dh + tt : 0];
  // ---- the residual-stream row of sample b, LayerNorm (two-pass statistics, like the reference's fp32 computation) -----------------------------
  for (int idx = tid; idx < C; idx += 256) xrow[idx] = ElemIO<T>::ld(reinterpret_cast<const T*>(a.x) + (long long)b * C + idx);
  __syncthreads();
  float part_s = 0.f;
  for (int idx = tid; idx < C; idx += 256) part_s += xrow[idx];
  part_s = wave_sum(part_s);
  if (lane == 0) red[wave] = part_s;
  __syncthreads();
  const float mean = (((red[0] + red[1]) + red[2]) + red[3]) / (float)C;
  float part_q = 0.f;
  for (int idx = tid; idx < C; idx += 256) part_q += (xrow[idx] - mean) * (xrow[idx] - mean);
  part_q = wave_sum(part_q);
  if (lane == 0) red[4 + wave] = part_q;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((((red[4] + red[5]) + red[6]) + red[7]) / (float)C + a.ln_eps);
  for (int idx = tid; idx < C; idx += 256)
    ElemIO<T>::st(xn + idx, (xrow[idx] - mean) * rstd * a.ln_g[idx] + (a.ln_b ? a.ln_b[idx] : 0.f));
  __syncthreads();
  // ---- q of head h: this wave's K chunks, then the four waves' partial sums in wave order --------------------------------------------------------
  f32x4_t acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) acc[g] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < UM; ++u) {
    const int c = wave + 4 * u;
    if (c < nchunks) {  // (wave-uniform)
      const uint4 xv = *reinterpret_cast<const uint4*>(xn + c * BK + q4 * VECW);
      const uint4 xf = make_uint4(l15 == 0 ? xv.x : 0u, l15 == 0 ? xv.y : 0u, l15 == 0 ? xv.z : 0u, l15 == 0 ? xv.w : 0u);  // MFMA column 0 = the row
#pragma unroll
      for (int g = 0; g < NG; ++g) Mma<T>::run(wfr[g][u], xf, acc[g]);
    }
  }
  if (l15 == 0) {
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) part[wave * dh + g * 16 + 4 * q4 + i] = acc[g][i];
  }
  __syncthreads();
  if (tid < dh) {
    const float val = (((part[tid] + part[dh + tid]) + part[2 * dh + tid]) + part[3 * dh + tid]) + (a.bias ? bval : 0.f);
    T r;
    ElemIO<T>::st(&r, val);
    qs[tid] = ElemIO<T>::ld(&r) * a.scale;
  }
  __syncthreads();
  // ---- softmax(q Kc^T) Vc over the Lc context keys of sample b, head h ----------------------------------------------------------------------------
  const T* K = reinterpret_cast<const T*>(a.ck) + (long long)b * a.Lc * C + h * dh;
  const T* V = reinterpret_cast<const T*>(a.cv) + (long long)b * a.Lc * C + h * dh;
  attn_range_body<T>(K, C, V, C, a.Lc, dh, qs, sc, red, outp, ml, ml + 1, tid);
  __syncthreads();
  if (tid < dh) ElemIO<T>::st(reinterpret_cast<T*>(a.o) + (long long)b * C + h * dh + tid, outp[tid] * (1.0f / ml[1]));
}

// Which instantiation takes this geometry: 1 and (*ng, *um) = its template arguments (and *sc_elems, *smem when given), 0 = none.  The one decision
// both the launch below and the decode step's cross route (decode_step.hip: gm_decode_cross_route) consult.
static int cross_attn_rows_select(const CrossAttnArgs& a, int dtype, int* ng_out, int* um_out, int* sc_out, size_t* smem_out) {
  static const bool on = !(getenv("GM_DECODE_CROSS_FUSE") && getenv("GM_DECODE_CROSS_FUSE")[0] == '0');  // bench switch (tools/bench_c5.py)
  if (!on || (dtype != GM_F32 && dtype != GM_BF16)) return 0;
  const int bk = dtype == GM_F32 ? 16 : 32, vecw = dtype == GM_F32 ? 4 : 8;
  if (a.H <= 0 || a.dh <= 0 || a.C != a.H * a.dh || a.C % bk) return 0;
  if (a.dh != 16 && a.dh != 32 && a.dh != 64 && a.dh != 128) return 0;  // NG in {1, 2, 4, 8}
  if (a.Lc < 1 || a.Lc > GM_DECODE_CROSS_MAX_FUSED_CTX || a.B < 1 || (long long)a.B * a.H > 65535) return 0;
  const int ng = a.dh / 16, nchunks = a.C / bk, need = (nchunks + 3) / 4;
  const int um = need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 0;
  if (!um || ng * um > 32) return 0;  // (the weight fragments are 4 registers each)
  const int keys = (a.Lc + 3) & ~3;
  const int sc_elems = keys > 256 * vecw ? keys : 256 * vecw;  // the score buffer doubles as the [KL][dh] partial table
  if (ng_out) *ng_out = ng;
  if (um_out) *um_out = um;
  if (sc_out) *sc_out = sc_elems;
  if (smem_out) *smem_out = (size_t)(sc_elems + a.dh + 8 + a.dh + 4 + a.C + 4 * a.dh) * sizeof(float) + (size_t)a.C * (dtype == GM_F32 ? 4 : 2);
  return 1;
}
extern "C" int gm_cross_attn_rows_plan(const CrossAttnArgs* ap, int dtype, int* ng, int* um) {
  return cross_attn_rows_select(*ap, dtype, ng, um, nullptr, nullptr);
}

extern "C" int gm_cross_attn_rows(const CrossAttnArgs* ap, int dtype, void* stream) {
  const CrossAttnArgs& a = *ap;
  int ng = 0, um = 0, sc_elems = 0;
  size_t smem = 0;
  if (!a.x || !a.ln_g || !a.w || !a.ck || !a.cv || !a.o) return 0;
  if (!cross_attn_rows_select(a, dtype, &ng, &um, &sc_elems, &smem)) return 0;
  CrossAttnArgs k = a;
  k.sc_elems = sc_elems;
  hipStream_t st = (hipStream_t)stream;
#define GM_CROSS_LAUNCH(NG, UM)                                                                          \
  if (ng == NG && um == UM) {                                                                            \
    if (dtype == GM_BF16) cross_attn_rows_kernel<bf16_raw, NG, UM><<<a.B * a.H, 256, smem, st>>>(k);     \
    else cross_attn_rows_kernel<float, NG, UM><<<a.B * a.H, 256, smem, st>>>(k);                         \
    return hipGetLastError() == hipSuccess ? 1 : -1;                                                     \
  }
  GM_CROSS_LAUNCH(1, 2) GM_CROSS_LAUNCH(1, 4) GM_CROSS_LAUNCH(1, 8)
  GM_CROSS_LAUNCH(2, 2) GM_CROSS_LAUNCH(2, 4) GM_CROSS_LAUNCH(2, 8)
  GM_CROSS_LAUNCH(4, 2) GM_CROSS_LAUNCH(4, 4) GM_CROSS_LAUNCH(4, 8)
  GM_CROSS_LAUNCH(8, 2) GM_CROSS_LAUNCH(8, 4)
#undef GM_CROSS_LAUNCH
  return 0;
}


template <typename T>
__global__ __launch_bounds__(64) void attn_decode_combine_kernel(GmAttnDesc p, const float* __restrict__ ws) {
  const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H, dh = p.dh;
  for (int c = threadIdx.x; c < dh; c += 64) {
    float out = kv_merge_one(ws, gridDim.x, dh, bh, c);
    if (p.res) out += ElemIO<T>::ld(reinterpret_cast<const T*>(p.res) + (long long)b * p.res_ld + h * dh + c);
    ElemIO<T>::st(reinterpret_cast<T*>(p.o) + (long long)b * p.o_ld + h * dh + c, out);
  }
}

// 1 = launched, 0 = not this kernel's case.  `ws` holds gm_attention_decode_split_ws_elems(B, H, dh, nsplit) floats.
extern "C" long long gm_attention_decode_split_ws_elems(int B, int H, int dh, int nsplit) { return (long long)B * H * nsplit * (dh + 2); }
// `merge`: 1 = partials + merge; 0 = partials only, for a consumer that merges them itself (GmRowsFused.kv_ws); 2 = the merge launch only.
// `cap` = rows of the K / V caches per batch entry (>= the key count): the key ranges are cut from it, so they are the same for every position.
extern "C" int gm_attention_decode_split(const GmAttnDesc* dp, const int* lk_dev, float* ws, int nsplit, int merge, int cap, void* stream) {
  const GmAttnDesc& d = *dp;
  if (d.Lq != 1 || d.dh > 256 || d.Lk < 1 || cap < d.Lk || nsplit != GM_DECODE_KV_SPLITS || !ws) return 0;  // (the merge code unrolls over the split count)
  if (d.dtype != GM_F32 && d.dtype != GM_BF16) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int vecw = d.dtype == GM_F32 ? 4 : 8;
  const int chunk = ((cap + nsplit - 1) / nsplit + 63) & ~63;
  const int sc_elems = chunk > 256 * vecw ? chunk : 256 * vecw;  // the score buffer doubles as the [KL][dh] partial table
  if (sc_elems > 32768) return 0;
  const size_t smem = (size_t)(sc_elems + d.dh + 4) * sizeof(float);
  // (measured and removed: a variant issuing the key row, the value vectors, the query and the key count before its first wait -- one exposed
  //  round trip instead of four -- ran 6.4 vs 6.5 us: these launches are bound by their ~4.5 us floor and their instruction count, not by loads)
  dim3 grid(d.B * d.H, nsplit);
  if (d.dtype == GM_F32) {
    if (merge != 2) attn_decode_split_kernel<float><<<grid, 256, smem, st>>>(d, lk_dev, ws, nsplit, sc_elems, chunk, cap);
    if (merge) attn_decode_combine_kernel<float><<<d.B * d.H, 64, 0, st>>>(d, ws);
  } else {
    if (merge != 2) attn_decode_split_kernel<bf16_raw><<<grid, 256, smem, st>>>(d, lk_dev, ws, nsplit, sc_elems, chunk, cap);
    if (merge) attn_decode_combine_kernel<bf16_raw><<<d.B * d.H, 64, 0, st>>>(d, ws);
  }
  return 1;
}
