// Kernels of the SPADE VAE-GAN generator (reference: generative/networks/nets/spade_network.py; Park et al. 2019).
//
// gm_spade_block_apply -- the decoder's one memory-bound pass per SPADE norm.  A SPADEResNetBlock normalises the SAME x twice (norm_0 for the
//   main branch, norm_s for the learned shortcut) and, from the second block on, x is the nearest 2x up-sampling of the previous block's
//   output.  Replicating every voxel 2^d times changes neither the per-channel mean nor the biased variance, so the instance-norm (scale,
//   shift) of up(x) are those of x: this kernel reads x on its own (half-resolution) grid, applies them, and writes one or two modulated
//   outputs on the full-resolution grid.  up(x) is never materialised and no statistics pass runs over it.
// gm_leaky_relu -- LeakyReLU with a runtime slope (the reference's blocks use 0.2), forward and backward, over a dense tensor.
// gm_kld -- the VAE's KL term and its gradients: one work-group, fp64, fixed summation order.
//
// All three are HBM-bound element-wise passes: 16 bytes per lane where C, the pitches and the base addresses allow it, a scalar path for
// everything else (C == 1 is a real case: the last block of every SPADENet), grid capped at 2048 blocks with a grid-stride loop.
#include "gm_common.h"

#define GM_SB_ACT_NONE 0
#define GM_SB_ACT_SILU 1
#define GM_SB_ACT_LEAKY 3  // (2 is ReLU in the shared activation table: LeakyReLU with slope 0)

template <typename T> __device__ __forceinline__ float sb_act(float v, int act, float slope) {
  if (act == GM_SB_ACT_SILU) return sizeof(T) == 4 ? gm_silu_precise(v) : gm_silu(v);
  if (act == GM_SB_ACT_LEAKY) return v > 0.f ? v : v * slope;
  return v;
}

// grid (blocks, N); one lane per (output voxel, channel vector) of its sample, indexed in 32 bits (the host checks V * C / VEC < 2^32).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void spade_block_apply_kernel(const T* __restrict__ x, long long x_ld, const float* __restrict__ scale,
                                                               const float* __restrict__ shift, long long ss_ld, const T* __restrict__ g0,
                                                               const T* __restrict__ b0, long long gb0_ld, T* __restrict__ y0, long long y0_ld,
                                                               const T* __restrict__ g1, const T* __restrict__ b1, long long gb1_ld,
                                                               T* __restrict__ y1, long long y1_ld, unsigned Ho, unsigned Wo, unsigned Hs, unsigned Ws,
                                                               long long Vs, long long Vo, unsigned CV, unsigned items, int up, int act0, float slope) {
  const long long n = blockIdx.y;
  const float* sc = scale + n * ss_ld;
  const float* sh = shift + n * ss_ld;
  const unsigned step = gridDim.x * 256u;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < items; i += step) {
    const unsigned v = i / CV;
    const unsigned c = (i - v * CV) * VEC;
    unsigned sv = v;
    if (up) {  // output voxel (d, h, w) reads the source voxel (d >> 1, h >> 1, w >> 1); a 2-D grid has one depth slice on both sides
      const unsigned q = v / Wo, w = v - q * Wo;
      const unsigned d = q / Ho, h = q - d * Ho;
      sv = ((d >> 1) * Hs + (h >> 1)) * Ws + (w >> 1);
    }
    const long long orow = n * Vo + v;
    float t[VEC], o[VEC];
    VecIO<T, VEC>::ld(x + (n * Vs + sv) * x_ld + c, t);
#pragma unroll
    for (int k = 0; k < VEC; ++k) t[k] = t[k] * sc[c + k] + sh[c + k];
    if (g0) {
      float gv[VEC], bv[VEC];
      VecIO<T, VEC>::ld(g0 + orow * gb0_ld + c, gv);
      VecIO<T, VEC>::ld(b0 + orow * gb0_ld + c, bv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = t[k] * gv[k] + bv[k];
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = t[k];
    }
    if (act0 != GM_SB_ACT_NONE) {  // (tested once per vector, as in gm_spade_apply)
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = sb_act<T>(o[k], act0, slope);
    }
    VecIO<T, VEC>::st(y0 + orow * y0_ld + c, o);
    if (g1) {
      float gv[VEC], bv[VEC];
      VecIO<T, VEC>::ld(g1 + orow * gb1_ld + c, gv);
      VecIO<T, VEC>::ld(b1 + orow * gb1_ld + c, bv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = t[k] * gv[k] + bv[k];
      VecIO<T, VEC>::st(y1 + orow * y1_ld + c, o);
    }
  }
}

// x: [N][Ds*Hs*Ws] rows of x_ld elements; every map / output: [N][Do*Ho*Wo] rows of its own pitch.  up == 0: the two grids are equal.
// up == 1: Ho == 2 Hs, Wo == 2 Ws and Do == 2 Ds, or Do == Ds == 1 for a 2-D grid.  g0 == NULL: y0 = act0(norm(x)).  g1 != NULL adds y1.
extern "C" int gm_spade_block_apply(const void* x, long long x_ld, const float* scale, const float* shift, long long ss_ld, const void* g0,
                                    const void* b0, long long gb0_ld, void* y0, long long y0_ld, const void* g1, const void* b1,
                                    long long gb1_ld, void* y1, long long y1_ld, int N, int Ds, int Hs, int Ws, int Do, int Ho, int Wo, int C,
                                    int up, int act0, float slope, int dtype, void* stream) {
  GM_REQUIRE(x && scale && shift && y0, "null pointer");
  GM_REQUIRE((g0 == nullptr) == (b0 == nullptr) && (g1 == nullptr) == (b1 == nullptr), "a map set is a (gamma, beta) pair");
  GM_REQUIRE(g1 == nullptr || y1 != nullptr, "the second map set needs its output");
  GM_REQUIRE(act0 == GM_SB_ACT_NONE || act0 == GM_SB_ACT_SILU || act0 == GM_SB_ACT_LEAKY, "activation: none, silu or leakyrelu");
  GM_REQUIRE(N >= 0 && Ds >= 0 && Hs >= 0 && Ws >= 0 && Do >= 0 && Ho >= 0 && Wo >= 0 && C >= 0, "negative extent");
  if (up) GM_REQUIRE(Ho == 2 * Hs && Wo == 2 * Ws && (Do == 2 * Ds || (Do == 1 && Ds == 1)), "up: the output grid is twice the source grid");
  else GM_REQUIRE(Do == Ds && Ho == Hs && Wo == Ws, "the output grid equals the source grid");
  GM_REQUIRE(x_ld >= C && ss_ld >= C && y0_ld >= C && (!g0 || gb0_ld >= C) && (!g1 || (gb1_ld >= C && y1_ld >= C)), "pitch below C");
  const long long Vs = (long long)Ds * Hs * Ws, Vo = (long long)Do * Ho * Wo;
  if ((long long)N * Vo * C == 0) return 0;
  GM_REQUIRE(N <= 65535, "batch above 65535");
  const int vec = dtype == GM_F32 ? 4 : 8;
  const bool vec_ok = (C % vec == 0) && (x_ld % vec == 0) && (y0_ld % vec == 0) && gm_aligned16(x) && gm_aligned16(y0) &&
                      (!g0 || ((gb0_ld % vec == 0) && gm_aligned16(g0) && gm_aligned16(b0))) &&
                      (!g1 || ((gb1_ld % vec == 0) && (y1_ld % vec == 0) && gm_aligned16(g1) && gm_aligned16(b1) && gm_aligned16(y1)));
  const long long CV = vec_ok ? C / vec : C, items = Vo * CV;
  GM_REQUIRE(items < (1ll << 32), "one sample holds 2^32 or more work items");
  long long grid = (items + 255) / 256;  // memory-bound: about 8 blocks per CU, the rest by grid stride
  const long long cap = (2048 + N - 1) / N;
  if (grid > cap) grid = cap;
  hipStream_t st = (hipStream_t)stream;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        spade_block_apply_kernel<T, decltype(tv)::vec><<<dim3((unsigned)grid, (unsigned)N), 256, 0, st>>>(
            (const T*)x, x_ld, scale, shift, ss_ld, (const T*)g0, (const T*)b0, gb0_ld, (T*)y0, y0_ld, (const T*)g1, (const T*)b1, gb1_ld, (T*)y1, y1_ld,
            (unsigned)Ho, (unsigned)Wo, (unsigned)Hs, (unsigned)Ws, Vs, Vo, (unsigned)CV, (unsigned)items, up, act0, slope);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

// gy == NULL: out = x > 0 ? x : slope * x.  Otherwise out = gy * (x > 0 ? 1 : slope), x being the pre-activation.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void leaky_relu_kernel(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ out, float slope,
                                                        long long items) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
    float v[VEC], o[VEC];
    VecIO<T, VEC>::ld(x + i * VEC, v);
    if (gy) {
      float g[VEC];
      VecIO<T, VEC>::ld(gy + i * VEC, g);
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = v[k] > 0.f ? g[k] : g[k] * slope;
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = v[k] > 0.f ? v[k] : v[k] * slope;
    }
    VecIO<T, VEC>::st(out + i * VEC, o);
  }
}

extern "C" int gm_leaky_relu(const void* x, const void* gy, void* out, float slope, long long total, int dtype, void* stream) {
  GM_REQUIRE(x && out, "null pointer");
  GM_REQUIRE(total >= 0, "negative size");
  if (total == 0) return 0;
  const int vec = dtype == GM_F32 ? 4 : 8;
  const bool vec_ok = (total % vec == 0) && gm_aligned16(x) && gm_aligned16(out) && (!gy || gm_aligned16(gy));
  const long long items = vec_ok ? total / vec : total;
  long long grid = (items + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipStream_t st = (hipStream_t)stream;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        leaky_relu_kernel<T, decltype(tv)::vec><<<(unsigned)grid, 256, 0, st>>>((const T*)x, (const T*)gy, (T*)out, slope, items);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

// KLD = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) (reference: spade_network.py KLDLoss).  One work-group: lane t adds elements t, t + 256, ...
// in fp64, the 256 partials are folded by a fixed LDS tree -> the value is bitwise repeatable.  dmu / dlogvar (optional, both or neither):
// up * mu and up * -0.5 * (1 - exp(logvar)), `up` the upstream gradient read from device memory (NULL: 1).
template <typename T>
__global__ __launch_bounds__(256) void kld_kernel(const T* __restrict__ mu, const T* __restrict__ logvar, long long total, float* __restrict__ out,
                                                 const float* __restrict__ upstream, T* __restrict__ dmu, T* __restrict__ dlogvar) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  const double up = upstream ? (double)*upstream : 1.0;
  double acc = 0.0;
  for (long long i = t; i < total; i += 256) {
    const double m = (double)ElemIO<T>::ld(mu + i), lv = (double)ElemIO<T>::ld(logvar + i);
    const double e = exp(lv);
    acc += 1.0 + lv - m * m - e;
    if (dmu) {
      ElemIO<T>::st(dmu + i, (float)(up * m));
      ElemIO<T>::st(dlogvar + i, (float)(up * -0.5 * (1.0 - e)));
    }
  }
  part[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0 && out) *out = (float)(-0.5 * part[0]);
}

extern "C" int gm_kld(const void* mu, const void* logvar, long long total, float* out, const float* upstream, void* dmu, void* dlogvar, int dtype,
                      void* stream) {
  GM_REQUIRE(mu && logvar, "null pointer");
  GM_REQUIRE(total >= 0, "negative size");
  GM_REQUIRE((dmu == nullptr) == (dlogvar == nullptr), "the two gradients are written together");
  GM_REQUIRE(out || dmu, "nothing to write");
  hipStream_t st = (hipStream_t)stream;
  if (!gm_dispatch_dtype(dtype, [&](auto tv) {
        using T = typename decltype(tv)::type;
        kld_kernel<T><<<1, 256, 0, st>>>((const T*)mu, (const T*)logvar, total, out, upstream, (T*)dmu, (T*)dlogvar);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}
