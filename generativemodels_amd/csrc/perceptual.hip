// The three kernels PerceptualLoss (losses/perceptual.py: LPIPS over a frozen AlexNet / VGG16 stack) adds to the convolutions, each with its backward.
// All tensors are dense channels-last arenas; every sum runs in a fixed order and nothing is accumulated with atomics, so a step is bitwise repeatable.
//   gm_maxpool2d / _bwd       MaxPool2d(k, 2), k = 2 or 3, floor mode, no padding.  The backward is a gather over the at most four windows that cover an input
//                             element: each window's arg-max is recomputed from x (first maximum in row-major order, NaN wins: torch's rule), no index tensor.
//   gm_lpips_layer / _bwd     per sample: mean over pixels of sum_c w_c (f_c / (|f| + 1e-10) - g_c / (|g| + 1e-10))^2.  A group of G lanes (a power of two,
//                             G * 16 bytes >= a pixel's channels where that fits a wave) holds one pixel's channels in registers; the channel sums are xor
//                             butterflies inside the group, the pixel sum is fp64 per group, an LDS tree per work-group and a fold launch over the work-groups.
//                             The backward recomputes |f|, |g| (it reads f and g anyway: keeping them would add 16 bytes per pixel, recomputing adds none).
//   gm_slice_gather / _bwd    the chosen slices across one axis of an (N, C, D, H, W) volume, C = 1 or 3, as three-channel images (x - shift) / scale.
#include "gm_common.h"

template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to<bf16_raw>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// ---- max pooling ---------------------------------------------------------------------------------------------------------------------------------------
// the window's maxima (and, ARG, which element holds each: a * k + b) over VEC channels; `base` = the window's first element
template <typename T, int VEC, bool ARG>
__device__ __forceinline__ void pool_window(const T* base, int W, int C, int k, float* m, int* arg) {
  VecIO<T, VEC>::ld(base, m);
#pragma unroll
  for (int e = 0; e < VEC; ++e)
    if (ARG) arg[e] = 0;
  for (int a = 0; a < k; ++a)
    for (int b = (a == 0 ? 1 : 0); b < k; ++b) {
      float v[VEC];
      VecIO<T, VEC>::ld(base + ((long long)a * W + b) * C, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (v[e] > m[e] || v[e] != v[e]) {
          m[e] = v[e];
          if (ARG) arg[e] = a * k + b;
        }
    }
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool2d_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo, int k) {
  const int cv = C / VEC;
  const long long total = (long long)N * Ho * Wo * cv;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int c = (int)(i % cv) * VEC;
    long long p = i / cv;
    const int wo = (int)(p % Wo);
    p /= Wo;
    const int ho = (int)(p % Ho), n = (int)(p / Ho);
    float m[VEC];
    pool_window<T, VEC, false>(x + (((long long)n * H + 2 * ho) * W + 2 * wo) * C + c, W, C, k, m, nullptr);
    VecIO<T, VEC>::st(y + (i / cv) * C + c, m);
  }
}

// dx[n, h, w, c] = the sum of gy over the windows whose arg-max is (h, w), windows in row-major order, rounded to T after every addition (what
// torch's scatter in T does, so that a bf16 result agrees bit for bit)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void maxpool2d_bwd_kernel(const T* __restrict__ x, const T* __restrict__ gy, T* __restrict__ dx, int N, int H, int W, int C,
                                                            int Ho, int Wo, int k) {
  const int cv = C / VEC;
  const long long total = (long long)N * H * W * cv;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int c = (int)(i % cv) * VEC;
    long long p = i / cv;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H), n = (int)(p / H);
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    const int ho0 = h - k + 1 > 0 ? (h - k + 2) / 2 : 0, ho1 = h / 2 < Ho - 1 ? h / 2 : Ho - 1;
    const int wo0 = w - k + 1 > 0 ? (w - k + 2) / 2 : 0, wo1 = w / 2 < Wo - 1 ? w / 2 : Wo - 1;
    for (int ho = ho0; ho <= ho1; ++ho)
      for (int wo = wo0; wo <= wo1; ++wo) {
        float m[VEC], gv[VEC];
        int arg[VEC];
        pool_window<T, VEC, true>(x + (((long long)n * H + 2 * ho) * W + 2 * wo) * C + c, W, C, k, m, arg);
        VecIO<T, VEC>::ld(gy + (((long long)n * Ho + ho) * Wo + wo) * C + c, gv);
        const int mine = (h - 2 * ho) * k + (w - 2 * wo);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (arg[e] == mine) acc[e] = round_to<T>(acc[e] + gv[e]);
      }
    VecIO<T, VEC>::st(dx + (i / cv) * C + c, acc);
  }
}

static int pool_check(const char* fn, int N, int H, int W, int C, int k) {
  if (N < 1 || C < 1 || (k != 2 && k != 3)) { gm_set_error(fn, -1, "max pooling: kernel 2 or 3 at stride 2, N >= 1, C >= 1"); return -1; }
  if (H < k || W < k) { gm_set_error(fn, -1, "max pooling: the image is smaller than the window"); return -1; }
  return 0;
}
static inline unsigned stream_grid(long long total) { const long long b = (total + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > (1 << 20) ? (1 << 20) : b)); }

extern "C" int gm_maxpool2d(const void* x, void* y, int N, int H, int W, int C, int k, int dtype, void* stream) {
  GM_REQUIRE(x && y, "null pointer");
  if (pool_check(__func__, N, H, W, C, k)) return -1;
  const int Ho = (H - k) / 2 + 1, Wo = (W - k) / 2 + 1;
  hipStream_t st = (hipStream_t)stream;
  const bool vec_ok = gm_aligned16(x) && gm_aligned16(y) && C % (dtype == GM_F32 ? 4 : 8) == 0;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        constexpr int VEC = decltype(tv)::vec;
        maxpool2d_kernel<T, VEC><<<stream_grid((long long)N * Ho * Wo * (C / VEC)), 256, 0, st>>>((const T*)x, (T*)y, N, H, W, C, Ho, Wo, k);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_maxpool2d_bwd(const void* x, const void* gy, void* dx, int N, int H, int W, int C, int k, int dtype, void* stream) {
  GM_REQUIRE(x && gy && dx, "null pointer");
  if (pool_check(__func__, N, H, W, C, k)) return -1;
  const int Ho = (H - k) / 2 + 1, Wo = (W - k) / 2 + 1;
  hipStream_t st = (hipStream_t)stream;
  const bool vec_ok = gm_aligned16(x) && gm_aligned16(gy) && gm_aligned16(dx) && C % (dtype == GM_F32 ? 4 : 8) == 0;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        constexpr int VEC = decltype(tv)::vec;
        maxpool2d_bwd_kernel<T, VEC><<<stream_grid((long long)N * H * W * (C / VEC)), 256, 0, st>>>((const T*)x, (const T*)gy, (T*)dx, N, H, W, C, Ho, Wo, k);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

// ---- the LPIPS layer distance --------------------------------------------------------------------------------------------------------------------------
#define LP_EPS 1e-10f
#define LP_MAXV 2  // 16-byte vectors of a pixel per lane: C <= 512 in fp32 is 128 vectors over the 64 lanes of a wave

// lanes per pixel: the power of two that covers the pixel's C / VEC vectors, one wave at the most
static inline int lp_group(int C, int vec) {
  int g = 8;
  while (g < 64 && g < C / vec) g <<= 1;
  return g;
}
static inline bool lp_channels_ok(int C) { return C == 64 || C == 128 || C == 192 || C == 256 || C == 384 || C == 512; }
// work-groups per sample: each walks a contiguous run of pixels, 256 / G of them per pass, about eight passes
static inline int lp_blocks(long long HW, int G) {
  const long long b = (HW + (256 / G) * 8 - 1) / ((256 / G) * 8);
  return (int)(b < 1 ? 1 : (b > 128 ? 128 : b));
}

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // (a + b on both lanes of a pair: every lane of the group ends with the same bits)
  return v;
}

// One pixel's channels of f and g in the group's registers, and what both directions need of them.  Control flow is uniform over the work-group (a lane
// without a vector, or past the last pixel, holds zeros), so every lane takes part in every butterfly.
template <typename T, int VEC> struct LpPixel {
  float f[LP_MAXV][VEC], g[LP_MAXV][VEC];
  float nf, ng;
  __device__ __forceinline__ void load(const T* fp, const T* gp, int gl, int G, int nvec, bool valid) {
    float sf = 0.f, sg = 0.f;
#pragma unroll
    for (int i = 0; i < LP_MAXV; ++i) {
      const int j = gl + G * i;
      if (valid && j < nvec) {
        VecIO<T, VEC>::ld(fp + j * VEC, f[i]);
        VecIO<T, VEC>::ld(gp + j * VEC, g[i]);
      } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) f[i][e] = g[i][e] = 0.f;
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) { sf += f[i][e] * f[i][e]; sg += g[i][e] * g[i][e]; }
    }
    nf = sqrtf(group_sum(sf, G));
    ng = sqrtf(group_sum(sg, G));
  }
};

template <int VEC> __device__ __forceinline__ void lp_load_w(const float* __restrict__ w, int gl, int G, int nvec, float (*wv)[VEC]) {
#pragma unroll
  for (int i = 0; i < LP_MAXV; ++i) {
    const int j = gl + G * i;
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const float4 t = j < nvec ? *reinterpret_cast<const float4*>(w + j * VEC + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
      wv[i][4 * q] = t.x; wv[i][4 * q + 1] = t.y; wv[i][4 * q + 2] = t.z; wv[i][4 * q + 3] = t.w;
    }
  }
}

// partial[n][b] = the sum of the pixel distances of work-group b's run of sample n (fp64)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void lpips_layer_kernel(const T* __restrict__ f, const T* __restrict__ g, const float* __restrict__ w,
                                                          double* __restrict__ partial, long long HW, int C, int G) {
  __shared__ double red[256];
  const int t = threadIdx.x, n = blockIdx.y, nvec = C / VEC, gpb = 256 / G, grp = t / G, gl = t % G;
  const long long chunk = (HW + gridDim.x - 1) / gridDim.x;
  const long long p0 = (long long)blockIdx.x * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;
  float wv[LP_MAXV][VEC];
  lp_load_w<VEC>(w, gl, G, nvec, wv);
  double acc = 0.0;
  for (long long base = p0; base < p1; base += gpb) {
    const long long p = base + grp;
    const bool valid = p < p1;
    const long long off = ((long long)n * HW + (valid ? p : p0)) * C;
    LpPixel<T, VEC> px;
    px.load(f + off, g + off, gl, G, nvec, valid);
    const float af = px.nf + LP_EPS, ag = px.ng + LP_EPS;
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < LP_MAXV; ++i)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float u = px.f[i][e] / af - px.g[i][e] / ag;
        d += wv[i][e] * u * u;
      }
    d = group_sum(d, G);
    if (valid && gl == 0) acc += (double)d;
  }
  red[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  if (t == 0) partial[(long long)n * gridDim.x + blockIdx.x] = red[0];
}

// out[n] = (the partials of sample n, added in work-group order) / HW
__global__ __launch_bounds__(64) void lpips_fold_kernel(const double* __restrict__ partial, float* __restrict__ out, int N, int B, double inv_hw) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= N) return;
  double s = 0.0;
  for (int b = 0; b < B; ++b) s += partial[(long long)n * B + b];
  out[n] = (float)(s * inv_hw);
}

// With u_c = f_c / (|f| + eps) - g_c / (|g| + eps), s_f = sum_c w_c u_c f_c, s_g = sum_c w_c u_c g_c and k = 2 up[n] / HW:
//   df_c = k (w_c u_c / (|f| + eps) - f_c s_f / (|f| (|f| + eps)^2)),   dg_c = k (-w_c u_c / (|g| + eps) + g_c s_g / (|g| (|g| + eps)^2));
// a pixel whose vector is all zero gets the gradient 0 (torch's autograd of the formula gives NaN there: inf * 0 through the square root).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void lpips_layer_bwd_kernel(const T* __restrict__ f, const T* __restrict__ g, const float* __restrict__ w,
                                                              const float* __restrict__ up, T* __restrict__ df, T* __restrict__ dg, long long P, long long HW,
                                                              int C, int G, float two_over_hw) {
  const int t = threadIdx.x, nvec = C / VEC, gpb = 256 / G, grp = t / G, gl = t % G;
  float wv[LP_MAXV][VEC];
  lp_load_w<VEC>(w, gl, G, nvec, wv);
  for (long long base = (long long)blockIdx.x * gpb; base < P; base += (long long)gridDim.x * gpb) {
    const long long p = base + grp;
    const bool valid = p < P;
    const long long off = (valid ? p : 0) * C;
    LpPixel<T, VEC> px;
    px.load(f + off, g + off, gl, G, nvec, valid);
    const float af = px.nf + LP_EPS, ag = px.ng + LP_EPS;
    float u[LP_MAXV][VEC], sf = 0.f, sg = 0.f;
#pragma unroll
    for (int i = 0; i < LP_MAXV; ++i)
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        u[i][e] = wv[i][e] * (px.f[i][e] / af - px.g[i][e] / ag);  // w_c u_c
        sf += u[i][e] * px.f[i][e];
        sg += u[i][e] * px.g[i][e];
      }
    sf = group_sum(sf, G);
    sg = group_sum(sg, G);
    if (!valid) continue;  // (past the butterflies; `valid` is uniform over a group)
    const float kk = up[p / HW] * two_over_hw;
    const float a1 = px.nf > 0.f ? kk / af : 0.f, a2 = px.nf > 0.f ? kk * sf / (px.nf * af * af) : 0.f;
    const float b1 = px.ng > 0.f ? kk / ag : 0.f, b2 = px.ng > 0.f ? kk * sg / (px.ng * ag * ag) : 0.f;
#pragma unroll
    for (int i = 0; i < LP_MAXV; ++i) {
      const int j = gl + G * i;
      if (j >= nvec) continue;
      float o[VEC];
      if (df) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = u[i][e] * a1 - px.f[i][e] * a2;
        VecIO<T, VEC>::st(df + off + j * VEC, o);
      }
      if (dg) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = px.g[i][e] * b2 - u[i][e] * b1;
        VecIO<T, VEC>::st(dg + off + j * VEC, o);
      }
    }
  }
}

static int lp_check(const char* fn, int N, long long HW, int C, int dtype) {
  if (N < 1 || HW < 1 || N > 65535) { gm_set_error(fn, -1, "lpips layer: 1 <= N <= 65535 samples of HW >= 1 pixels"); return -1; }
  if (!lp_channels_ok(C)) { gm_set_error(fn, -1, "lpips layer: C must be 64, 128, 192, 256, 384 or 512 (the taps of the AlexNet and VGG16 stacks)"); return -1; }
  if (dtype != GM_F32 && dtype != GM_BF16) { gm_set_error(fn, -2, "unsupported dtype"); return -2; }
  return 0;
}

extern "C" long long gm_lpips_layer_workspace_bytes(int N, long long HW, int C, int dtype) {
  if (N < 1 || HW < 1 || !lp_channels_ok(C) || (dtype != GM_F32 && dtype != GM_BF16)) return -1;
  return (long long)N * lp_blocks(HW, lp_group(C, dtype == GM_F32 ? 4 : 8)) * (long long)sizeof(double);
}

extern "C" int gm_lpips_layer(const void* f, const void* g, const float* w, float* out, void* workspace, long long workspace_bytes, int N, long long HW, int C,
                              int dtype, void* stream) {
  GM_REQUIRE(f && g && w && out && workspace, "null pointer");
  if (const int rc = lp_check(__func__, N, HW, C, dtype)) return rc;
  GM_REQUIRE(gm_aligned16(f) && gm_aligned16(g) && gm_aligned16(w), "lpips layer: operands must be 16-byte aligned");
  GM_REQUIRE(workspace_bytes >= gm_lpips_layer_workspace_bytes(N, HW, C, dtype), "lpips layer: workspace too small (gm_lpips_layer_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  gm_dispatch_vec(dtype, true, [&](auto tv) {
    using T = typename decltype(tv)::type;
    constexpr int VEC = decltype(tv)::vec;
    const int G = lp_group(C, VEC), B = lp_blocks(HW, G);
    lpips_layer_kernel<T, VEC><<<dim3(B, N), 256, 0, st>>>((const T*)f, (const T*)g, w, (double*)workspace, HW, C, G);
    lpips_fold_kernel<<<gm_cdiv(N, 64), 64, 0, st>>>((const double*)workspace, out, N, B, 1.0 / (double)HW);
  });
  GM_LAUNCH_CHECK();
}

extern "C" int gm_lpips_layer_bwd(const void* f, const void* g, const float* w, const float* up, void* df, void* dg, int N, long long HW, int C, int dtype,
                                  void* stream) {
  GM_REQUIRE(f && g && w && up, "null pointer");
  GM_REQUIRE(df || dg, "nothing to write");
  if (const int rc = lp_check(__func__, N, HW, C, dtype)) return rc;
  GM_REQUIRE(gm_aligned16(f) && gm_aligned16(g) && gm_aligned16(w) && gm_aligned16(df) && gm_aligned16(dg), "lpips layer: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  gm_dispatch_vec(dtype, true, [&](auto tv) {
    using T = typename decltype(tv)::type;
    constexpr int VEC = decltype(tv)::vec;
    const int G = lp_group(C, VEC);
    const long long P = (long long)N * HW, blocks = (P + 256 / G - 1) / (256 / G);
    lpips_layer_bwd_kernel<T, VEC><<<(unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks), 256, 0, st>>>((const T*)f, (const T*)g, w, up, (T*)df, (T*)dg, P, HW, C, G,
                                                                                                       (float)(2.0 / (double)HW));
  });
  GM_LAUNCH_CHECK();
}

// ---- the slice gather of the 2.5-D path (and, with E = 1 and no index, the entry of the 2-D one) --------------------------------------------------------
// Slice m of the volume's N * E slices across one axis is (n, s) = (m / E, m % E); element (p0, p1) of its channel c is vol[n sN + c sC + s sA + p0 s0 + p1 s1].
template <typename Ti, typename To>
__global__ __launch_bounds__(256) void slice_gather_kernel(const Ti* __restrict__ vol, const long long* __restrict__ idx, To* __restrict__ out, long long total, int E,
                                                           int C, int P0, int P1, long long sN, long long sC, long long sA, long long s0, long long s1,
                                                           const float* __restrict__ shift, const float* __restrict__ scale) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int p1 = (int)(i % P1), p0 = (int)((i / P1) % P0);
    const long long mp = i / ((long long)P1 * P0), m = idx ? idx[mp] : mp;
    const Ti* src = vol + (m / E) * sN + (m % E) * sA + p0 * s0 + p1 * s1;
#pragma unroll
    for (int c = 0; c < 3; ++c) ElemIO<To>::st(out + i * 3 + c, (ElemIO<Ti>::ld(src + (C == 3 ? c * sC : 0)) - shift[c]) / scale[c]);
  }
}

// the adjoint: dvol (zero-filled by the entry point when there is an index) at the selected slices = gout / scale, the three channels summed where C = 1
template <typename Tg, typename Tv>
__global__ __launch_bounds__(256) void slice_gather_bwd_kernel(const Tg* __restrict__ gout, const long long* __restrict__ idx, Tv* __restrict__ dvol, long long total,
                                                               int E, int C, int P0, int P1, long long sN, long long sC, long long sA, long long s0, long long s1,
                                                               const float* __restrict__ scale) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
    const int p1 = (int)(i % P1), p0 = (int)((i / P1) % P0);
    const long long mp = i / ((long long)P1 * P0), m = idx ? idx[mp] : mp;
    Tv* dst = dvol + (m / E) * sN + (m % E) * sA + p0 * s0 + p1 * s1;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = ElemIO<Tg>::ld(gout + i * 3 + c) / scale[c];
    if (C == 3) {
#pragma unroll
      for (int c = 0; c < 3; ++c) ElemIO<Tv>::st(dst + c * sC, v[c]);
    } else {
      ElemIO<Tv>::st(dst, v[0] + v[1] + v[2]);
    }
  }
}

static int gather_check(const char* fn, long long Mp, int E, int C, int P0, int P1) {
  if (Mp < 1 || E < 1 || P0 < 1 || P1 < 1) { gm_set_error(fn, -1, "slice gather: empty selection or image"); return -1; }
  if (C != 1 && C != 3) { gm_set_error(fn, -1, "slice gather: the volume has 1 or 3 channels"); return -1; }
  return 0;
}
// (input type, output type) of the two gather kernels: equal, or fp32 -> bf16 forward / bf16 -> fp32 backward (fp32 volumes under bf16 autocast)
template <typename F> static inline bool gather_dispatch(int a, int b, F&& f) {
  if (a == GM_F32 && b == GM_F32) f(GmTV<float>{}, GmTV<float>{});
  else if (a == GM_BF16 && b == GM_BF16) f(GmTV<bf16_raw>{}, GmTV<bf16_raw>{});
  else if (a == GM_F32 && b == GM_BF16) f(GmTV<float>{}, GmTV<bf16_raw>{});
  else if (a == GM_BF16 && b == GM_F32) f(GmTV<bf16_raw>{}, GmTV<float>{});
  else return false;
  return true;
}

extern "C" int gm_slice_gather(const void* vol, const long long* idx, void* out, long long Mp, int E, int C, int P0, int P1, long long sN, long long sC,
                               long long sA, long long s0, long long s1, const float* shift, const float* scale, int in_dtype, int out_dtype, void* stream) {
  GM_REQUIRE(vol && out && shift && scale, "null pointer");
  if (gather_check(__func__, Mp, E, C, P0, P1)) return -1;
  hipStream_t st = (hipStream_t)stream;
  const long long total = Mp * P0 * P1;
  if (!gather_dispatch(in_dtype, out_dtype, [&](auto ti, auto to) {
        using Ti = typename decltype(ti)::type;
        using To = typename decltype(to)::type;
        slice_gather_kernel<Ti, To><<<stream_grid(total), 256, 0, st>>>((const Ti*)vol, idx, (To*)out, total, E, C, P0, P1, sN, sC, sA, s0, s1, shift, scale);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_slice_gather_bwd(const void* gout, const long long* idx, void* dvol, long long vol_elems, long long Mp, int E, int C, int P0, int P1,
                                   long long sN, long long sC, long long sA, long long s0, long long s1, const float* scale, int g_dtype, int vol_dtype,
                                   void* stream) {
  GM_REQUIRE(gout && dvol && scale, "null pointer");
  if (gather_check(__func__, Mp, E, C, P0, P1)) return -1;
  GM_REQUIRE(vol_elems >= Mp * P0 * P1 * C, "slice gather: the volume is smaller than the selection");
  hipStream_t st = (hipStream_t)stream;
  const long long total = Mp * P0 * P1;
  if (!gather_dispatch(g_dtype, vol_dtype, [&](auto tg, auto tvv) {
        using Tg = typename decltype(tg)::type;
        using Tv = typename decltype(tvv)::type;
        if (idx) (void)hipMemsetAsync(dvol, 0, (size_t)vol_elems * sizeof(Tv), st);  // (without an index the selection is every slice: each element is written)
        slice_gather_bwd_kernel<Tg, Tv><<<stream_grid(total), 256, 0, st>>>((const Tg*)gout, idx, (Tv*)dvol, total, E, C, P0, P1, sN, sC, sA, s0, s1, scale);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}
