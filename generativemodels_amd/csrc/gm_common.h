// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of generativemodels_amd.
// Everything here is wave64 / CDNA4 specific by design: no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gm_amd.h"       // the public interface (include/): every Gm* struct, GM_* constant and exported prototype, defined there only
#include "gm_internal.h"  // the cross-file helpers that are not part of it

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef uint16_t bf16_raw;  // storage type of a bf16 element in HBM / LDS

// ---- error plumbing shared by every extern "C" entry point (gm_set_error: capi.cpp) --------------------------------
#define GM_FAIL(code, msg)                 \
  do {                                     \
    gm_set_error(__func__, (code), (msg)); \
    return (code);                         \
  } while (0)
#define GM_REQUIRE(cond, msg) \
  do {                        \
    if (!(cond)) GM_FAIL(-1, msg); \
  } while (0)
#define GM_LAUNCH_CHECK()                                          \
  do {                                                             \
    hipError_t e__ = hipGetLastError();                            \
    if (e__ != hipSuccess) GM_FAIL((int)e__, hipGetErrorString(e__)); \
    return 0;                                                      \
  } while (0)

// ---- bf16 <-> f32 (round-to-nearest-even, NaN preserved) ------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(bf16_raw v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_raw f32_to_bf16(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_raw)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (bf16_raw)(u >> 16);
}

template <typename T> struct ElemIO;
template <> struct ElemIO<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct ElemIO<bf16_raw> {
  static __device__ __forceinline__ float ld(const bf16_raw* p) { return bf16_to_f32(*p); }
  static __device__ __forceinline__ void st(bf16_raw* p, float v) { *p = f32_to_bf16(v); }
};
template <> struct ElemIO<_Float16> {  // (inputs of the metric kernels only: gm_dispatch_dtype_f16)
  static __device__ __forceinline__ float ld(const _Float16* p) { return (float)*p; }
  static __device__ __forceinline__ void st(_Float16* p, float v) { *p = (_Float16)v; }
};

// two fp32 -> packed bf16x2 (lo in bits 0..15) with the gfx950 hardware converter (round-to-nearest-even)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// 16-byte operand vector <-> 4/8 floats
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static __device__ __forceinline__ void unpack(const uint4& v, float* o) {
    o[0] = __uint_as_float(v.x); o[1] = __uint_as_float(v.y); o[2] = __uint_as_float(v.z); o[3] = __uint_as_float(v.w);
  }
  static __device__ __forceinline__ uint4 pack(const float* o) {
    return make_uint4(__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3]));
  }
};
template <> struct Vec16<bf16_raw> {
  static __device__ __forceinline__ void unpack(const uint4& v, float* o) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[2 * i] = __uint_as_float(w[i] << 16); o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ uint4 pack(const float* o) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf16x2(o[2 * i], o[2 * i + 1]);
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};

// ---- the IO of the streaming (memory-bound) kernels: VEC consecutive elements <-> VEC floats.  VEC = 16 / sizeof(T) is one 16-byte access (the host
// has checked the alignment of the base, the pitches and the channel count: gm_aligned16 and the entry point's vec_ok), VEC = 1 is ElemIO. -------------
template <typename T, int VEC> struct VecIO {
  static_assert(VEC * sizeof(T) == 16, "a vector access is 16 bytes: 4 fp32 or 8 bf16");
  static __device__ __forceinline__ void ld(const T* p, float* o) { Vec16<T>::unpack(*reinterpret_cast<const uint4*>(p), o); }
  static __device__ __forceinline__ void st(T* p, const float* v) { *reinterpret_cast<uint4*>(p) = Vec16<T>::pack(v); }
};
template <typename T> struct VecIO<T, 1> {
  static __device__ __forceinline__ void ld(const T* p, float* o) { o[0] = ElemIO<T>::ld(p); }
  static __device__ __forceinline__ void st(T* p, const float* v) { ElemIO<T>::st(p, v[0]); }
};
static inline bool gm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- host dispatch over the storage type of a streaming entry point.  `f` is a generic lambda that launches for the tag it is given
// (`using T = typename decltype(tv)::type`, `decltype(tv)::vec`); the result says whether the dtype is served.  The refusal stays in the entry point's
// own body -- `if (!gm_dispatch_dtype(dtype, [&](auto tv) {...})) GM_FAIL(-2, "unsupported dtype");` -- because GM_FAIL records __func__. ----------------
template <typename T, int VEC = 1> struct GmTV { using type = T; static constexpr int vec = VEC; };
template <typename F> static inline bool gm_dispatch_dtype(int dtype, F&& f) {
  if (dtype == GM_F32) f(GmTV<float>{});
  else if (dtype == GM_BF16) f(GmTV<bf16_raw>{});
  else return false;
  return true;
}
// the three metric entry points also read fp16
template <typename F> static inline bool gm_dispatch_dtype_f16(int dtype, F&& f) {
  if (dtype == GM_F16) { f(GmTV<_Float16>{}); return true; }
  return gm_dispatch_dtype(dtype, f);
}
// (type, vector width): the 16-byte form where the entry point's vec_ok holds, else one element per access
template <typename F> static inline bool gm_dispatch_vec(int dtype, bool vec_ok, F&& f) {
  if (dtype == GM_F32) { if (vec_ok) f(GmTV<float, 4>{}); else f(GmTV<float, 1>{}); }
  else if (dtype == GM_BF16) { if (vec_ok) f(GmTV<bf16_raw, 8>{}); else f(GmTV<bf16_raw, 1>{}); }
  else return false;
  return true;
}
// fast SiLU for the bf16 path: v_exp_f32 + v_rcp_f32 (about 1 ulp each; far below bf16 resolution)
__device__ __forceinline__ float gm_silu(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float gm_silu_precise(float x) { return x / (1.0f + expf(-x)); }

// wave64 butterfly reductions
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- GroupNorm finalisation over SHORT statistic tables (every source S <= GM_GN_SHORT_MAX_ROWS rows of [N][C_i][2] fp64 partials) -- shared by gm_gn_finalize_channels
// (groupnorm.hip) and the consumer-side prologues (gn_short_table below), which must agree bit for bit: a channel's partials are added in ROW order, a group is the sum
// of its channels in CHANNEL order, everything in fp64.  Channel c of the concatenation (C0 + C1 channels) lives in source 0 when c < C0.
// (the bound was 64 until the second half of round 6: the 32^3 level of a latent UNet leaves 128-row tables -- one partial per 256-voxel tile)
__device__ __forceinline__ double2 gn_short_channel_sum(const double* s0, int S0, int C0, const double* s1, int S1, int C1, int N, int n, int c) {
  const bool first = c < C0;
  const double* src = first ? s0 + ((long long)n * C0 + c) * 2 : s1 + ((long long)n * C1 + (c - C0)) * 2;
  const long long pitch = (long long)N * (first ? C0 : C1) * 2;
  const int S = first ? S0 : S1;
  double a = 0.0, b = 0.0;
  int sl = 0;
  for (; sl + 8 <= S; sl += 8) {  // eight rows in flight, added in row order
    double2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const double2*>(src + (long long)(sl + k) * pitch);
#pragma unroll
    for (int k = 0; k < 8; ++k) { a += v[k].x; b += v[k].y; }
  }
  for (; sl < S; ++sl) {
    const double2 v = *reinterpret_cast<const double2*>(src + (long long)sl * pitch);
    a += v.x; b += v.y;
  }
  return make_double2(a, b);
}
// (a, b) = the group's (sum, sum of squares) over cpg channels x V voxels -> this channel's scale = rstd * gamma, shift = beta - mean * rstd * gamma
__device__ __forceinline__ void gn_short_scale_shift(double a, double b, int cpg, long long V, float eps, float gamma, float beta, float& scale, float& shift) {
  const double cnt = (double)cpg * (double)V;
  const double mean = a / cnt;
  double var = b / cnt - mean * mean;
  if (var < 0.0) var = 0.0;
  const double rstd = 1.0 / sqrt(var + (double)eps);
  scale = (float)(rstd * (double)gamma);
  shift = (float)((double)beta - mean * rstd * (double)gamma);
}
// The finalisation in a CONSUMER's prologue (conv_sn.hip, conv_sk.hip, token_gemm_wide_kernel), by all NT threads of a work-group, for sample n: the channel sums
// of the whole groups [cov0, cov1) into csum[c - cov0] (a thread owns a channel: rows in row order), then scale / shift of channels [ch0, ch1) into
// tab[c - ch0] / tab[sh_off + c - ch0] (a group = its channels' sums in channel order); a barrier behind each step.  V = voxels of the normalised tensor.
// Only gn_short_channel_sum / gn_short_scale_shift do arithmetic here, in the order of gm_gn_finalize_channels' short form: the tables agree bit for bit.
template <int NT>
__device__ __forceinline__ void gn_short_table(float* tab, int sh_off, double* csum, int ch0, int ch1, int cov0, int cov1, int cpg, const double* s0, int S0, int C0,
                                               const double* s1, int S1, int C1, int N, int n, long long V, float eps, const float* gamma, const float* beta, int tid) {
  for (int c = cov0 + tid; c < cov1; c += NT) {
    const double2 v = gn_short_channel_sum(s0, S0, C0, s1, S1, C1, N, n, c);
    csum[2 * (c - cov0)] = v.x; csum[2 * (c - cov0) + 1] = v.y;
  }
  __syncthreads();
  for (int c = ch0 + tid; c < ch1; c += NT) {
    const int g = c / cpg;
    double a = 0.0, b = 0.0;
    for (int j = 0; j < cpg; ++j) { a += csum[2 * (g * cpg + j - cov0)]; b += csum[2 * (g * cpg + j - cov0) + 1]; }
    float sc, sh;
    gn_short_scale_shift(a, b, cpg, V, eps, gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f, sc, sh);
    tab[c - ch0] = sc;
    tab[sh_off + (c - ch0)] = sh;
  }
  __syncthreads();
}

static inline int gm_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
