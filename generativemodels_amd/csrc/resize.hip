// Separable resampling of an arena tensor (N, D, H, W, C): every mode of F.interpolate (align_corners = False, no antialiasing) and its gradient
// in ONE kernel (reference: networks/blocks/encoder_modules.py:60,77-78 -- SpatialRescaler's interpolation stages).
//   gm_resize_taps   y[n, o, c] = sum over the taps of (o_d, o_h, o_w) of (w_d * w_h) * w_w * x[n, i, c]
// Along one axis every mode is a short weighted sum: output index o reads the inputs index[start[o] .. start[o + 1]) with the weights
// weight[start[o] .. start[o + 1]) -- a CSR table per axis, computed on the HOST (generativemodels_amd/resize_plan.py: the fp32 source coordinate of
// torch decides the indices, so nothing of it is re-derived per element here).  The gradient is the same launch on the TRANSPOSED tables (per input
// index the outputs that read it, in ascending order) with the roles of x and y swapped: a gather through the inverted index, no atomics, and a
// fixed summation order -- bitwise reproducible.  HBM / cache bound: a lane owns one 16-byte channel group of one output voxel when the channel count,
// both leading dimensions and both base pointers allow it, else up to four channels read and written one by one (C = 1 .. 4 conditioning images:
// a voxel's channels then share one lane and one walk over the tables).  fp32 accumulation, one rounding on store.  No LDS.
#include "gm_common.h"

static int resize_grid(long long total, int per_block = 256) {
  long long g = (total + per_block - 1) / per_block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (int)g;
}

// G channels of one voxel -> fp32.  VEC: one 16-byte load (G = 4 fp32 / 8 bf16, all of them in range); else cn <= G scalar loads.
template <typename T, int G, bool VEC>
__device__ __forceinline__ void resize_load(const T* __restrict__ p, int cn, float (&v)[G]) {
  if constexpr (VEC) {
    VecIO<T, G>::ld(p, v);
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = j < cn ? ElemIO<T>::ld(p + j) : 0.0f;
  }
}

template <typename T, int G, bool VEC>
__device__ __forceinline__ void resize_store(T* __restrict__ p, int cn, const float (&a)[G]) {
  if constexpr (VEC) {
    if constexpr (sizeof(T) == 4) {
      f32x4_t q;
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = a[j];
      *reinterpret_cast<f32x4_t*>(p) = q;
    } else {
      uint4 q;
      q.x = pack_bf16x2(a[0], a[1]);
      q.y = pack_bf16x2(a[2], a[3]);
      q.z = pack_bf16x2(a[4], a[5]);
      q.w = pack_bf16x2(a[6], a[7]);
      *reinterpret_cast<uint4*>(p) = q;
    }
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j)
      if (j < cn) ElemIO<T>::st(p + j, a[j]);
  }
}

// one work item = (n, od, oh, ow, channel group), the group fastest: neighbouring lanes read neighbouring channels of the same input voxels.
// A wave whose outputs all have at most RESIZE_HOLD taps on the w axis (every forward table but a coarse `area`) holds those taps in registers across the
// d and h loops instead of re-reading the table for every (d, h) pair; the taps are visited in the same order either way, so both forms give the same bits.
#define RESIZE_HOLD 4
template <typename T, int G, bool VEC>
__global__ __launch_bounds__(256) void resize_taps_kernel(const T* __restrict__ x, long long x_ld, T* __restrict__ y, long long y_ld, int N, int C,
                                                         int groups, GmResizeDesc d) {
  const int Di = d.n_in[0], Hi = d.n_in[1], Wi = d.n_in[2], Do = d.n_out[0], Ho = d.n_out[1], Wo = d.n_out[2];
  const long long total = (long long)N * Do * Ho * Wo * groups;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int g = (int)(i % groups);
    long long r = i / groups;
    const int ow = (int)(r % Wo); r /= Wo;
    const int oh = (int)(r % Ho); r /= Ho;
    const int od = (int)(r % Do);
    const int n = (int)(r / Do);
    const int c0 = g * G, cn = min(G, C - c0);
    const int d0 = d.start[0][od], d1 = d.start[0][od + 1], h0 = d.start[1][oh], h1 = d.start[1][oh + 1], w0 = d.start[2][ow], w1 = d.start[2][ow + 1];
    const int nw = w1 - w0;
    const T* __restrict__ xc = x + c0;
    float acc[G];
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] = 0.0f;
    auto tap = [&](long long voxel, float w) {
      float v[G];
      resize_load<T, G, VEC>(xc + voxel * x_ld, cn, v);
#pragma unroll
      for (int j = 0; j < G; ++j) acc[j] = fmaf(w, v[j], acc[j]);
    };
    if (__all(nw <= RESIZE_HOLD)) {  // decided per wave: lanes that split over the two forms would run both
      int iw[RESIZE_HOLD];
      float ww[RESIZE_HOLD];
#pragma unroll
      for (int k = 0; k < RESIZE_HOLD; ++k) {
        iw[k] = k < nw ? d.index[2][w0 + k] : 0;
        ww[k] = k < nw ? d.weight[2][w0 + k] : 0.0f;
      }
      for (int td = d0; td < d1; ++td) {
        const float wd = d.weight[0][td];
        const long long pd = (long long)n * Di + d.index[0][td];
        for (int th = h0; th < h1; ++th) {
          const float wdh = wd * d.weight[1][th];
          const long long ph = (pd * Hi + d.index[1][th]) * Wi;
#pragma unroll
          for (int kw = 0; kw < RESIZE_HOLD; ++kw)
            if (kw < nw) tap(ph + iw[kw], wdh * ww[kw]);
        }
      }
    } else {
      for (int td = d0; td < d1; ++td) {
        const float wd = d.weight[0][td];
        const long long pd = (long long)n * Di + d.index[0][td];
        for (int th = h0; th < h1; ++th) {
          const float wdh = wd * d.weight[1][th];
          const long long ph = (pd * Hi + d.index[1][th]) * Wi;
          for (int tw = w0; tw < w1; ++tw) tap(ph + d.index[2][tw], wdh * d.weight[2][tw]);
        }
      }
    }
    const long long dst = (((long long)n * Do + od) * Ho + oh) * Wo + ow;
    resize_store<T, G, VEC>(y + dst * y_ld + c0, cn, acc);
  }
}

template <typename T>
static void resize_launch(const void* x, long long x_ld, void* y, long long y_ld, int N, int C, const GmResizeDesc& d, hipStream_t st) {
  constexpr int GV = 16 / (int)sizeof(T);
  const bool vec = C % GV == 0 && x_ld % GV == 0 && y_ld % GV == 0 && gm_aligned16(x) && gm_aligned16(y);
  const long long voxels = (long long)N * d.n_out[0] * d.n_out[1] * d.n_out[2];
  if (vec) {
    const int groups = C / GV;
    resize_taps_kernel<T, GV, true><<<resize_grid(voxels * groups), 256, 0, st>>>((const T*)x, x_ld, (T*)y, y_ld, N, C, groups, d);
  } else {
    const int groups = (C + 3) / 4;
    resize_taps_kernel<T, 4, false><<<resize_grid(voxels * groups), 256, 0, st>>>((const T*)x, x_ld, (T*)y, y_ld, N, C, groups, d);
  }
}

extern "C" int gm_resize_taps(const void* x, long long x_ld, void* y, long long y_ld, int N, int C, const GmResizeDesc* d, int dtype, void* stream) {
  GM_REQUIRE(x && y && d, "null pointer");
  GM_REQUIRE(N >= 0 && C >= 0 && x_ld >= C && y_ld >= C, "leading dimension smaller than the channel count");
  for (int a = 0; a < 3; ++a) {
    GM_REQUIRE(d->n_in[a] > 0 && d->n_out[a] > 0, "empty spatial extent");
    GM_REQUIRE(d->start[a] && d->index[a] && d->weight[a], "null table");
  }
  const bool empty = N == 0 || C == 0;  // (the dtype is refused before an empty problem returns)
  if (!gm_dispatch_dtype(dtype, [&](auto tv) {
        if (!empty) resize_launch<typename decltype(tv)::type>(x, x_ld, y, y_ld, N, C, *d, (hipStream_t)stream);
      })) GM_FAIL(-2, "unsupported dtype");
  if (empty) return 0;
  GM_LAUNCH_CHECK();
}
