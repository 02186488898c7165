// The classifier head of DiffusionModelEncoder (networks/nets/diffusion_model_unet.py): Linear(F, H) -> ReLU -> Dropout -> Linear(H, K) over the
// flattened feature map, forward and backward, reading the channels-last arena directly.
//
// The reference flattens N C [D] H W, so column f of W1 belongs to (channel c, voxel s) with f = c * S + s, while the arena holds (voxel, channel).
// W1 (H x F, 8 MB in fp32 at F = 4096, H = 512) is never permuted or copied: the SMALL operand, a chunk of samples of the N x F activations, is
// transposed through LDS into the weight's column order (head_stage_transposed), and every kernel walks W1 along its rows with 16-byte loads.
// All sums are fp32 in a fixed order (a lane's strided partial, the wave butterfly, a fixed LDS fold): no atomics, two runs agree bit for bit.
//   gm_head_hidden    a = relu(W1 h + b1) * mask                     one wave per hidden row, the chunk's activations in LDS
//   gm_head_tail      logits = W2 a + b2; with labels y: logp = log_softmax(logits)[y] and e = onehot(y) - softmax(logits); with g: e = g;
//                     da = W2^T e -- one launch, one work-group per sample, softmax in fp32
//   gm_head_dinput    dh[n, s, c] = sum_j dz[n, j] W1[j, c S + s],  dz = da * mask * [a > 0]; grid over feature slabs, stored in arena layout
//   gm_head_dparams   dW1 (reference column order), db1, dW2, db2 as sums over the samples in sample order; honours `accumulate`
// dtype is the storage type of the activations (h, a, mask, g, logits, dh), wdtype that of the parameters: (fp32, fp32), (bf16, bf16) and bf16
// activations with fp32 parameters (autocast).  da and every parameter gradient are fp32.
#include <stdio.h>
#include "gm_common.h"

#define HEAD_LDS_BYTES 65536  // the staged chunk: gm_head_chunk(dtype) samples x F elements
#define HEAD_MAX_F 4096
#define HEAD_MAX_H 4096
#define HEAD_MAX_K 1024

// V consecutive elements -> V floats in one 8- or 16-byte access
template <typename T, int V> struct HeadLd;
template <> struct HeadLd<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* o) { Vec16<float>::unpack(*reinterpret_cast<const uint4*>(p), o); }
};
template <> struct HeadLd<bf16_raw, 8> {
  static __device__ __forceinline__ void ld(const bf16_raw* p, float* o) { Vec16<bf16_raw>::unpack(*reinterpret_cast<const uint4*>(p), o); }
};
template <> struct HeadLd<bf16_raw, 4> {
  static __device__ __forceinline__ void ld(const bf16_raw* p, float* o) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  }
};
template <typename T> __device__ __forceinline__ float head_round(float v);  // v as the storage type holds it
template <> __device__ __forceinline__ float head_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float head_round<bf16_raw>(float v) { return bf16_to_f32(f32_to_bf16(v)); }

static inline int head_chunk(int dtype) { return dtype == GM_F32 ? 4 : dtype == GM_BF16 ? 8 : -1; }
// a wave of the staging loop reads 2^ts voxels x 64 / 2^ts channels: the largest power of two up to 16 that divides S
static inline int head_ts_log2(int S) {
  int t = 0;
  while (t < 4 && S % (2 << t) == 0) ++t;
  return t;
}

// samples [n0, n0 + nc) of the arena h (N, S, C; `ld` elements between voxels) into LDS in W1's column order: hT[n * F + c * S + s].  Consecutive lanes take
// 2^ts consecutive voxels of one channel, then the next channel: the LDS stores of a 32-lane half fall on 32 / 2^ts rows S apart (2-way conflicts at
// ts = 4), the global loads on 2^ts rows of 64 / 2^ts contiguous channels.
template <typename TA>
__device__ __forceinline__ void head_stage_transposed(TA* hT, const TA* __restrict__ h, long long ld, int S, int C, int n0, int nc, int ts, int tid, int nthreads) {
  const int F = S * C, mask = (1 << ts) - 1;
  for (int i = tid; i < nc * F; i += nthreads) {
    const int n = i / F;
    int r = i - n * F;
    const int sl = r & mask;
    r >>= ts;
    const int st = r / C, c = r - st * C;
    const int s = (st << ts) + sl;
    hT[n * F + c * S + s] = h[((long long)(n0 + n) * S + s) * ld + c];
  }
}

// dz[n, j] = da * mask * [a > 0]  (mask == 0 leaves a == 0, so [a > 0] is [z > 0] wherever the product is not 0 anyway)
template <typename TA>
__device__ __forceinline__ float head_dz(const float* __restrict__ da, const TA* __restrict__ a, const TA* __restrict__ mask, long long idx) {
  if (!(ElemIO<TA>::ld(a + idx) > 0.f)) return 0.f;
  return mask ? da[idx] * ElemIO<TA>::ld(mask + idx) : da[idx];
}

// ---- a = relu(W1 h + b1) * mask: 4 hidden rows per work-group, one per wave; samples [n0, n0 + NC) of the batch -------------------------------------------
template <typename TA, typename TP, int NC>
__global__ __launch_bounds__(256) void head_hidden_kernel(const TA* __restrict__ h, long long ld, int S, int C, int ts, const TP* __restrict__ w1,
                                                         const TP* __restrict__ b1, const TA* __restrict__ mask, TA* __restrict__ a, int N, int H, int n0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_lds[];
  TA* hT = reinterpret_cast<TA*>(head_lds);
  constexpr int VW = 16 / sizeof(TP);
  const int F = S * C;
  const int nc = N - n0 < NC ? N - n0 : NC;
  head_stage_transposed<TA>(hT, h, ld, S, C, n0, nc, ts, threadIdx.x, 256);
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + wave;
  if (j >= H) return;  // (behind the only barrier)
  float acc[NC];
#pragma unroll
  for (int n = 0; n < NC; ++n) acc[n] = 0.f;
  const TP* wr = w1 + (long long)j * F;
#pragma unroll 4
  for (int f = lane * VW; f < F; f += 64 * VW) {
    float wv[VW];
    HeadLd<TP, VW>::ld(wr + f, wv);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      if (n < nc) {
        float hv[VW];
        HeadLd<TA, VW>::ld(hT + n * F + f, hv);
#pragma unroll
        for (int v = 0; v < VW; ++v) acc[n] = fmaf(wv[v], hv[v], acc[n]);
      }
    }
  }
  const float bias = b1 ? ElemIO<TP>::ld(b1 + j) : 0.f;
#pragma unroll
  for (int n = 0; n < NC; ++n) {
    if (n < nc) {
      const float z = wave_sum(acc[n]) + bias;
      if (lane == 0) {
        const long long idx = (long long)(n0 + n) * H + j;
        float v = z > 0.f ? z : 0.f;
        if (mask) v *= ElemIO<TA>::ld(mask + idx);
        ElemIO<TA>::st(a + idx, v);
      }
    }
  }
}

// ---- logits, log-probability of the label and da: one work-group per sample ----------------------------------------------------------------------------------
template <typename TA, typename TP>
__global__ __launch_bounds__(256) void head_tail_kernel(const TA* __restrict__ a, const TP* __restrict__ w2, const TP* __restrict__ b2, const long long* __restrict__ y,
                                                       const TA* __restrict__ g, TA* __restrict__ logits, float* __restrict__ logp, float* __restrict__ da, int H,
                                                       int K) {
  __shared__ float sa[HEAD_MAX_H];
  __shared__ float e[HEAD_MAX_K];
  __shared__ float red[256];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const long long n = blockIdx.x;
  if (!g) {  // (every branch on a pointer is uniform over the work-group)
    for (int j = t; j < H; j += 256) sa[j] = ElemIO<TA>::ld(a + n * H + j);
    __syncthreads();
    for (int k = wave; k < K; k += 4) {
      const TP* wr = w2 + (long long)k * H;
      float acc = 0.f;
      for (int j = lane; j < H; j += 64) acc = fmaf(ElemIO<TP>::ld(wr + j), sa[j], acc);
      acc = head_round<TA>(wave_sum(acc) + (b2 ? ElemIO<TP>::ld(b2 + k) : 0.f));  // the softmax reads the logits as they are stored
      if (lane == 0) {
        e[k] = acc;
        if (logits) ElemIO<TA>::st(logits + n * K + k, acc);
      }
    }
    __syncthreads();
    if (y) {
      float m = -INFINITY;
      for (int k = t; k < K; k += 256) m = fmaxf(m, e[k]);
      red[t] = m;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
      }
      m = red[0];
      __syncthreads();
      float z = 0.f;
      for (int k = t; k < K; k += 256) z += expf(e[k] - m);
      red[t] = z;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
      }
      z = red[0];
      const long long label = y[n];
      const bool valid = label >= 0 && label < K;  // (a label outside [0, K): logp is NaN and no class is the target)
      const float lp = valid ? e[valid ? label : 0] - m - logf(z) : __uint_as_float(0x7fc00000u);
      __syncthreads();  // e[label] is read above, e is rewritten below
      if (t == 0 && logp) logp[n] = lp;
      for (int k = t; k < K; k += 256) e[k] = (k == label ? 1.f : 0.f) - expf(e[k] - m) / z;
      __syncthreads();
    }
  } else {
    for (int k = t; k < K; k += 256) e[k] = ElemIO<TA>::ld(g + n * K + k);
    __syncthreads();
  }
  if (da) {
    for (int j = t; j < H; j += 256) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(ElemIO<TP>::ld(w2 + (long long)k * H + j), e[k], acc);
      da[n * H + j] = acc;
    }
  }
}

// ---- dh: a slab of 8 weight vectors (8 * VW features) per work-group; thread (rg, l8) adds the hidden rows rg, rg + 32, ... in row order, the 32 partials of a
// feature are folded in rg order ---------------------------------------------------------------------------------------------------------------------------------
template <typename TA, typename TP, int NC>
__global__ __launch_bounds__(256) void head_dinput_kernel(const float* __restrict__ da, const TA* __restrict__ a, const TA* __restrict__ mask, const TP* __restrict__ w1,
                                                         TA* __restrict__ dh, long long ld, int S, int C, int N, int H, int n0) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_lds[];
  constexpr int VW = 16 / sizeof(TP), FB = 8 * VW;
  float* dz = reinterpret_cast<float*>(head_lds);  // [NC][H]
  float* part = dz + NC * H;                       // [32][FB]
  const int F = S * C;
  const int nc = N - n0 < NC ? N - n0 : NC;
  const int t = threadIdx.x, rg = t >> 3, l8 = t & 7;
  const int f0 = blockIdx.x * FB;
  for (int i = t; i < nc * H; i += 256) dz[i] = head_dz<TA>(da, a, mask, (long long)n0 * H + i);
  __syncthreads();
  float acc[NC][VW];
#pragma unroll
  for (int n = 0; n < NC; ++n)
#pragma unroll
    for (int v = 0; v < VW; ++v) acc[n][v] = 0.f;
#pragma unroll 4
  for (int j = rg; j < H; j += 32) {
    float wv[VW];
    HeadLd<TP, VW>::ld(w1 + (long long)j * F + f0 + l8 * VW, wv);
#pragma unroll
    for (int n = 0; n < NC; ++n) {
      if (n < nc) {
        const float d = dz[n * H + j];
#pragma unroll
        for (int v = 0; v < VW; ++v) acc[n][v] = fmaf(d, wv[v], acc[n][v]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < NC; ++n) {
    if (n < nc) {  // (uniform: every thread reaches the barriers)
#pragma unroll
      for (int v = 0; v < VW; ++v) part[rg * FB + l8 * VW + v] = acc[n][v];
      __syncthreads();
      if (t < FB) {
        float sum = 0.f;
        for (int r = 0; r < 32; ++r) sum += part[r * FB + t];
        const int f = f0 + t, c = f / S, s = f - c * S;
        ElemIO<TA>::st(dh + ((long long)(n0 + n) * S + s) * ld + c, sum);
      }
      __syncthreads();
    }
  }
}

// ---- dW1 / db1: 8 hidden rows per work-group; the samples pass through LDS chunk by chunk, a row of dW1 is read-modified-written by its one owner ------------
template <typename TA>
__global__ __launch_bounds__(256) void head_dw1_kernel(const TA* __restrict__ h, long long ld, int S, int C, int ts, const float* __restrict__ da, const TA* __restrict__ a,
                                                      const TA* __restrict__ mask, float* __restrict__ dw1, float* __restrict__ db1, int N, int H, int chunk,
                                                      int accumulate) {
  extern __shared__ __attribute__((aligned(16))) unsigned char head_lds[];
  TA* hT = reinterpret_cast<TA*>(head_lds);
  __shared__ float dzs[8 * 8];  // [row][sample of the chunk]
  const int F = S * C, t = threadIdx.x;
  const int j0 = blockIdx.x * 8;
  for (int n0 = 0; n0 < N; n0 += chunk) {
    const int nc = N - n0 < chunk ? N - n0 : chunk;
    __syncthreads();  // the previous chunk has been read
    head_stage_transposed<TA>(hT, h, ld, S, C, n0, nc, ts, t, 256);
    if (t < 64) {
      const int jj = t >> 3, n = t & 7, j = j0 + jj;
      dzs[t] = (j < H && n < nc) ? head_dz<TA>(da, a, mask, (long long)(n0 + n) * H + j) : 0.f;
    }
    __syncthreads();
    if (dw1) {
      for (int jj = 0; jj < 8 && j0 + jj < H; ++jj) {
        float* row = dw1 + (long long)(j0 + jj) * F;
        for (int f = t * 4; f < F; f += 1024) {
          float o[4] = {0.f, 0.f, 0.f, 0.f};
          for (int n = 0; n < nc; ++n) {
            float hv[4];
            HeadLd<TA, 4>::ld(hT + n * F + f, hv);
            const float d = dzs[jj * 8 + n];
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] = fmaf(d, hv[v], o[v]);
          }
          if (n0 > 0 || accumulate) {
            float old[4];
            HeadLd<float, 4>::ld(row + f, old);
#pragma unroll
            for (int v = 0; v < 4; ++v) o[v] += old[v];
          }
          *reinterpret_cast<uint4*>(row + f) = Vec16<float>::pack(o);
        }
      }
    }
  }
  if (db1 && t < 8 && j0 + t < H) {
    const int j = j0 + t;
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += head_dz<TA>(da, a, mask, (long long)n * H + j);
    db1[j] = accumulate ? db1[j] + sum : sum;
  }
}

// ---- dW2[k, j] = sum_n g[n, k] a[n, j], db2[k] = sum_n g[n, k]: one work-group per class --------------------------------------------------------------------
template <typename TA>
__global__ __launch_bounds__(256) void head_dw2_kernel(const TA* __restrict__ g, const TA* __restrict__ a, float* __restrict__ dw2, float* __restrict__ db2, int N, int H, int K,
                                                      int accumulate) {
  const int k = blockIdx.x, t = threadIdx.x;
  if (dw2) {
    for (int j = t; j < H; j += 256) {
      float sum = 0.f;
      for (int n = 0; n < N; ++n) sum = fmaf(ElemIO<TA>::ld(g + (long long)n * K + k), ElemIO<TA>::ld(a + (long long)n * H + j), sum);
      float* o = dw2 + (long long)k * H + j;
      *o = accumulate ? *o + sum : sum;
    }
  }
  if (db2 && t == 0) {
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += ElemIO<TA>::ld(g + (long long)n * K + k);
    db2[k] = accumulate ? db2[k] + sum : sum;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------
// (activations, parameters): fp32 / fp32, bf16 / bf16, bf16 / fp32
template <typename Fn> static inline bool head_dispatch(int dtype, int wdtype, Fn&& f) {
  if (dtype == GM_F32 && wdtype == GM_F32) f(GmTV<float>{}, GmTV<float>{});
  else if (dtype == GM_BF16 && wdtype == GM_BF16) f(GmTV<bf16_raw>{}, GmTV<bf16_raw>{});
  else if (dtype == GM_BF16 && wdtype == GM_F32) f(GmTV<bf16_raw>{}, GmTV<float>{});
  else return false;
  return true;
}
// the smallest instantiated chunk that holds nc samples
static inline int head_nc(int nc) { return nc <= 1 ? 1 : nc <= 2 ? 2 : nc <= 4 ? 4 : 8; }

static char head_msg[160];
#define HEAD_REQUIRE_VALUE(cond, fmt, value)                     \
  do {                                                           \
    if (!(cond)) {                                               \
      snprintf(head_msg, sizeof(head_msg), fmt, (long long)(value)); \
      GM_FAIL(-1, head_msg);                                     \
    }                                                            \
  } while (0)

// the shape checks the four entry points share; slab = the feature multiple the caller's kernel assumes
#define HEAD_CHECK_SHAPE(slab)                                                                                                              \
  GM_REQUIRE(N >= 0 && S > 0 && C > 0 && H > 0, "N, S, C, H: non-negative batch, positive extents");                                    \
  HEAD_REQUIRE_VALUE((long long)S * C <= HEAD_MAX_F, "F = S * C = %lld: the staged chunk holds at most 4096 features per sample", (long long)S * C); \
  HEAD_REQUIRE_VALUE(((long long)S * C) % (slab) == 0, "F = S * C = %lld is not a multiple of the kernel's feature slab", (long long)S * C);       \
  HEAD_REQUIRE_VALUE(H <= HEAD_MAX_H, "H = %lld: at most 4096 hidden units", H)

extern "C" int gm_head_chunk(int dtype) { return head_chunk(dtype); }

extern "C" int gm_head_hidden(const void* h, long long h_ld, int N, int S, int C, const void* w1, const void* b1, const void* mask, void* a, int H, int dtype,
                              int wdtype, void* stream) {
  GM_REQUIRE(h && w1 && a, "null pointer");
  HEAD_CHECK_SHAPE(wdtype == GM_BF16 ? 8 : 4);
  GM_REQUIRE(h_ld >= C, "leading dimension smaller than the channel count");
  GM_REQUIRE(gm_aligned16(w1), "W1 must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int chunk = head_chunk(dtype), ts = head_ts_log2(S);
  if (!head_dispatch(dtype, wdtype, [&](auto ta, auto tp) {
        using TA = typename decltype(ta)::type;
        using TP = typename decltype(tp)::type;
        const dim3 grid(gm_cdiv(H, 4));
        for (int n0 = 0; n0 < N; n0 += chunk) {  // one launch per chunk of samples
          const int nc = head_nc(N - n0 < chunk ? N - n0 : chunk);
          const size_t lds = (size_t)nc * S * C * sizeof(TA);  // <= HEAD_LDS_BYTES: nc <= chunk, F <= HEAD_MAX_F
#define HEAD_GO(NC_)                                                                                                                              \
  head_hidden_kernel<TA, TP, NC_><<<grid, 256, lds, st>>>((const TA*)h, h_ld, S, C, ts, (const TP*)w1, (const TP*)b1, (const TA*)mask, (TA*)a, N, H, n0)
          if (nc == 1) HEAD_GO(1);
          else if (nc == 2) HEAD_GO(2);
          else if (nc == 4) HEAD_GO(4);
          else if constexpr (sizeof(TA) == 2) HEAD_GO(8);
#undef HEAD_GO
        }
      })) GM_FAIL(-2, "unsupported dtype pair: fp32 / fp32, bf16 / bf16 or bf16 activations with fp32 parameters");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_head_tail(const void* a, const void* w2, const void* b2, const long long* y, const void* g, void* logits, float* logp, float* da, int N, int H,
                            int K, int dtype, int wdtype, void* stream) {
  GM_REQUIRE(w2 && (a || g), "null pointer");
  GM_REQUIRE(N >= 0 && H > 0, "N, H: non-negative batch, positive width");
  HEAD_REQUIRE_VALUE(H <= HEAD_MAX_H, "H = %lld: at most 4096 hidden units", H);
  HEAD_REQUIRE_VALUE(K >= 1 && K <= HEAD_MAX_K, "K = %lld: 1 .. 1024 classes", K);
  GM_REQUIRE(!(y && g), "one source of the output gradient: labels or g");
  GM_REQUIRE(g || a, "the logits need a");
  GM_REQUIRE(!logp || y, "logp needs labels");
  GM_REQUIRE(!da || y || g, "da needs labels or g");
  GM_REQUIRE(logits || logp || da, "nothing to write");
  hipStream_t st = (hipStream_t)stream;
  if (!head_dispatch(dtype, wdtype, [&](auto ta, auto tp) {
        using TA = typename decltype(ta)::type;
        using TP = typename decltype(tp)::type;
        if (N == 0) return;
        head_tail_kernel<TA, TP><<<N, 256, 0, st>>>((const TA*)a, (const TP*)w2, (const TP*)b2, y, (const TA*)g, (TA*)logits, logp, da, H, K);
      })) GM_FAIL(-2, "unsupported dtype pair: fp32 / fp32, bf16 / bf16 or bf16 activations with fp32 parameters");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_head_dinput(const float* da, const void* a, const void* mask, const void* w1, void* dh, long long dh_ld, int N, int S, int C, int H, int dtype,
                              int wdtype, void* stream) {
  GM_REQUIRE(da && a && w1 && dh, "null pointer");
  HEAD_CHECK_SHAPE(wdtype == GM_BF16 ? 64 : 32);
  GM_REQUIRE(dh_ld >= C, "leading dimension smaller than the channel count");
  GM_REQUIRE(gm_aligned16(w1), "W1 must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int chunk = head_chunk(dtype);
  {  // the first launch holds the most samples: its dz table [nc][H] and the fold buffer [32][slab] must fit what a launch stages in LDS
    const long long nc_max = head_nc(N < chunk ? N : chunk), slab = wdtype == GM_BF16 ? 64 : 32;
    HEAD_REQUIRE_VALUE(chunk < 0 || (nc_max * H + 32 * slab) * 4 <= HEAD_LDS_BYTES, "H = %lld: the chunk's dz table does not fit the 64 KiB of LDS of a launch", H);
  }
  if (!head_dispatch(dtype, wdtype, [&](auto ta, auto tp) {
        using TA = typename decltype(ta)::type;
        using TP = typename decltype(tp)::type;
        constexpr int FB = 8 * (16 / (int)sizeof(TP));
        const dim3 grid(S * C / FB);
        for (int n0 = 0; n0 < N; n0 += chunk) {
          const int nc = head_nc(N - n0 < chunk ? N - n0 : chunk);
          const size_t lds = ((size_t)nc * H + 32 * FB) * sizeof(float);  // <= HEAD_LDS_BYTES: checked above for the largest nc
#define HEAD_GO(NC_)                                                                                                                                  \
  head_dinput_kernel<TA, TP, NC_><<<grid, 256, lds, st>>>(da, (const TA*)a, (const TA*)mask, (const TP*)w1, (TA*)dh, dh_ld, S, C, N, H, n0)
          if (nc == 1) HEAD_GO(1);
          else if (nc == 2) HEAD_GO(2);
          else if (nc == 4) HEAD_GO(4);
          else if constexpr (sizeof(TA) == 2) HEAD_GO(8);
#undef HEAD_GO
        }
      })) GM_FAIL(-2, "unsupported dtype pair: fp32 / fp32, bf16 / bf16 or bf16 activations with fp32 parameters");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_head_dparams(const void* h, long long h_ld, const float* da, const void* a, const void* mask, const void* g, float* dw1, float* db1, float* dw2,
                               float* db2, int N, int S, int C, int H, int K, int accumulate, int dtype, void* stream) {
  GM_REQUIRE(a, "null pointer");
  GM_REQUIRE(!(dw1 || db1) || (h && da), "dW1 / db1 need h and da");
  GM_REQUIRE(!(dw2 || db2) || g, "dW2 / db2 need g");
  GM_REQUIRE(dw1 || db1 || dw2 || db2, "nothing to write");
  HEAD_CHECK_SHAPE(4);
  HEAD_REQUIRE_VALUE(K >= 1 && K <= HEAD_MAX_K, "K = %lld: 1 .. 1024 classes", K);
  GM_REQUIRE(!h || h_ld >= C, "leading dimension smaller than the channel count");
  GM_REQUIRE(!dw1 || gm_aligned16(dw1), "dW1 must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // (half a chunk per pass: with the kernel's static table the staged samples stay inside the 64 KiB a launch may ask for without opting in to more)
  const int chunk = head_chunk(dtype) / 2, ts = head_ts_log2(S);
  if (!gm_dispatch_dtype(dtype, [&](auto tv) {
        using TA = typename decltype(tv)::type;
        if (dw1 || db1)
          head_dw1_kernel<TA><<<gm_cdiv(H, 8), 256, (size_t)chunk * S * C * sizeof(TA), st>>>((const TA*)h, h_ld, S, C, ts, da, (const TA*)a, (const TA*)mask, dw1, db1, N,
                                                                                            H, chunk, accumulate);
        if (dw2 || db2) head_dw2_kernel<TA><<<K, 256, 0, st>>>((const TA*)g, (const TA*)a, dw2, db2, N, H, K, accumulate);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}
