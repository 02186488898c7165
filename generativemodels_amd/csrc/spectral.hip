// Discrete Fourier transforms of real NC[D]HW tensors over the channel axis and every spatial axis, and the spectral (Jukebox) loss on them
// (reference: losses/spectral_loss.py:56-87 -- fftn, the amplitude, the squared difference).
//   gm_dft_lines       one pass of 1-D transforms over a grid of lines: mixed-radix Stockham autosort between two LDS buffers
//   gm_spectral_loss   (|X| - |Y|)^2 over two half spectra: the reduced value, the full map, and / or the spectra of the gradient
// The passes, their order, the radices of every stage and the twiddle tables come from the HOST planner (generativemodels_amd/spectral_plan.py), whose NumPy
// emulator runs the same stages; nothing of the plan is re-derived here.  A stage of radix r over a line of N = n * s points (s = the product of the radices
// before it, m = n / r), for p < m, q < s, u < r:
//     out[q + s * (r * p + u)] = (sum over t < r of in[q + s * (p + t * m)] * w_r^(t u)) * w_N^(s p u)
// Radices 2, 3, 4 and 5 have their own butterflies (one work item per (p, q)); any other prime is evaluated directly (one work item per output).  A work-group
// stages L lines of one pass: with unit stride along the transformed axis a line is read along itself, otherwise the L lines are neighbours on the tensor's
// innermost axis and are read across -- coalesced either way.  The LDS line stride is N | 1 complex numbers: odd, so that the lines of a power-of-two length do
// not start on one bank when they are read across.  All arithmetic is fp32; bf16 / fp16 operands are converted on load, the gradient once on store.
// Reductions are per work-group fp64 partials folded in a fixed order: no atomics, bit-reproducible.
#include "gm_common.h"

#define DFT_COMPLEX 3       // complex fp32 lines
#define DFT_HERMITIAN 4     // source only: a line holds the n / 2 + 1 bins of a Hermitian spectrum, expanded to n on load
#define DFT_THREADS 256
#define DFT_MAX_LINES 64    // lines per work-group (a power of two)
#define DFT_TILE_POINTS 5056  // L * stride at most this (79 KiB of line buffers + the 1 KiB line table: two work-groups per CU) unless one line alone is longer
#define DFT_LDS_BYTES (160 * 1024)
#define DFT_LINE_TABLE_BYTES 1024  // DFT_MAX_LINES x (source, destination) offsets
#define DFT_MAX_STAGES 16
#define DFT_MAX_LENGTH ((DFT_LDS_BYTES - DFT_LINE_TABLE_BYTES) / 16 - 1)
static_assert(sizeof(GmDftDesc::radix) == DFT_MAX_STAGES * sizeof(int), "GmDftDesc.radix (include/gm_amd.h) holds DFT_MAX_STAGES radices");

__device__ __forceinline__ float2 c_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 c_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 c_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 c_scale(float2 a, float s) { return make_float2(a.x * s, a.y * s); }
// a * w_4: a quarter turn in the direction of the transform (dir = 1 forward: -i, dir = -1 inverse: +i)
__device__ __forceinline__ float2 c_rot(float2 a, float dir) { return make_float2(dir * a.y, -dir * a.x); }

__device__ __forceinline__ float2 dft_load(const GmDftDesc& d, long long base, int j) {
  const int kind = d.src_kind;
  if (kind == DFT_HERMITIAN) {
    const int half = d.n / 2 + 1;
    const int jj = j < half ? j : d.n - j;
    float2 v = reinterpret_cast<const float2*>(d.src)[base + (long long)jj * d.src_axis_stride];
    if (j >= half) v.y = -v.y;
    return v;
  }
  if (j >= d.n_valid) return make_float2(0.f, 0.f);
  const long long at = base + (long long)j * d.src_axis_stride;
  if (kind == DFT_COMPLEX) return reinterpret_cast<const float2*>(d.src)[at];
  if (kind == GM_F32) return make_float2(reinterpret_cast<const float*>(d.src)[at], 0.f);
  if (kind == GM_BF16) return make_float2(bf16_to_f32(reinterpret_cast<const bf16_raw*>(d.src)[at]), 0.f);
  return make_float2((float)reinterpret_cast<const _Float16*>(d.src)[at], 0.f);
}

__device__ __forceinline__ void dft_store(const GmDftDesc& d, long long base, int j, float2 v, float scale) {
  const long long at = base + (long long)j * d.dst_axis_stride;
  const int kind = d.dst_kind;
  if (kind == DFT_COMPLEX)
    reinterpret_cast<float2*>(d.dst)[at] = c_scale(v, scale);
  else if (kind == GM_F32)
    reinterpret_cast<float*>(d.dst)[at] = v.x * scale;
  else if (kind == GM_BF16)
    reinterpret_cast<bf16_raw*>(d.dst)[at] = f32_to_bf16(v.x * scale);
  else
    reinterpret_cast<_Float16*>(d.dst)[at] = (_Float16)(v.x * scale);
}

__global__ __launch_bounds__(DFT_THREADS) void dft_lines_kernel(GmDftDesc d, int L, int stride, long long lines) {
  extern __shared__ __align__(16) unsigned char dft_smem[];
  long long* lsrc = reinterpret_cast<long long*>(dft_smem);
  long long* ldst = lsrc + DFT_MAX_LINES;
  float2* buf0 = reinterpret_cast<float2*>(dft_smem + DFT_LINE_TABLE_BYTES);
  float2* buf1 = buf0 + (size_t)L * stride;
  const int tid = threadIdx.x;
  const int N = d.n;
  const float dir = d.inverse ? -1.f : 1.f;
  const float2* __restrict__ tw = reinterpret_cast<const float2*>(d.twiddle);
  const float scale = d.scale_dev ? d.scale * d.scale_dev[0] : d.scale;
  const long long tiles = (lines + L - 1) / L;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long l0 = tile * L;
    const int nl = (int)min((long long)L, lines - l0);
    __syncthreads();  // the previous tile's stores have read the line table
    for (int t = tid; t < nl; t += DFT_THREADS) {
      long long r = l0 + t, so = 0, dof = 0;
#pragma unroll
      for (int a = 3; a >= 0; --a) {
        const long long i = r % d.extent[a];
        r /= d.extent[a];
        so += i * d.src_stride[a];
        dof += i * d.dst_stride[a];
      }
      lsrc[t] = so;
      ldst[t] = dof;
    }
    __syncthreads();
    const int total = nl * N;
    if (d.src_axis_stride == 1 || nl == 1) {  // along the line
      for (int idx = tid; idx < total; idx += DFT_THREADS) {
        const int ll = idx / N, j = idx - ll * N;
        buf0[ll * stride + j] = dft_load(d, lsrc[ll], j);
      }
    } else {  // across the L neighbouring lines
      for (int idx = tid; idx < total; idx += DFT_THREADS) {
        const int j = idx / nl, ll = idx - j * nl;
        buf0[ll * stride + j] = dft_load(d, lsrc[ll], j);
      }
    }
    __syncthreads();
    float2* in = buf0;
    float2* out = buf1;
    int s = 1;
    for (int st = 0; st < d.nstages; ++st) {
      const int r = d.radix[st];
      const int nb = N / r;  // butterflies per line = m * s
      if (r == 2 || r == 3 || r == 4 || r == 5) {
        const int items = nl * nb;
        for (int w = tid; w < items; w += DFT_THREADS) {
          const int ll = w / nb, b = w - ll * nb;
          const int p = b / s, q = b - p * s;
          const float2* a = in + ll * stride + b;
          float2* o = out + ll * stride + q + s * r * p;
          const int tstep = s * p;  // w_N^(s p u) = tw[tstep * u]
          float2 y[5];
          if (r == 2) {
            const float2 a0 = a[0], a1 = a[nb];
            y[0] = c_add(a0, a1);
            y[1] = c_sub(a0, a1);
          } else if (r == 4) {
            const float2 a0 = a[0], a1 = a[nb], a2 = a[2 * nb], a3 = a[3 * nb];
            const float2 e0 = c_add(a0, a2), e1 = c_sub(a0, a2), o0 = c_add(a1, a3), o1 = c_rot(c_sub(a1, a3), dir);
            y[0] = c_add(e0, o0);
            y[1] = c_add(e1, o1);
            y[2] = c_sub(e0, o0);
            y[3] = c_sub(e1, o1);
          } else if (r == 3) {
            const float2 a0 = a[0], a1 = a[nb], a2 = a[2 * nb];
            const float2 sm = c_add(a1, a2);
            const float2 mid = c_sub(a0, c_scale(sm, 0.5f));
            const float2 df = c_rot(c_scale(c_sub(a1, a2), 0.86602540378443864676f), dir);
            y[0] = c_add(a0, sm);
            y[1] = c_add(mid, df);
            y[2] = c_sub(mid, df);
          } else {
            const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f, s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
            const float2 a0 = a[0], a1 = a[nb], a2 = a[2 * nb], a3 = a[3 * nb], a4 = a[4 * nb];
            const float2 t1 = c_add(a1, a4), t2 = c_add(a2, a3), d1 = c_sub(a1, a4), d2 = c_sub(a2, a3);
            const float2 m1 = c_add(c_add(a0, c_scale(t1, c1)), c_scale(t2, c2));
            const float2 m2 = c_add(c_add(a0, c_scale(t1, c2)), c_scale(t2, c1));
            const float2 n1 = c_rot(c_add(c_scale(d1, s1), c_scale(d2, s2)), dir);
            const float2 n2 = c_rot(c_sub(c_scale(d1, s2), c_scale(d2, s1)), dir);
            y[0] = c_add(c_add(a0, t1), t2);
            y[1] = c_add(m1, n1);
            y[2] = c_add(m2, n2);
            y[3] = c_sub(m2, n2);
            y[4] = c_sub(m1, n1);
          }
          o[0] = y[0];
#pragma unroll
          for (int u = 1; u < 5; ++u)
            if (u < r) {
              float2 t = tw[tstep * u];
              t.y *= dir;
              o[s * u] = c_mul(y[u], t);
            }
        }
      } else {  // any other prime: one output per work item, the sum in t order
        const int items = nl * N;
        for (int w = tid; w < items; w += DFT_THREADS) {
          const int ll = w / N, rem = w - ll * N;
          const int u = rem / nb, b = rem - u * nb;
          const int p = b / s, q = b - p * s;
          const float2* a = in + ll * stride + b;
          float2 acc = a[0];
          int k = 0;  // (t * u) mod r
          for (int t = 1; t < r; ++t) {
            k += u;
            if (k >= r) k -= r;
            float2 wr = tw[k * nb];
            wr.y *= dir;
            const float2 pr = c_mul(a[(long long)t * nb], wr);
            acc = c_add(acc, pr);
          }
          if (u) {
            float2 t = tw[s * p * u];
            t.y *= dir;
            acc = c_mul(acc, t);
          }
          out[ll * stride + q + s * (r * p + u)] = acc;
        }
      }
      __syncthreads();
      float2* sw = in;
      in = out;
      out = sw;
      s *= r;
    }
    const int ns = d.n_store;
    const int stotal = nl * ns;
    if (d.dst_axis_stride == 1 || nl == 1) {
      for (int idx = tid; idx < stotal; idx += DFT_THREADS) {
        const int ll = idx / ns, j = idx - ll * ns;
        dft_store(d, ldst[ll], j, in[ll * stride + j], scale);
      }
    } else {
      for (int idx = tid; idx < stotal; idx += DFT_THREADS) {
        const int j = idx / nl, ll = idx - j * nl;
        dft_store(d, ldst[ll], j, in[ll * stride + j], scale);
      }
    }
  }
}

extern "C" int gm_dft_max_length(void) { return DFT_MAX_LENGTH; }

extern "C" int gm_dft_lines(const GmDftDesc* d, void* stream) {
  GM_REQUIRE(d && d->src && d->dst && d->twiddle, "null pointer");
  GM_REQUIRE(d->n >= 1 && d->n <= DFT_MAX_LENGTH, "transform length outside 1 .. gm_dft_max_length()");
  GM_REQUIRE(d->n_valid >= 1 && d->n_valid <= d->n && d->n_store >= 1 && d->n_store <= d->n, "valid / stored point counts outside 1 .. n");
  GM_REQUIRE(d->nstages >= 0 && d->nstages <= DFT_MAX_STAGES, "too many stages");
  GM_REQUIRE(d->src_kind >= GM_F32 && d->src_kind <= DFT_HERMITIAN && d->dst_kind >= GM_F32 && d->dst_kind <= DFT_COMPLEX, "unknown element kind");
  long long prod = 1, lines = 1;
  for (int s = 0; s < d->nstages; ++s) {
    GM_REQUIRE(d->radix[s] >= 2 && d->radix[s] <= d->n, "radix outside 2 .. n");
    prod *= d->radix[s];
  }
  GM_REQUIRE(prod == d->n, "the radices do not multiply to the transform length");
  for (int a = 0; a < 4; ++a) {
    GM_REQUIRE(d->extent[a] >= 1, "empty line grid");
    lines *= d->extent[a];
  }
  const int stride = d->n | 1;
  int L = 1;
  while (L < DFT_MAX_LINES && (long long)(2 * L) * stride <= DFT_TILE_POINTS && L < lines) L *= 2;
  const size_t lds = DFT_LINE_TABLE_BYTES + (size_t)2 * L * stride * sizeof(float2);
  GM_REQUIRE(lds <= DFT_LDS_BYTES, "line buffers exceed the LDS");
  static bool configured = false;
  if (!configured) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dft_lines_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, DFT_LDS_BYTES);
    if (e != hipSuccess) GM_FAIL((int)e, hipGetErrorString(e));
    configured = true;
  }
  const long long tiles = (lines + L - 1) / L;
  const int grid = (int)(tiles < 256 * 16 ? tiles : 256 * 16);
  dft_lines_kernel<<<grid, DFT_THREADS, lds, (hipStream_t)stream>>>(*d, L, stride, lines);
  GM_LAUNCH_CHECK();
}

// ---- the loss over two half spectra ---------------------------------------------------------------------------------------------------------------
// x, y: (rows, half) complex, rows = batch * m0 * m1 * m2 (the leading transformed axes, missing ones 1), half = n_last / 2 + 1.  Bin (k, kl) of the half
// spectrum stands for itself and, unless kl is 0 or n_last / 2 (even n_last), for its mirror (-k, n_last - kl) of the full spectrum.
#define SL_THREADS 256
#define SL_MAX_PARTS 1024

static int spectral_parts(long long bins) {
  long long g = (bins + SL_THREADS - 1) / SL_THREADS;
  if (g > SL_MAX_PARTS) g = SL_MAX_PARTS;
  if (g < 1) g = 1;
  return (int)g;
}

__global__ __launch_bounds__(SL_THREADS) void spectral_loss_kernel(const float2* x, const float2* y, long long rows, int m0, int m1, int m2, int N,
                                                                  const float* __restrict__ up, float2* hx, float2* hy, float* __restrict__ full,
                                                                  double* __restrict__ partials) {
  const int half = N / 2 + 1;
  const long long total = rows * half;
  const bool mirror = up != nullptr || full != nullptr;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * SL_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * SL_THREADS) {
    const long long r = i / half;
    const int kl = (int)(i - r * half);
    const bool self = kl == 0 || 2 * kl == N;
    long long rm = r;
    if (mirror) {
      long long t = r;
      const int k2 = (int)(t % m2); t /= m2;
      const int k1 = (int)(t % m1); t /= m1;
      const int k0 = (int)(t % m0);
      const long long b = t / m0;
      rm = ((b * m0 + (k0 ? m0 - k0 : 0)) * m1 + (k1 ? m1 - k1 : 0)) * m2 + (k2 ? m2 - k2 : 0);
    }
    // the full map takes both members of a self-mirrored pair from ONE of them (the lower row): they are equal bit for bit
    const long long at = (full != nullptr && self) ? (r < rm ? r : rm) * half + kl : i;
    const float2 xv = x[at], yv = y[at];
    const float ax = sqrtf(xv.x * xv.x + xv.y * xv.y), ay = sqrtf(yv.x * yv.x + yv.y * yv.y);
    const float df = ax - ay;
    const float v = df * df;
    acc += (self ? 1.0 : 2.0) * (double)v;
    if (full != nullptr) {
      full[r * N + kl] = v;
      if (!self) full[rm * N + (N - kl)] = v;
    }
    if (hx != nullptr || hy != nullptr) {
      const float ub = up != nullptr ? 0.5f * (up[r * N + kl] + up[rm * N + (kl ? N - kl : 0)]) : 1.f;
      const float g = 2.f * ub * df;
      if (hx != nullptr) {
        const float c = ax > 0.f ? g / ax : 0.f;  // a bin of amplitude zero contributes nothing (the reference's sqrt has no gradient there)
        hx[i] = make_float2(xv.x * c, xv.y * c);
      }
      if (hy != nullptr) {
        const float c = ay > 0.f ? -g / ay : 0.f;
        hy[i] = make_float2(yv.x * c, yv.y * c);
      }
    }
  }
  if (partials != nullptr) {
    __shared__ double part[SL_THREADS / 64];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
  }
}

// out[0] = (the partials added in a fixed order) * out_scale: thread t adds partials t, t + 256, ... in index order, then a fixed tree
__global__ __launch_bounds__(SL_THREADS) void spectral_fold_kernel(const double* __restrict__ partials, int parts, double out_scale, float* __restrict__ out) {
  __shared__ double red[SL_THREADS];
  double a = 0.0;
  for (int j = threadIdx.x; j < parts; j += SL_THREADS) a += partials[j];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = SL_THREADS / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(red[0] * out_scale);
}

extern "C" int gm_spectral_loss_partials(long long bins) { return spectral_parts(bins); }

extern "C" int gm_spectral_loss(const float* x, const float* y, long long batch, int m0, int m1, int m2, int n_last, const float* upstream, float* hx,
                                float* hy, float* full, double* partials, float* out, double out_scale, void* stream) {
  GM_REQUIRE(x && y, "null pointer");
  GM_REQUIRE(batch >= 1 && m0 >= 1 && m1 >= 1 && m2 >= 1 && n_last >= 1, "empty spectrum");
  GM_REQUIRE((out != nullptr) == (partials != nullptr), "the reduced value needs the partials workspace, and only it");
  GM_REQUIRE(out || full || hx || hy, "nothing asked for");
  GM_REQUIRE(!(full && (hx || hy)), "the full map and the gradient spectra are separate launches");
  GM_REQUIRE(!upstream || hx || hy, "an upstream map without a gradient spectrum");
  const long long rows = batch * m0 * m1 * m2;
  const long long bins = rows * (n_last / 2 + 1);
  const int grid = spectral_parts(bins);
  hipStream_t st = (hipStream_t)stream;
  spectral_loss_kernel<<<grid, SL_THREADS, 0, st>>>(reinterpret_cast<const float2*>(x), reinterpret_cast<const float2*>(y), rows, m0, m1, m2, n_last, upstream,
                                                    reinterpret_cast<float2*>(hx), reinterpret_cast<float2*>(hy), full, partials);
  if (out) spectral_fold_kernel<<<1, SL_THREADS, 0, st>>>(partials, grid, out_scale, out);
  GM_LAUNCH_CHECK();
}
