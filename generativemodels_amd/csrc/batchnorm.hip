// BatchNorm (+ LeakyReLU) forward and backward over arena tensors [rows][C] with a row pitch (nn.BatchNorm{2,3}d + nn.LeakyReLU / nn.ReLU: the
// normalised layers of the PatchGAN discriminators, networks/nets/patchgan_discriminator.py).
//
// Every table is per CHANNEL -- [C], not [N][C] as in the GroupNorm kernels -- so the samples of a batch are one flat range of rows = N * V rows and a
// lane keeps the coefficients of its channel vector in registers for the whole launch.
//   gm_bn_finalize      [S][N][C][2] fp64 (sum, sum of squares) partials (ops.channel_stats / a convolution epilogue) -> scale, shift, mean, invstd and the
//                       running buffers (training), or scale / shift from the running buffers (eval).  One wave per channel.
//   gm_bn_apply         y = act(x * scale[c] + shift[c]), act none or LeakyReLU(slope >= 0); y rounded once.
//   gm_bn_bwd_stats     per row block and channel {sum g, sum g * xhat}, g = gy * act'(x * scale + shift): one plain fp64 store per partial.
//   gm_bn_bwd_finalize  the fold of those partials -> dgamma, dbeta and the two coefficient tables of the apply pass.
//   gm_bn_bwd_apply     dx = g * scale + (x - mean) * cb + cc.
// No atomics: every sum is a fold in a fixed order (lane-strided slots, then an xor-shuffle tree; or rows in row order, then an LDS column), so a
// training step is bitwise repeatable.  fp32 arithmetic per element, fp64 wherever values are added up.  The three streaming kernels are HBM-bound:
// lane <-> one 16-byte channel vector (a scalar form where C, a pitch or a base address does not allow it -- C = 1 and C = 3 are real cases),
// 256 / CV rows in flight per work-group, four rows requested per wait, as in gn_apply_rows_kernel / gn_bwd_apply_kernel.
#include "gm_common.h"

#define BN_ACT_NONE 0
#define BN_ACT_LEAKY 1

// the pre-activation exactly as the forward formed it: one fused multiply-add, so that the backward's sign test sees the forward's value
__device__ __forceinline__ float bn_pre(float x, float sc, float sh) { return __builtin_fmaf(x, sc, sh); }

// ---- finalisation: one wave per channel, lane l folds entries l, l + 64, ... of the S * N partials of its channel, then the xor-shuffle tree -------------
__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ stats, int entries, int C, double count, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, float momentum, int training,
                                                         float* __restrict__ running_mean, float* __restrict__ running_var, float* __restrict__ scale,
                                                         float* __restrict__ shift, float* __restrict__ mean_out, float* __restrict__ invstd_out) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;  // (whole waves leave; no barrier below)
  double mean, var;
  if (training) {
    double a = 0.0, b = 0.0;
    for (int e = lane; e < entries; e += 64) {
      const double2 v = *reinterpret_cast<const double2*>(stats + ((long long)e * C + c) * 2);
      a += v.x; b += v.y;
    }
    a = wave_sum(a); b = wave_sum(b);
    mean = a / count;
    var = b / count - mean * mean;
    if (var < 0.0) var = 0.0;
  } else {
    mean = (double)running_mean[c];
    var = (double)running_var[c];
  }
  if (lane != 0) return;
  const double istd = 1.0 / sqrt(var + (double)eps);
  const double sc = (gamma ? (double)gamma[c] : 1.0) * istd;
  scale[c] = (float)sc;
  shift[c] = (float)((beta ? (double)beta[c] : 0.0) - mean * sc);
  if (mean_out) mean_out[c] = (float)mean;
  if (invstd_out) invstd_out[c] = (float)istd;
  if (training && running_mean) {
    const double m = (double)momentum;
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
    running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * unbiased);
  }
}

extern "C" int gm_bn_finalize(const double* stats, int S, int N, int C, long long V, const float* gamma, const float* beta, float eps, float momentum,
                              int training, float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* invstd,
                              void* stream) {
  GM_REQUIRE(scale && shift, "null pointer");
  GM_REQUIRE(S >= 0 && N >= 0 && C >= 0 && V >= 0, "negative extent");
  GM_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "the running buffers come as a pair");
  if (training) {
    GM_REQUIRE(stats, "training needs the statistic partials");
    GM_REQUIRE((long long)S * N <= 0x7fffffffll, "statistic table too long");
  } else {
    GM_REQUIRE(running_mean, "eval needs the running buffers");
  }
  if (C == 0) return 0;
  if (training) GM_REQUIRE(S > 0 && (long long)N * V > 0, "training over an empty batch");
  bn_finalize_kernel<<<(unsigned)((C + 3) / 4), 256, 0, (hipStream_t)stream>>>(stats, S * N, C, (double)N * (double)V, gamma, beta, eps, momentum, training,
                                                                                 running_mean, running_var, scale, shift, mean, invstd);
  GM_LAUNCH_CHECK();
}

// ---- the launch geometry of the three streaming kernels -------------------------------------------------------------------------------------------------
// CV channel vectors per row (host: CV <= 256), R = 256 / CV rows in flight per work-group; a work-group walks rows_per_block consecutive rows.
struct BnGeom { bool vec_ok; int CV, R; long long nblk; int rpb; };

static bool bn_geometry(long long rows, int C, int vec, bool vec_ok, long long max_blocks, int min_iters, BnGeom& g) {
  g.vec_ok = vec_ok;
  g.CV = vec_ok ? C / vec : C;
  if (g.CV < 1 || g.CV > 256) return false;
  g.R = 256 / g.CV;
  long long iters = (rows + (long long)g.R * max_blocks - 1) / ((long long)g.R * max_blocks);  // rows per lane
  iters = (iters + 3) / 4 * 4;
  if (iters < min_iters) iters = min_iters;
  const long long rpb = (long long)g.R * iters;
  if (rpb > 0x7fffffffll) return false;
  g.rpb = (int)rpb;
  g.nblk = (rows + rpb - 1) / rpb;
  return g.nblk >= 1 && g.nblk <= 0x7fffffffll;
}

template <typename T, int VEC> __device__ __forceinline__ void bn_load_table(const float* __restrict__ tab, int c0, float* o) {
#pragma unroll
  for (int k = 0; k < VEC; ++k) o[k] = tab[c0 + k];
}

// ---- forward apply -------------------------------------------------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, long long x_ld, T* __restrict__ y, long long y_ld,
                                                      const float* __restrict__ scale, const float* __restrict__ shift, long long rows, int C,
                                                      int rows_per_block, int act, float slope) {
  const int CV = C / VEC, R = 256 / CV;
  const int t = threadIdx.x;
  const int cv = t % CV, r0 = t / CV;
  if (r0 >= R) return;
  const long long row_begin = (long long)blockIdx.x * rows_per_block;
  long long row_end = row_begin + rows_per_block;
  if (row_end > rows) row_end = rows;
  float sc[VEC], sh[VEC];
  bn_load_table<T, VEC>(scale, cv * VEC, sc);
  bn_load_table<T, VEC>(shift, cv * VEC, sh);
  const T* xb = x + (long long)cv * VEC;
  T* yb = y + (long long)cv * VEC;
  constexpr int UB = 4;  // rows requested per wait (clamped addresses, masked stores)
  for (long long r = row_begin + r0; r < row_end; r += (long long)UB * R) {
    float v[UB][VEC];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const long long rr = r + (long long)u * R < row_end ? r + (long long)u * R : r;
      VecIO<T, VEC>::ld(xb + rr * x_ld, v[u]);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[u][k] = bn_pre(v[u][k], sc[k], sh[k]);
      if (act == BN_ACT_LEAKY) {  // (tested once per vector: see gn_apply_vec_kernel)
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[u][k] = v[u][k] > 0.f ? v[u][k] : v[u][k] * slope;
      }
      const long long rr = r + (long long)u * R;
      if (rr < row_end) VecIO<T, VEC>::st(yb + rr * y_ld, v[u]);
    }
  }
}

extern "C" int gm_bn_apply(const void* x, long long x_ld, void* y, long long y_ld, const float* scale, const float* shift, long long rows, int C, int act,
                           float slope, int dtype, void* stream) {
  GM_REQUIRE(x && y && scale && shift, "null pointer");
  GM_REQUIRE(rows >= 0 && C >= 0, "negative extent");
  GM_REQUIRE(x_ld >= C && y_ld >= C, "pitch below C");
  GM_REQUIRE(act == BN_ACT_NONE || (act == BN_ACT_LEAKY && slope >= 0.f), "activation: none, or leakyrelu with a slope >= 0");
  if (rows == 0 || C == 0) return 0;
  const int vec = dtype == GM_F32 ? 4 : 8;
  const bool vec_ok = (C % vec == 0) && (x_ld % vec == 0) && (y_ld % vec == 0) && gm_aligned16(x) && gm_aligned16(y);
  hipStream_t st = (hipStream_t)stream;
  BnGeom g{};
  bool launched = true;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        if (!(launched = bn_geometry(rows, C, vec, vec_ok, 2048, 4, g))) return;
        bn_apply_kernel<T, decltype(tv)::vec><<<(unsigned)g.nblk, 256, 0, st>>>((const T*)x, x_ld, (T*)y, y_ld, scale, shift, rows, C, g.rpb, act, slope);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_REQUIRE(launched, "too many channels or rows for gm_bn_apply");
  GM_LAUNCH_CHECK();
}

// ---- backward statistics: out[blk][c] = {sum g, sum g * xhat} over the rows of block blk --------------------------------------------------------------------
// fp32 partial sums per lane over its rows (in row order), an fp64 LDS column over the R rows in flight, one double2 store per (block, channel).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bn_bwd_stats_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ gy, long long gy_ld,
                                                          const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                                          const float* __restrict__ invstd, long long rows, int C, int rows_per_block, int act, float slope,
                                                          double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int CV = C / VEC, R = 256 / CV;
  float* part_a = reinterpret_cast<float*>(smem_raw);  // [R][C]
  float* part_b = part_a + (size_t)R * C;
  const int t = threadIdx.x;
  const int cv = t % CV, r0 = t / CV;
  const long long row_begin = (long long)blockIdx.x * rows_per_block;
  long long row_end = row_begin + rows_per_block;
  if (row_end > rows) row_end = rows;
  if (r0 < R) {
    float sc[VEC], sh[VEC], mu[VEC], a[VEC], b[VEC];
    bn_load_table<T, VEC>(scale, cv * VEC, sc);
    bn_load_table<T, VEC>(shift, cv * VEC, sh);
    bn_load_table<T, VEC>(mean, cv * VEC, mu);
#pragma unroll
    for (int k = 0; k < VEC; ++k) { a[k] = 0.f; b[k] = 0.f; }
    const T* xb = x + (long long)cv * VEC;
    const T* gb = gy + (long long)cv * VEC;
    constexpr int UB = 4;
    for (long long r = row_begin + r0; r < row_end; r += (long long)UB * R) {
      float xv[UB][VEC], gv[UB][VEC];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const long long rr = r + (long long)u * R < row_end ? r + (long long)u * R : r;
        VecIO<T, VEC>::ld(xb + rr * x_ld, xv[u]);
        VecIO<T, VEC>::ld(gb + rr * gy_ld, gv[u]);
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const bool ok = r + (long long)u * R < row_end;
        if (act == BN_ACT_LEAKY) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) gv[u][k] = bn_pre(xv[u][k], sc[k], sh[k]) > 0.f ? gv[u][k] : gv[u][k] * slope;
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) { a[k] += ok ? gv[u][k] : 0.f; b[k] += ok ? gv[u][k] * (xv[u][k] - mu[k]) : 0.f; }
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      part_a[(size_t)r0 * C + cv * VEC + k] = a[k];
      part_b[(size_t)r0 * C + cv * VEC + k] = b[k];
    }
  }
  __syncthreads();
  for (int c = t; c < C; c += 256) {
    double da = 0.0, db = 0.0;
    for (int r = 0; r < R; ++r) { da += (double)part_a[(size_t)r * C + c]; db += (double)part_b[(size_t)r * C + c]; }
    *reinterpret_cast<double2*>(out + ((long long)blockIdx.x * C + c) * 2) = make_double2(da, db * (double)invstd[c]);
  }
}

// the partial rows of gm_bn_bwd_stats depend on the row count alone (>= 256 rows per work-group, at most 1024 partial rows), as in gm_gn_bwd_stats
static void bn_bwd_stats_rows(long long rows, long long& nblk, long long& rpb) {
  nblk = (rows + 255) / 256;
  if (nblk > 1024) nblk = 1024;
  if (nblk < 1) nblk = 1;
  rpb = (rows + nblk - 1) / nblk;
  if (rpb < 1) rpb = 1;
  nblk = (rows + rpb - 1) / rpb;
  if (nblk < 1) nblk = 1;
}

extern "C" long long gm_bn_bwd_stats_slots(long long rows) {
  if (rows <= 0) return 0;
  long long nblk, rpb;
  bn_bwd_stats_rows(rows, nblk, rpb);
  return nblk;
}

extern "C" int gm_bn_bwd_stats(const void* x, long long x_ld, const void* gy, long long gy_ld, const float* scale, const float* shift, const float* mean,
                               const float* invstd, long long rows, int C, int act, float slope, double* out, int dtype, void* stream) {
  GM_REQUIRE(x && gy && scale && shift && mean && invstd && out, "null pointer");
  GM_REQUIRE(rows >= 0 && C >= 0, "negative extent");
  GM_REQUIRE(x_ld >= C && gy_ld >= C, "pitch below C");
  GM_REQUIRE(act == BN_ACT_NONE || (act == BN_ACT_LEAKY && slope >= 0.f), "activation: none, or leakyrelu with a slope >= 0");
  if (rows == 0 || C == 0) return 0;
  const int vec = dtype == GM_F32 ? 4 : 8;
  const bool vec_ok = (C % vec == 0) && (x_ld % vec == 0) && (gy_ld % vec == 0) && gm_aligned16(x) && gm_aligned16(gy);
  hipStream_t st = (hipStream_t)stream;
  BnGeom g{};
  bool launched = true;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        long long nblk, rpb;
        bn_bwd_stats_rows(rows, nblk, rpb);
        g.CV = vec_ok ? C / vec : C;
        if (!(launched = g.CV <= 256 && rpb <= 0x7fffffffll)) return;
        g.R = 256 / g.CV; g.nblk = nblk; g.rpb = (int)rpb;
        const size_t smem = (size_t)g.R * C * 2 * sizeof(float);  // [R][C] partial sums of g and of g * (x - mean): at most 16 KiB
        bn_bwd_stats_kernel<T, decltype(tv)::vec><<<(unsigned)g.nblk, 256, smem, st>>>((const T*)x, x_ld, (const T*)gy, gy_ld, scale, shift, mean, invstd, rows,
                                                                                      C, g.rpb, act, slope, out);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_REQUIRE(launched, "too many channels or rows for gm_bn_bwd_stats");
  GM_LAUNCH_CHECK();
}

// ---- the fold of the backward partials: one wave per channel ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ partials, int slots, int C, double count,
                                                             const float* __restrict__ scale, const float* __restrict__ invstd, int training,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ cb,
                                                             float* __restrict__ cc) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  double sg = 0.0, sgx = 0.0;
  for (int s = lane; s < slots; s += 64) {
    const double2 v = *reinterpret_cast<const double2*>(partials + ((long long)s * C + c) * 2);
    sg += v.x; sgx += v.y;
  }
  sg = wave_sum(sg); sgx = wave_sum(sgx);
  if (lane != 0) return;
  if (dgamma) dgamma[c] = (float)sgx;
  if (dbeta) dbeta[c] = (float)sg;
  if (training) {  // dx = scale * (g - mean(g) - xhat * mean(g * xhat)),  xhat = (x - mean) * invstd
    const double sc = (double)scale[c];
    cb[c] = (float)(-sc * (double)invstd[c] * (sgx / count));
    cc[c] = (float)(-sc * (sg / count));
  } else {         // the statistics are constants: dx = g * scale
    cb[c] = 0.f;
    cc[c] = 0.f;
  }
}

extern "C" int gm_bn_bwd_finalize(const double* partials, int slots, int C, long long rows, const float* scale, const float* invstd, int training,
                                  float* dgamma, float* dbeta, float* cb, float* cc, void* stream) {
  GM_REQUIRE(partials && scale && invstd && cb && cc, "null pointer");
  GM_REQUIRE(slots > 0 && C >= 0 && rows > 0, "empty problem");
  if (C == 0) return 0;
  bn_bwd_finalize_kernel<<<(unsigned)((C + 3) / 4), 256, 0, (hipStream_t)stream>>>(partials, slots, C, (double)rows, scale, invstd, training, dgamma, dbeta,
                                                                                     cb, cc);
  GM_LAUNCH_CHECK();
}

// ---- backward apply: dx = g * scale + (x - mean) * cb + cc --------------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ x, long long x_ld, const T* __restrict__ gy, long long gy_ld, T* __restrict__ dx,
                                                          long long dx_ld, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const float* __restrict__ mean, const float* __restrict__ cb, const float* __restrict__ cc,
                                                          long long rows, int C, int rows_per_block, int act, float slope) {
  const int CV = C / VEC, R = 256 / CV;
  const int t = threadIdx.x;
  const int cv = t % CV, r0 = t / CV;
  if (r0 >= R) return;
  const long long row_begin = (long long)blockIdx.x * rows_per_block;
  long long row_end = row_begin + rows_per_block;
  if (row_end > rows) row_end = rows;
  float sc[VEC], sh[VEC], mu[VEC], kb[VEC], kc[VEC];
  bn_load_table<T, VEC>(scale, cv * VEC, sc);
  bn_load_table<T, VEC>(shift, cv * VEC, sh);
  bn_load_table<T, VEC>(mean, cv * VEC, mu);
  bn_load_table<T, VEC>(cb, cv * VEC, kb);
  bn_load_table<T, VEC>(cc, cv * VEC, kc);
  const T* xb = x + (long long)cv * VEC;
  const T* gb = gy + (long long)cv * VEC;
  T* db = dx + (long long)cv * VEC;
  constexpr int UB = 4;
  for (long long r = row_begin + r0; r < row_end; r += (long long)UB * R) {
    float xv[UB][VEC], gv[UB][VEC];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const long long rr = r + (long long)u * R < row_end ? r + (long long)u * R : r;
      VecIO<T, VEC>::ld(xb + rr * x_ld, xv[u]);
      VecIO<T, VEC>::ld(gb + rr * gy_ld, gv[u]);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      float o[VEC];
      if (act == BN_ACT_LEAKY) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) gv[u][k] = bn_pre(xv[u][k], sc[k], sh[k]) > 0.f ? gv[u][k] : gv[u][k] * slope;
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) o[k] = gv[u][k] * sc[k] + ((xv[u][k] - mu[k]) * kb[k] + kc[k]);
      const long long rr = r + (long long)u * R;
      if (rr < row_end) VecIO<T, VEC>::st(db + rr * dx_ld, o);
    }
  }
}

extern "C" int gm_bn_bwd_apply(const void* x, long long x_ld, const void* gy, long long gy_ld, void* dx, long long dx_ld, const float* scale,
                               const float* shift, const float* mean, const float* cb, const float* cc, long long rows, int C, int act, float slope,
                               int dtype, void* stream) {
  GM_REQUIRE(x && gy && dx && scale && shift && mean && cb && cc, "null pointer");
  GM_REQUIRE(rows >= 0 && C >= 0, "negative extent");
  GM_REQUIRE(x_ld >= C && gy_ld >= C && dx_ld >= C, "pitch below C");
  GM_REQUIRE(act == BN_ACT_NONE || (act == BN_ACT_LEAKY && slope >= 0.f), "activation: none, or leakyrelu with a slope >= 0");
  if (rows == 0 || C == 0) return 0;
  const int vec = dtype == GM_F32 ? 4 : 8;
  const bool vec_ok = (C % vec == 0) && (x_ld % vec == 0) && (gy_ld % vec == 0) && (dx_ld % vec == 0) && gm_aligned16(x) && gm_aligned16(gy) && gm_aligned16(dx);
  hipStream_t st = (hipStream_t)stream;
  BnGeom g{};
  bool launched = true;
  if (!gm_dispatch_vec(dtype, vec_ok, [&](auto tv) {
        using T = typename decltype(tv)::type;
        if (!(launched = bn_geometry(rows, C, vec, vec_ok, 4096, 8, g))) return;
        bn_bwd_apply_kernel<T, decltype(tv)::vec><<<(unsigned)g.nblk, 256, 0, st>>>((const T*)x, x_ld, (const T*)gy, gy_ld, (T*)dx, dx_ld, scale, shift, mean, cb,
                                                                                   cc, rows, C, g.rpb, act, slope);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_REQUIRE(launched, "too many channels or rows for gm_bn_bwd_apply");
  GM_LAUNCH_CHECK();
}
