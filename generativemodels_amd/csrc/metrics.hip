// generative.metrics on gfx950: SSIM / contrast sensitivity, the 2x pooling between MS-SSIM scales, and the MMD terms.
//   gm_ssim_cs          fused separable SSIM + cs: per batch item means, optional full maps   (reference: metrics/ssim.py:169-231)
//   gm_avgpool2_pair    avg_pool{2,3}d(kernel_size=2) of both images in one launch            (reference: metrics/ms_ssim.py:140-141)
//   gm_mmd              the three Gram-matrix means of MMDMetric from column sums             (reference: metrics/mmd.py:68-80)
// Every reduction is per work-group partials + a fold in a fixed order: no atomics, results are bit-reproducible.
#include "gm_common.h"

#include "ssim_common.h"  // the plan (SsimGeom, SsimTaps, ssim_geom, ssim_lds_floats, ssim_check_geom), shared with metrics_bwd.hip

// ssim.py:224-229 in its own order, every operation rounded (no contraction)
__device__ __forceinline__ void ssim_point(float mx, float my, float mxx, float myy, float mxy, float c1, float c2, float& ssim, float& cs) {
#pragma clang fp contract(off)
  const float sigma_x = mxx - mx * mx;
  const float sigma_y = myy - my * my;
  const float sigma_xy = mxy - mx * my;
  cs = (2.0f * sigma_xy + c2) / (sigma_x + sigma_y + c2);
  ssim = ((2.0f * mx * my + c1) / (mx * mx + my * my + c1)) * cs;
}

// A work-group owns a 16 x 16 (H, W) output tile of one volume and marches along D over `dc` output planes.  Per input plane: the (16 + kh - 1) x (16 + kw - 1)
// halo of both images goes to LDS once; the W pass forms x, y, x^2, y^2, xy and filters them along W; the H pass filters along H into one slot of a ring of
// kd planes; once kd planes are in the ring the D pass filters across it and evaluates the point expression.  LDS per work-group: halo + W-filtered rows +
// kd * 5 KiB of ring (69 KiB at 11^3, 100 KiB at 16^3).
template <typename T>
__global__ __launch_bounds__(256) void ssim_cs_kernel(const T* __restrict__ x, const T* __restrict__ y, float* __restrict__ ssim_map,
                                                     float* __restrict__ cs_map, double2* __restrict__ partials, SsimGeom g, float c1, float c2,
                                                     SsimTaps taps) {
  extern __shared__ __align__(16) float lds[];
  const int RH = SSIM_TH + g.kh - 1, RW = SSIM_TW + g.kw - 1;
  float* rawx = lds;
  float* rawy = rawx + RH * RW;
  float* wf = rawy + RH * RW;             // [5][RH][16]
  float* ring = wf + 5 * RH * SSIM_TW;    // [kd][5][256]
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % g.tiles, chunk = blockIdx.x / g.tiles;
  const long long vol = blockIdx.y;
  const int th0 = (tile / g.tiles_w) * SSIM_TH, tw0 = (tile % g.tiles_w) * SSIM_TW;
  const int od0 = chunk * g.dc;
  const int od1 = min(g.Do, od0 + g.dc);
  const int ty = tid >> 4, tx = tid & 15;
  const bool valid = th0 + ty < g.Ho && tw0 + tx < g.Wo;
  const long long plane = (long long)g.H * g.W;
  const T* xv = x + vol * g.D * plane;
  const T* yv = y + vol * g.D * plane;
  const long long out_base = vol * g.Do * g.Ho * g.Wo + (long long)(th0 + ty) * g.Wo + (tw0 + tx);
  double acc_s = 0.0, acc_c = 0.0;
  int slot = 0;  // ring slot of input plane dz: (dz - od0) % kd
  for (int dz = od0; dz < od1 + g.kd - 1; ++dz) {
    // halo of both images: 32 lanes across a row (RW <= 31), 8 rows per pass; outside the volume reads as 0 (it only feeds outputs that are not kept)
    {
      const int c = tid & 31;
      const int gw = tw0 + c;
      for (int r = tid >> 5; r < RH; r += 8) {
        const int gh = th0 + r;
        if (c < RW) {
          float a = 0.0f, b = 0.0f;
          if (gh < g.H && gw < g.W) {
            const long long o = (long long)dz * plane + (long long)gh * g.W + gw;
            a = ElemIO<T>::ld(xv + o);
            b = ElemIO<T>::ld(yv + o);
          }
          rawx[r * RW + c] = a;
          rawy[r * RW + c] = b;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < RH * SSIM_TW; i += 256) {  // W pass
      const int r = i >> 4, c = i & 15;
      const float* px = rawx + r * RW + c;
      const float* py = rawy + r * RW + c;
      float sx = 0.0f, sy = 0.0f, sxx = 0.0f, syy = 0.0f, sxy = 0.0f;
      for (int j = 0; j < g.kw; ++j) {
        const float t = taps.w[j], a = px[j], b = py[j];
        sx += t * a;
        sy += t * b;
        sxx += t * (a * a);
        syy += t * (b * b);
        sxy += t * (a * b);
      }
      wf[0 * RH * SSIM_TW + i] = sx;
      wf[1 * RH * SSIM_TW + i] = sy;
      wf[2 * RH * SSIM_TW + i] = sxx;
      wf[3 * RH * SSIM_TW + i] = syy;
      wf[4 * RH * SSIM_TW + i] = sxy;
    }
    __syncthreads();
    {  // H pass -> ring[slot]
      float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      for (int j = 0; j < g.kh; ++j) {
        const float t = taps.h[j];
        const float* p = wf + (ty + j) * SSIM_TW + tx;
#pragma unroll
        for (int f = 0; f < 5; ++f) s[f] += t * p[f * RH * SSIM_TW];
      }
      float* q = ring + slot * 5 * 256 + tid;
#pragma unroll
      for (int f = 0; f < 5; ++f) q[f * 256] = s[f];
    }
    __syncthreads();
    if (dz - od0 >= g.kd - 1) {  // D pass: output plane od = dz - (kd - 1); tap j meets input plane od + j, which sits in slot (slot + 1 + j) % kd
      float s[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      int sl = slot + 1 == g.kd ? 0 : slot + 1;
      for (int j = 0; j < g.kd; ++j) {
        const float t = taps.d[j];
        const float* p = ring + sl * 5 * 256 + tid;
#pragma unroll
        for (int f = 0; f < 5; ++f) s[f] += t * p[f * 256];
        sl = sl + 1 == g.kd ? 0 : sl + 1;
      }
      if (valid) {
        float sv, cv;
        ssim_point(s[0], s[1], s[2], s[3], s[4], c1, c2, sv, cv);
        acc_s += (double)sv;
        acc_c += (double)cv;
        if (ssim_map) {
          const long long o = out_base + (long long)(dz - (g.kd - 1)) * g.Ho * g.Wo;
          ssim_map[o] = sv;
          cs_map[o] = cv;
        }
      }
    }
    slot = slot + 1 == g.kd ? 0 : slot + 1;
    // the next plane's halo and W pass touch rawx / rawy / wf only, all last read before the barrier above; its H pass overwrites the ring's oldest slot after two more barriers
  }
  // the four waves' sums meet in the halo buffer (idle now; all of the kernel's LDS is the dynamic allocation, which may then be the full 160 KiB)
  double* part = reinterpret_cast<double*>(lds);  // [2][4]
  acc_s = wave_sum(acc_s);
  acc_c = wave_sum(acc_c);
  if ((tid & 63) == 0) {
    part[tid >> 6] = acc_s;
    part[4 + (tid >> 6)] = acc_c;
  }
  __syncthreads();
  if (tid == 0) partials[vol * gridDim.x + blockIdx.x] = make_double2(part[0] + part[1] + part[2] + part[3], part[4] + part[5] + part[6] + part[7]);
}

// out[b] = (sum of batch item b's partials, in a fixed order) / count: thread t adds partials t, t + 256, ... in index order, then a fixed tree
__global__ __launch_bounds__(256) void ssim_fold_kernel(const double2* __restrict__ partials, long long per_item, double count,
                                                       float* __restrict__ ssim_mean, float* __restrict__ cs_mean) {
  __shared__ double2 sh[256];
  const double2* p = partials + (long long)blockIdx.x * per_item;
  double a = 0.0, b = 0.0;
  for (long long i = threadIdx.x; i < per_item; i += 256) {
    a += p[i].x;
    b += p[i].y;
  }
  sh[threadIdx.x] = make_double2(a, b);
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sh[threadIdx.x].x += sh[threadIdx.x + o].x;
      sh[threadIdx.x].y += sh[threadIdx.x + o].y;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    ssim_mean[blockIdx.x] = (float)(sh[0].x / count);
    cs_mean[blockIdx.x] = (float)(sh[0].y / count);
  }
}

extern "C" int gm_ssim_max_window(void) { return SSIM_MAX_WINDOW; }

// bytes of gm_ssim_cs's workspace: one (ssim, cs) fp64 pair per work-group; needs no initialisation.  < 0: bad geometry (gm_last_error)
extern "C" long long gm_ssim_workspace_bytes(long long B, long long C, int D, int H, int W, int kd, int kh, int kw) {
  if (ssim_check_geom(B, C, D, H, W, kd, kh, kw) != 0) return -1;
  const SsimGeom g = ssim_geom(D, H, W, kd, kh, kw);
  return B * C * (long long)g.chunks * g.tiles * (long long)sizeof(double2);
}

template <typename T>
static int ssim_launch(const void* x, const void* y, long long B, long long C, const SsimGeom& g, float c1, float c2, const SsimTaps& taps, float* ssim_mean,
                       float* cs_mean, float* ssim_map, float* cs_map, void* workspace, hipStream_t st) {
  static bool attr_done = false;  // (per instantiation)
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ssim_cs_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) GM_FAIL((int)e, hipGetErrorString(e));
    attr_done = true;
  }
  const long long per_vol = (long long)g.chunks * g.tiles;
  GM_REQUIRE(per_vol <= 0x7fffffffLL, "too many work-groups per volume");
  dim3 grid((unsigned)per_vol, (unsigned)(B * C));
  ssim_cs_kernel<T><<<grid, 256, (size_t)ssim_lds_floats(g) * sizeof(float), st>>>((const T*)x, (const T*)y, ssim_map, cs_map, (double2*)workspace, g, c1, c2, taps);
  const double count = (double)C * g.Do * g.Ho * g.Wo;
  ssim_fold_kernel<<<(unsigned)B, 256, 0, st>>>((const double2*)workspace, C * per_vol, count, ssim_mean, cs_mean);
  GM_LAUNCH_CHECK();
}

extern "C" int gm_ssim_cs(const void* x, const void* y, int dtype, long long B, long long C, int D, int H, int W, const float* taps_d, int kd,
                          const float* taps_h, int kh, const float* taps_w, int kw, float c1, float c2, float* ssim_mean, float* cs_mean,
                          float* ssim_map, float* cs_map, void* workspace, long long workspace_bytes, void* stream) {
  GM_REQUIRE(x && y && taps_d && taps_h && taps_w && ssim_mean && cs_mean && workspace, "null pointer");
  GM_REQUIRE((ssim_map == nullptr) == (cs_map == nullptr), "the two maps come together");
  if (ssim_check_geom(B, C, D, H, W, kd, kh, kw) != 0) return -1;
  const SsimGeom g = ssim_geom(D, H, W, kd, kh, kw);
  GM_REQUIRE(workspace_bytes >= B * C * (long long)g.chunks * g.tiles * (long long)sizeof(double2), "workspace too small (gm_ssim_workspace_bytes)");
  GM_REQUIRE(ssim_lds_floats(g) * (long long)sizeof(float) <= 160 * 1024, "LDS plan exceeds 160 KiB");
  SsimTaps taps = {};
  for (int j = 0; j < kd; ++j) taps.d[j] = taps_d[j];
  for (int j = 0; j < kh; ++j) taps.h[j] = taps_h[j];
  for (int j = 0; j < kw; ++j) taps.w[j] = taps_w[j];
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  if (!gm_dispatch_dtype_f16(dtype, [&](auto tv) {
        rc = ssim_launch<typename decltype(tv)::type>(x, y, B, C, g, c1, c2, taps, ssim_mean, cs_mean, ssim_map, cs_map, workspace, st);
      })) GM_FAIL(-2, "unsupported dtype");
  return rc;
}

// ---- avg_pool{2,3}d(kernel_size=2) of two images at once: (nvol, D, H, W) -> (nvol, D / pd, H / 2, W / 2) fp32, pd = 2 (3-D) or 1 (2-D) ---------------------
template <typename T>
__global__ __launch_bounds__(256) void avgpool2_pair_kernel(const T* __restrict__ a, const T* __restrict__ b, float* __restrict__ oa, float* __restrict__ ob,
                                                           long long total, int D, int H, int W, int Dp, int Hp, int Wp, int pd) {
  const float inv = pd == 2 ? 0.125f : 0.25f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int w = (int)(i % Wp);
    long long r = i / Wp;
    const int h = (int)(r % Hp);
    r /= Hp;
    const int d = (int)(r % Dp);
    const long long vol = r / Dp;
    const long long base = ((vol * D + (long long)d * pd) * H + 2 * h) * W + 2 * w;  // 2h + 1 < H, 2w + 1 < W, d * pd + pd - 1 < D by the floor
    float sa = 0.0f, sb = 0.0f;
    for (int z = 0; z < pd; ++z) {
      const long long o = base + (long long)z * H * W;
      sa += ElemIO<T>::ld(a + o) + ElemIO<T>::ld(a + o + 1) + ElemIO<T>::ld(a + o + W) + ElemIO<T>::ld(a + o + W + 1);
      sb += ElemIO<T>::ld(b + o) + ElemIO<T>::ld(b + o + 1) + ElemIO<T>::ld(b + o + W) + ElemIO<T>::ld(b + o + W + 1);
    }
    oa[i] = sa * inv;
    ob[i] = sb * inv;
  }
}

extern "C" int gm_avgpool2_pair(const void* a, const void* b, int dtype, float* out_a, float* out_b, long long nvol, int D, int H, int W, int pool_depth,
                                void* stream) {
  GM_REQUIRE(a && b && out_a && out_b, "null pointer");
  GM_REQUIRE(nvol > 0 && D > 0 && H > 0 && W > 0, "empty input");
  const int pd = pool_depth ? 2 : 1;
  const int Dp = D / pd, Hp = H / 2, Wp = W / 2;
  GM_REQUIRE(Dp > 0 && Hp > 0 && Wp > 0, "an extent below 2 cannot be pooled");
  const long long total = nvol * Dp * Hp * Wp;
  long long gx = (total + 255) / 256;
  if (gx > 65536) gx = 65536;
  hipStream_t st = (hipStream_t)stream;
  if (!gm_dispatch_dtype_f16(dtype, [&](auto tv) {
        using T = typename decltype(tv)::type;
        avgpool2_pair_kernel<T><<<(unsigned)gx, 256, 0, st>>>((const T*)a, (const T*)b, out_a, out_b, total, D, H, W, Dp, Hp, Wp, pd);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

// ---- MMD: mean(Y Y^T) = |sum_i y_i|^2 / B^2, so the three Gram means are dot products of the two column-sum vectors -------------------------------------
static long long mmd_blocks(long long F) {
  long long gx = (F + 255) / 256;
  return gx > 1024 ? 1024 : (gx < 1 ? 1 : gx);
}

struct MmdPartial { double yy, pp, py; };

template <typename T>
__global__ __launch_bounds__(256) void mmd_colsum_kernel(const T* __restrict__ y, const T* __restrict__ p, long long B, long long F, MmdPartial* __restrict__ partials) {
  double yy = 0.0, pp = 0.0, py = 0.0;
  for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (long long)gridDim.x * blockDim.x) {
    double sy = 0.0, sp = 0.0;
    for (long long r = 0; r < B; ++r) {
      sy += (double)ElemIO<T>::ld(y + r * F + f);
      sp += (double)ElemIO<T>::ld(p + r * F + f);
    }
    yy += sy * sy;
    pp += sp * sp;
    py += sp * sy;
  }
  __shared__ double part[3][4];
  yy = wave_sum(yy);
  pp = wave_sum(pp);
  py = wave_sum(py);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = yy;
    part[1][threadIdx.x >> 6] = pp;
    part[2][threadIdx.x >> 6] = py;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    MmdPartial r;
    r.yy = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    r.pp = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    r.py = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    partials[blockIdx.x] = r;
  }
}

// beta * (mean(yy / F) + mean(pp / F)) - gamma * mean(py / F), beta = 1, gamma = 2 (mmd.py:75-80); the partials are added in block order
__global__ void mmd_fold_kernel(const MmdPartial* __restrict__ partials, int parts, double inv_b2f, float* __restrict__ out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double yy = 0.0, pp = 0.0, py = 0.0;
    for (int j = 0; j < parts; ++j) {
      yy += partials[j].yy;
      pp += partials[j].pp;
      py += partials[j].py;
    }
    out[0] = (float)(1.0 * (yy * inv_b2f + pp * inv_b2f) - 2.0 * (py * inv_b2f));
  }
}

extern "C" long long gm_mmd_workspace_bytes(long long B, long long F) {
  (void)B;
  return mmd_blocks(F) * (long long)sizeof(MmdPartial);
}

extern "C" int gm_mmd(const void* y, const void* y_pred, int dtype, long long B, long long F, float* out, void* workspace, long long workspace_bytes,
                      void* stream) {
  GM_REQUIRE(y && y_pred && out && workspace, "null pointer");
  GM_REQUIRE(B > 0 && F > 0, "empty input");
  const long long gx = mmd_blocks(F);
  GM_REQUIRE(workspace_bytes >= gx * (long long)sizeof(MmdPartial), "workspace too small (gm_mmd_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  MmdPartial* ws = (MmdPartial*)workspace;
  if (!gm_dispatch_dtype_f16(dtype, [&](auto tv) {
        using T = typename decltype(tv)::type;
        mmd_colsum_kernel<T><<<(unsigned)gx, 256, 0, st>>>((const T*)y, (const T*)y_pred, B, F, ws);
      })) GM_FAIL(-2, "unsupported dtype");
  mmd_fold_kernel<<<1, 64, 0, st>>>(ws, (int)gx, 1.0 / ((double)B * (double)B * (double)F), out);
  GM_LAUNCH_CHECK();
}
