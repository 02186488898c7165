// The backward of gm_ssim_cs (metrics.hip) on gfx950, in two launches on the forward's structure -- a 16 x 16 (H, W) tile per work-group, a march along D,
// a ring of kd planes in LDS, k taps per axis:
//   ssim_coef_kernel     recomputes the five local moments and stores d(loss) / d(moment) per valid position as four fp32 maps
//                        (d sigma_x = d sigma_y, so the five coefficients are four maps)
//   ssim_gather_kernel   filters those maps with the transposed ("full") separable correlation over the INPUT extents, combines them with x(q), y(q) and
//                        stores dx and / or dy once; the backward of the 2x pooling between two MS-SSIM scales rides in its epilogue
// Every output element is one thread's sum in a fixed tap order: no atomics, bit-reproducible, and a batch item's gradient does not depend on its neighbours.
#include "gm_common.h"
#include "ssim_common.h"

#define SSIM_BWD_MAPS 4  // d mx, d my, d sigma (x and y alike), d sigma_xy

// With l = n1 / d1 and cs = n2 / d2 (ssim = l * cs) and the upstream gs, gc of ssim and cs at this position:
//   gcs = gc + gs l, gl = gs cs;  d sigma_xy = 2 gcs / d2;  d sigma_x = d sigma_y = -gcs n2 / d2^2;
//   d mx = gl (2 my / d1 - 2 mx n1 / d1^2) - 2 mx d sigma_x - my d sigma_xy, and d my with x and y exchanged
__device__ __forceinline__ void ssim_point_grad(float mx, float my, float mxx, float myy, float mxy, float c1, float c2, float gs, float gc, float* out) {
  const float sigma_x = mxx - mx * mx;
  const float sigma_y = myy - my * my;
  const float sigma_xy = mxy - mx * my;
  const float d1 = mx * mx + my * my + c1, d2 = sigma_x + sigma_y + c2;
  const float l = (2.0f * mx * my + c1) / d1;
  const float cs = (2.0f * sigma_xy + c2) / d2;
  const float gcs = gc + gs * l;
  const float a = 2.0f * (gs * cs) / d1;
  const float dsxy = 2.0f * gcs / d2;
  const float dsig = -gcs * cs / d2;
  out[0] = a * (my - mx * l) - 2.0f * mx * dsig - my * dsxy;
  out[1] = a * (mx - my * l) - 2.0f * my * dsig - mx * dsxy;
  out[2] = dsig;
  out[3] = dsxy;
}

// The forward's march (ssim_cs_kernel: same plan, same LDS layout, same tap order), ending in the coefficients instead of the values.  The upstream of a
// position is gs_mean[b] / count + gs_map[p] (and gc alike), each operand nullable.  coef: [4][volumes * Do * Ho * Wo].  The march is restated here, not
// shared as a template body, so that ssim_cs_kernel's instantiations are compiled from the text they always were and keep their bits.
template <typename T>
__global__ __launch_bounds__(256) void ssim_coef_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ gs_mean,
                                                       const float* __restrict__ gc_mean, const float* __restrict__ gs_map, const float* __restrict__ gc_map,
                                                       float* __restrict__ coef, long long coef_stride, SsimGeom g, int C, double count, float c1, float c2,
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
  const float gs0 = gs_mean ? (float)((double)gs_mean[vol / C] / count) : 0.0f;
  const float gc0 = gc_mean ? (float)((double)gc_mean[vol / C] / count) : 0.0f;
  int slot = 0;  // ring slot of input plane dz: (dz - od0) % kd
  for (int dz = od0; dz < od1 + g.kd - 1; ++dz) {
    {  // halo of both images; outside the volume reads as 0 (it only feeds outputs that are not kept)
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
    // no barrier here: a thread reads back only the ring entries it wrote itself, and the next plane's W pass (which overwrites wf) sits behind its halo barrier
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
        const long long o = out_base + (long long)(dz - (g.kd - 1)) * g.Ho * g.Wo;
        float k[SSIM_BWD_MAPS];
        ssim_point_grad(s[0], s[1], s[2], s[3], s[4], c1, c2, gs0 + (gs_map ? gs_map[o] : 0.0f), gc0 + (gc_map ? gc_map[o] : 0.0f), k);
#pragma unroll
        for (int f = 0; f < SSIM_BWD_MAPS; ++f) coef[f * coef_stride + o] = k[f];
      }
    }
    slot = slot + 1 == g.kd ? 0 : slot + 1;
  }
}

// The transposed correlation is the forward's "valid" correlation of the coefficient maps padded with k - 1 zeros per side, under flipped tables: `g` is the
// forward plan of that padded volume (g.Do, g.Ho, g.Wo = the INPUT extents D, H, W; padded position u is coefficient position u - (k - 1)), `taps` arrive
// flipped.  Per padded plane: the halo of the four maps goes to LDS, the W pass and the H pass filter it into one slot of the ring, the D pass filters across
// the ring; a plane of padding skips the passes and zeroes its slot.  The epilogue forms
//   dx(q) = A(q) + 2 x(q) B(q) + y(q) C(q),   dy(q) = A'(q) + 2 y(q) B(q) + x(q) C(q)      (A, A', B, C: the filtered d mx, d my, d sigma, d sigma_xy)
// adds pooled_dx / pooled_dy [q / 2] / 2^d -- the gradient of the next coarser MS-SSIM scale through avg_pool(kernel_size=2), nothing at an odd tail the
// floor dropped -- and stores each once in the dtype of the inputs.  Both values are always formed, so a one-sided call stores the bits of a two-sided one.
template <typename T>
__global__ __launch_bounds__(256) void ssim_gather_kernel(const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ coef, long long coef_stride,
                                                         const float* __restrict__ pooled_dx, const float* __restrict__ pooled_dy, T* __restrict__ dx,
                                                         T* __restrict__ dy, SsimGeom g, int pool_depth, SsimTaps taps) {
  extern __shared__ __align__(16) float lds[];
  constexpr int NF = SSIM_BWD_MAPS;
  const int RH = SSIM_TH + g.kh - 1, RW = SSIM_TW + g.kw - 1;
  float* raw = lds;                        // [4][RH][RW]
  float* wf = raw + NF * RH * RW;          // [4][RH][16]
  float* ring = wf + NF * RH * SSIM_TW;    // [kd][4][256]; a thread reads back only what it wrote itself: two barriers per plane
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % g.tiles, chunk = blockIdx.x / g.tiles;
  const long long vol = blockIdx.y;
  const int th0 = (tile / g.tiles_w) * SSIM_TH, tw0 = (tile % g.tiles_w) * SSIM_TW;
  const int od0 = chunk * g.dc;
  const int od1 = min(g.Do, od0 + g.dc);
  const int ty = tid >> 4, tx = tid & 15;
  const int qh = th0 + ty, qw = tw0 + tx;
  const bool valid = qh < g.Ho && qw < g.Wo;
  const int cD = g.Do - g.kd + 1, cH = g.Ho - g.kh + 1, cW = g.Wo - g.kw + 1;  // extents of the coefficient maps
  const float* cv = coef + vol * cD * cH * cW;
  const long long in_plane = (long long)g.Ho * g.Wo;
  const long long in_base = vol * g.Do * in_plane + (long long)qh * g.Wo + qw;
  const int pD = g.Do >> pool_depth, pH = g.Ho >> 1, pW = g.Wo >> 1;  // extents of the pooled gradients
  const float pool_w = pool_depth ? 0.125f : 0.25f;
  int slot = 0;  // ring slot of padded plane dz: (dz - od0) % kd
  for (int dz = od0; dz < od1 + g.kd - 1; ++dz) {
    const int cd = dz - (g.kd - 1);
    if (cd >= 0 && cd < cD) {  // (uniform over the work-group)
      {
        const int c = tid & 31;
        const int cw = tw0 + c - (g.kw - 1);
        for (int r = tid >> 5; r < RH; r += 8) {
          const int ch = th0 + r - (g.kh - 1);
          if (c < RW) {
            const bool in = ch >= 0 && ch < cH && cw >= 0 && cw < cW;
            const long long o = ((long long)cd * cH + ch) * cW + cw;
#pragma unroll
            for (int f = 0; f < NF; ++f) raw[(f * RH + r) * RW + c] = in ? cv[f * coef_stride + o] : 0.0f;
          }
        }
      }
      __syncthreads();
      for (int i = tid; i < RH * SSIM_TW; i += 256) {  // W pass
        const int r = i >> 4, c = i & 15;
        const float* p = raw + r * RW + c;
        float s[NF] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < g.kw; ++j) {
          const float t = taps.w[j];
#pragma unroll
          for (int f = 0; f < NF; ++f) s[f] += t * p[f * RH * RW + j];
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) wf[f * RH * SSIM_TW + i] = s[f];
      }
      __syncthreads();
      {  // H pass -> ring[slot]
        float s[NF] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < g.kh; ++j) {
          const float t = taps.h[j];
          const float* p = wf + (ty + j) * SSIM_TW + tx;
#pragma unroll
          for (int f = 0; f < NF; ++f) s[f] += t * p[f * RH * SSIM_TW];
        }
        float* q = ring + slot * NF * 256 + tid;
#pragma unroll
        for (int f = 0; f < NF; ++f) q[f * 256] = s[f];
      }
    } else {
      float* q = ring + slot * NF * 256 + tid;
#pragma unroll
      for (int f = 0; f < NF; ++f) q[f * 256] = 0.0f;
    }
    if (dz - od0 >= g.kd - 1) {  // D pass: input plane od = dz - (kd - 1); tap j meets padded plane od + j, which sits in slot (slot + 1 + j) % kd
      float s[NF] = {0.0f, 0.0f, 0.0f, 0.0f};
      int sl = slot + 1 == g.kd ? 0 : slot + 1;
      for (int j = 0; j < g.kd; ++j) {
        const float t = taps.d[j];
        const float* p = ring + sl * NF * 256 + tid;
#pragma unroll
        for (int f = 0; f < NF; ++f) s[f] += t * p[f * 256];
        sl = sl + 1 == g.kd ? 0 : sl + 1;
      }
      if (valid) {
        const int od = dz - (g.kd - 1);
        const long long o = in_base + (long long)od * in_plane;
        const float xq = ElemIO<T>::ld(x + o), yq = ElemIO<T>::ld(y + o);
        float gx = s[0] + 2.0f * xq * s[2] + yq * s[3];
        float gy = s[1] + 2.0f * yq * s[2] + xq * s[3];
        const int zd = od >> pool_depth, zh = qh >> 1, zw = qw >> 1;
        if (zd < pD && zh < pH && zw < pW) {
          const long long po = ((vol * pD + zd) * pH + zh) * pW + zw;
          if (pooled_dx) gx += pooled_dx[po] * pool_w;
          if (pooled_dy) gy += pooled_dy[po] * pool_w;
        }
        if (dx) ElemIO<T>::st(dx + o, gx);
        if (dy) ElemIO<T>::st(dy + o, gy);
      }
    }
    slot = slot + 1 == g.kd ? 0 : slot + 1;
  }
}

// the gather's plan: the forward plan of the coefficient maps padded to D + kd - 1, H + kh - 1, W + kw - 1
static SsimGeom ssim_gather_geom(int D, int H, int W, int kd, int kh, int kw) { return ssim_geom(D + kd - 1, H + kh - 1, W + kw - 1, kd, kh, kw); }

// bytes of gm_ssim_cs_backward's workspace: the four fp32 coefficient maps of the valid extents; needs no initialisation.  < 0: bad geometry (gm_last_error)
extern "C" long long gm_ssim_backward_workspace_bytes(long long B, long long C, int D, int H, int W, int kd, int kh, int kw) {
  if (ssim_check_geom(B, C, D, H, W, kd, kh, kw) != 0) return -1;
  return SSIM_BWD_MAPS * B * C * (long long)(D - kd + 1) * (H - kh + 1) * (W - kw + 1) * (long long)sizeof(float);
}

template <typename T>
static int ssim_backward_launch(const void* x, const void* y, long long B, long long C, const SsimGeom& g, const SsimGeom& gg, float c1, float c2,
                                const SsimTaps& taps, const SsimTaps& flipped, const float* gs_mean, const float* gc_mean, const float* gs_map,
                                const float* gc_map, const float* pooled_dx, const float* pooled_dy, int pool_depth, void* dx, void* dy, float* coef, hipStream_t st) {
  static bool attr_done = false;  // (per instantiation)
  if (!attr_done) {
    for (const void* k : {reinterpret_cast<const void*>(ssim_coef_kernel<T>), reinterpret_cast<const void*>(ssim_gather_kernel<T>)}) {
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      if (e != hipSuccess) GM_FAIL((int)e, hipGetErrorString(e));
    }
    attr_done = true;
  }
  const long long coef_stride = B * C * (long long)g.Do * g.Ho * g.Wo;
  const long long per_vol = (long long)g.chunks * g.tiles, per_vol_in = (long long)gg.chunks * gg.tiles;
  GM_REQUIRE(per_vol <= 0x7fffffffLL && per_vol_in <= 0x7fffffffLL, "too many work-groups per volume");
  const double count = (double)C * g.Do * g.Ho * g.Wo;
  ssim_coef_kernel<T><<<dim3((unsigned)per_vol, (unsigned)(B * C)), 256, (size_t)ssim_lds_floats(g) * sizeof(float), st>>>(
      (const T*)x, (const T*)y, gs_mean, gc_mean, gs_map, gc_map, coef, coef_stride, g, (int)C, count, c1, c2, taps);
  ssim_gather_kernel<T><<<dim3((unsigned)per_vol_in, (unsigned)(B * C)), 256, (size_t)ssim_lds_floats(gg, SSIM_BWD_MAPS, SSIM_BWD_MAPS) * sizeof(float), st>>>(
      (const T*)x, (const T*)y, coef, coef_stride, pooled_dx, pooled_dy, (T*)dx, (T*)dy, gg, pool_depth, flipped);
  GM_LAUNCH_CHECK();
}

extern "C" int gm_ssim_cs_backward(const void* x, const void* y, int dtype, long long B, long long C, int D, int H, int W, const float* taps_d, int kd,
                                   const float* taps_h, int kh, const float* taps_w, int kw, float c1, float c2, const float* g_ssim_mean,
                                   const float* g_cs_mean, const float* g_ssim_map, const float* g_cs_map, const float* pooled_dx, const float* pooled_dy,
                                   int pool_depth, void* dx, void* dy, void* workspace, long long workspace_bytes, void* stream) {
  GM_REQUIRE(x && y && taps_d && taps_h && taps_w && workspace, "null pointer");
  GM_REQUIRE(g_ssim_mean || g_cs_mean || g_ssim_map || g_cs_map, "no upstream gradient");
  GM_REQUIRE(dx || dy, "no gradient requested");
  if (ssim_check_geom(B, C, D, H, W, kd, kh, kw) != 0) return -1;
  GM_REQUIRE(C <= 0x7fffffffLL, "too many channels");
  pool_depth = pool_depth ? 1 : 0;  // the kernel shifts by it
  if (pooled_dx || pooled_dy) GM_REQUIRE((D >> pool_depth) > 0 && H / 2 > 0 && W / 2 > 0, "an extent below 2 has no pooled gradient");
  const SsimGeom g = ssim_geom(D, H, W, kd, kh, kw), gg = ssim_gather_geom(D, H, W, kd, kh, kw);
  GM_REQUIRE(workspace_bytes >= SSIM_BWD_MAPS * B * C * (long long)g.Do * g.Ho * g.Wo * (long long)sizeof(float),
             "workspace too small (gm_ssim_backward_workspace_bytes)");
  GM_REQUIRE(ssim_lds_floats(g) * (long long)sizeof(float) <= 160 * 1024 &&
                 ssim_lds_floats(gg, SSIM_BWD_MAPS, SSIM_BWD_MAPS) * (long long)sizeof(float) <= 160 * 1024, "LDS plan exceeds 160 KiB");
  SsimTaps taps = {}, flipped = {};
  for (int j = 0; j < kd; ++j) { taps.d[j] = taps_d[j]; flipped.d[j] = taps_d[kd - 1 - j]; }
  for (int j = 0; j < kh; ++j) { taps.h[j] = taps_h[j]; flipped.h[j] = taps_h[kh - 1 - j]; }
  for (int j = 0; j < kw; ++j) { taps.w[j] = taps_w[j]; flipped.w[j] = taps_w[kw - 1 - j]; }
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  if (!gm_dispatch_dtype_f16(dtype, [&](auto tv) {
        rc = ssim_backward_launch<typename decltype(tv)::type>(x, y, B, C, g, gg, c1, c2, taps, flipped, g_ssim_mean, g_cs_mean, g_ssim_map, g_cs_map,
                                                               pooled_dx, pooled_dy, pool_depth, dx, dy, (float*)workspace, st);
      })) GM_FAIL(-2, "unsupported dtype");
  return rc;
}
