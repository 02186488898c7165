// Host-side plan of the separable SSIM kernels, shared by the forward (metrics.hip) and the backward (metrics_bwd.hip).
#pragma once
#include "gm_common.h"

#define SSIM_MAX_WINDOW 16   // taps per axis the kernel is built for
#define SSIM_TH 16           // output tile (H, W) of a work-group; 256 threads, one output column each
#define SSIM_TW 16

struct SsimTaps { float d[SSIM_MAX_WINDOW], h[SSIM_MAX_WINDOW], w[SSIM_MAX_WINDOW]; };

struct SsimGeom {
  int D, H, W, kd, kh, kw, Do, Ho, Wo;
  int tiles_w, tiles;  // (H, W) tiles of SSIM_TH x SSIM_TW outputs
  int dc, chunks;      // output planes per work-group, work-groups along D
};

// One deterministic plan per volume geometry: the partial count, hence the summation order, depends on nothing else -- not on the batch size either, so a
// batch item's value does not depend on its neighbours.
static inline SsimGeom ssim_geom(int D, int H, int W, int kd, int kh, int kw) {
  SsimGeom g;
  g.D = D; g.H = H; g.W = W; g.kd = kd; g.kh = kh; g.kw = kw;
  g.Do = D - kd + 1; g.Ho = H - kh + 1; g.Wo = W - kw + 1;
  g.tiles_w = gm_cdiv(g.Wo, SSIM_TW);
  g.tiles = g.tiles_w * gm_cdiv(g.Ho, SSIM_TH);
  // a chunk re-filters kd - 1 planes of its neighbour: split D only as far as it takes for ONE volume to fill the chip (~1024 work-groups), and keep at least
  // 2 * kd output planes per chunk so that the redundant work stays under a third
  long long want = 1024 / g.tiles;
  if (want < 1) want = 1;
  int dc = gm_cdiv(g.Do, want);
  if (dc < 2 * kd) dc = 2 * kd;
  if (dc > g.Do) dc = g.Do;
  g.dc = dc;
  g.chunks = gm_cdiv(g.Do, dc);
  return g;
}

// floats of LDS of a march that filters `fields` maps from `sources` staged images: halo + W-filtered rows + the ring of kd planes
static inline long long ssim_lds_floats(const SsimGeom& g, int sources = 2, int fields = 5) {
  const long long rh = SSIM_TH + g.kh - 1, rw = SSIM_TW + g.kw - 1;
  return sources * rh * rw + fields * rh * SSIM_TW + (long long)g.kd * fields * SSIM_TH * SSIM_TW;
}

static inline int ssim_check_geom(long long B, long long C, int D, int H, int W, int kd, int kh, int kw) {
  GM_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, "empty input");
  GM_REQUIRE(kd >= 1 && kh >= 1 && kw >= 1 && kd <= SSIM_MAX_WINDOW && kh <= SSIM_MAX_WINDOW && kw <= SSIM_MAX_WINDOW, "window size outside 1..16");
  GM_REQUIRE(kd <= D && kh <= H && kw <= W, "window larger than the image");
  GM_REQUIRE(B * C <= 65535, "more than 65535 volumes");
  return 0;
}
