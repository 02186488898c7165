// PatchAdversarialLoss over one discriminator output (losses/adversarial_loss.py): activation, criterion, reduction and the gradient with respect to the
// logits in one launch.  One work-group, fp64, fixed summation order (lane t adds elements t, t + 256, ... and a fixed LDS tree folds the 256 partials:
// the shape of gm_kld) -- a discriminator output is a few thousand logits, and the value is bitwise repeatable.
//   criterion 0  bce            a = sigmoid(x),                 l = -(t * max(log a, -100) + (1 - t) * max(log(1 - a), -100))   (torch.nn.BCELoss)
//   criterion 1  hinge          a = tanh(x),                    l = -min(t * a - 1, 0),  t = +1 (real) / -1 (fake)
//   criterion 2  least squares  a = LeakyReLU_0.05(x) or x,     l = (a - t)^2
#include "gm_common.h"

#define ADV_BCE 0
#define ADV_HINGE 1
#define ADV_LSQ 2

// -> the element's loss; d = its derivative with respect to the logit x
__device__ __forceinline__ double adv_term(double x, int criterion, int act, double t, double& d) {
  if (criterion == ADV_BCE) {
    const double a = 1.0 / (1.0 + exp(-x));
    double la = log(a), lb = log(1.0 - a);
    if (la < -100.0) la = -100.0;
    if (lb < -100.0) lb = -100.0;
    const double q = a * (1.0 - a);
    d = (a - t) / (q > 1e-12 ? q : 1e-12) * q;  // BCELoss's backward (its denominator is clamped at 1e-12) times sigmoid'
    return -(t * la + (1.0 - t) * lb);
  }
  if (criterion == ADV_HINGE) {
    const double a = tanh(x);
    const double v = t * a - 1.0;
    d = v < 0.0 ? -t * (1.0 - a * a) : (v == 0.0 ? -0.5 * t * (1.0 - a * a) : 0.0);  // (torch.min splits the gradient of a tie)
    return v < 0.0 ? -v : 0.0;
  }
  const double a = act && x <= 0.0 ? 0.05 * x : x;
  d = 2.0 * (a - t) * (act && x <= 0.0 ? 0.05 : 1.0);
  return (a - t) * (a - t);
}

template <typename T>
__global__ __launch_bounds__(256) void patch_adv_loss_kernel(const T* __restrict__ x, long long total, int criterion, int act, float target, double out_scale,
                                                            float* __restrict__ out, T* __restrict__ elem, const float* __restrict__ upstream,
                                                            const T* __restrict__ upstream_elem, T* __restrict__ dx) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  const double up = (upstream ? (double)*upstream : 1.0) * out_scale;
  double acc = 0.0;
  for (long long i = t; i < total; i += 256) {
    double d;
    const double l = adv_term((double)ElemIO<T>::ld(x + i), criterion, act, (double)target, d);
    acc += l;
    if (elem) ElemIO<T>::st(elem + i, (float)l);
    if (dx) ElemIO<T>::st(dx + i, (float)(d * (upstream_elem ? (double)ElemIO<T>::ld(upstream_elem + i) : up)));
  }
  if (!out) return;  // (uniform: no thread reaches the barriers)
  part[t] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) part[t] += part[t + s];
    __syncthreads();
  }
  if (t == 0) *out = (float)(part[0] * out_scale);
}

extern "C" int gm_patch_adv_loss(const void* x, long long total, int criterion, int act, float target, double out_scale, float* out, void* elem,
                                 const float* upstream, const void* upstream_elem, void* dx, int dtype, void* stream) {
  GM_REQUIRE(x, "null pointer");
  GM_REQUIRE(total >= 0, "negative size");
  GM_REQUIRE(criterion == ADV_BCE || criterion == ADV_HINGE || criterion == ADV_LSQ, "criterion: 0 bce, 1 hinge, 2 least squares");
  GM_REQUIRE(out || elem || dx, "nothing to write");
  GM_REQUIRE(!(upstream && upstream_elem), "one upstream gradient: a scalar or a map");
  GM_REQUIRE(dx || !(upstream || upstream_elem), "an upstream gradient without a gradient to write");
  hipStream_t st = (hipStream_t)stream;
  if (!gm_dispatch_dtype(dtype, [&](auto tv) {
        using T = typename decltype(tv)::type;
        if (total == 0 && !out) return;  // (an empty output still gets its value: 0)
        patch_adv_loss_kernel<T><<<1, 256, 0, st>>>((const T*)x, total, criterion, act, target, out_scale, out, (T*)elem, upstream, (const T*)upstream_elem,
                                                    (T*)dx);
      })) GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}
