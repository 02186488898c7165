// Multi-tensor Adam / AdamW (optim.py): every tensor of an optimizer that holds a gradient is updated by ONE launch, driven by a descriptor table in
// device memory -- one entry per chunk of a tensor, one 256-thread work-group per entry (the grid is the chunk count).
//   entry (GM_OPTIM_ENTRY_WORDS = 8 64-bit words):  p, g, exp_avg, exp_avg_sq, max_exp_avg_sq (0 without amsgrad) | element count | index of the tensor's step
//                                                   counter | hyper-parameter row in bits 0..31, bit 32 = the planner found every pointer 16-byte aligned
//   hyper row (GM_OPTIM_HYPER_DOUBLES = 8 fp64):    lr, beta1, beta2, eps, weight_decay, flags (1 amsgrad, 2 maximize, 4 decoupled decay = AdamW), 0, 0
//   step counters:                                  fp32, one per parameter; a work-group reads t = counter + 1 and NO launch of this file writes a counter a
//                                                   work-group of the same launch reads: gm_adam_advance, enqueued behind the update, adds the 1.
// The arithmetic is torch's single-tensor order in fp32 registers; the scalars that depend on t (the two bias corrections) and the ones torch derives in Python
// doubles (1 - lr wd, 1 - beta) are made in fp64 by thread 0 of each work-group and rounded to fp32 once.  Moments are fp32 whatever the parameter dtype.
// This translation unit is compiled with -ffp-contract=off: adam_element is the one body of the update, inlined into the 16-byte path, its tail and the
// one-element path (gradients that are views into a flat bucket are only element aligned), and the three must give the same bits for the same values.
#include "gm_common.h"

#define OPT_AMSGRAD 1
#define OPT_MAXIMIZE 2
#define OPT_DECOUPLED 4

struct AdamCoef {
  float decay;      // 1 - lr wd (AdamW)
  float wd;         // weight_decay (Adam: g += wd p)
  float w1;         // 1 - beta1
  float b2, w2;     // beta2, 1 - beta2
  float eps;
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  int flags;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& vmax, const AdamCoef& c) {
  if (c.flags & OPT_MAXIMIZE) g = -g;
  if (c.wd != 0.f) {
    if (c.flags & OPT_DECOUPLED) p = p * c.decay;
    else g = g + c.wd * p;
  }
  m = m + (g - m) * c.w1;
  v = v * c.b2;
  v = v + (c.w2 * g) * g;
  float d;
  if (c.flags & OPT_AMSGRAD) {
    vmax = (v > vmax || v != v) ? v : vmax;  // torch.maximum: a NaN wins
    d = sqrtf(vmax);
  } else {
    d = sqrtf(v);
  }
  d = d / c.bc2_sqrt + c.eps;
  p = p - c.step_size * (m / d);
}

// VEC consecutive elements <-> floats without the hardware bf16 packer: the same software rounding (f32_to_bf16) on every path
template <typename T, int VEC> struct OptIO;
template <> struct OptIO<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* o) { Vec16<float>::unpack(*reinterpret_cast<const uint4*>(p), o); }
  static __device__ __forceinline__ void st(float* p, const float* o) { *reinterpret_cast<uint4*>(p) = Vec16<float>::pack(o); }
};
template <> struct OptIO<bf16_raw, 8> {
  static __device__ __forceinline__ void ld(const bf16_raw* p, float* o) { Vec16<bf16_raw>::unpack(*reinterpret_cast<const uint4*>(p), o); }
  static __device__ __forceinline__ void st(bf16_raw* p, const float* o) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f32_to_bf16(o[2 * i]) | ((uint32_t)f32_to_bf16(o[2 * i + 1]) << 16);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

template <typename T, int VEC>
__global__ __launch_bounds__(256) void adam_kernel(const long long* __restrict__ table, const float* __restrict__ steps, const double* __restrict__ hyper) {
  const long long* e = table + (long long)blockIdx.x * GM_OPTIM_ENTRY_WORDS;
  T* p = reinterpret_cast<T*>(e[0]);
  const T* g = reinterpret_cast<const T*>(e[1]);
  float* m = reinterpret_cast<float*>(e[2]);
  float* v = reinterpret_cast<float*>(e[3]);
  float* vmax = reinterpret_cast<float*>(e[4]);
  const long long n = e[5];
  __shared__ AdamCoef sc;
  if (threadIdx.x == 0) {
    const double* h = hyper + (e[7] & 0xffffffffll) * GM_OPTIM_HYPER_DOUBLES;
    const double t = (double)(steps[e[6]] + 1.0f);  // the counter's value after this step
    const double lr = h[0], b1 = h[1], b2 = h[2], wd = h[4];
    AdamCoef c;
    c.decay = (float)(1.0 - lr * wd);
    c.wd = (float)wd;
    c.w1 = (float)(1.0 - b1);
    c.b2 = (float)b2;
    c.w2 = (float)(1.0 - b2);
    c.eps = (float)h[3];
    c.step_size = (float)(lr / (1.0 - pow(b1, t)));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(b2, t));
    c.flags = (int)h[5];
    if (vmax == nullptr) c.flags &= ~OPT_AMSGRAD;  // (the host allocates max_exp_avg_sq whenever the row says amsgrad)
    sc = c;
  }
  __syncthreads();
  const AdamCoef c = sc;
  const bool ams = c.flags & OPT_AMSGRAD;
  const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax;
  const bool vec = ((e[7] >> 32) & 1) && (bits & 15) == 0;  // never a 16-byte access through a pointer that is not 16-byte aligned
  long long done = 0;
  if (vec) {
    const long long nv = n / VEC;
    for (long long i = threadIdx.x; i < nv; i += 256) {
      const long long o = i * VEC;
      float pp[VEC], gg[VEC], mm[VEC], vv[VEC], xx[VEC];
      OptIO<T, VEC>::ld(p + o, pp);
      OptIO<T, VEC>::ld(g + o, gg);
#pragma unroll
      for (int k = 0; k < VEC; k += 4) {
        OptIO<float, 4>::ld(m + o + k, mm + k);
        OptIO<float, 4>::ld(v + o + k, vv + k);
        if (ams) OptIO<float, 4>::ld(vmax + o + k, xx + k);
      }
#pragma unroll
      for (int k = 0; k < VEC; ++k) adam_element(pp[k], gg[k], mm[k], vv[k], xx[k], c);
      OptIO<T, VEC>::st(p + o, pp);
#pragma unroll
      for (int k = 0; k < VEC; k += 4) {
        OptIO<float, 4>::st(m + o + k, mm + k);
        OptIO<float, 4>::st(v + o + k, vv + k);
        if (ams) OptIO<float, 4>::st(vmax + o + k, xx + k);
      }
    }
    done = nv * VEC;
  }
  for (long long i = done + threadIdx.x; i < n; i += 256) {  // the whole chunk where a pointer is only element aligned, else the tail (< VEC elements)
    float pp = ElemIO<T>::ld(p + i), mm = m[i], vv = v[i], xx = ams ? vmax[i] : 0.f;
    adam_element(pp, ElemIO<T>::ld(g + i), mm, vv, xx, c);
    ElemIO<T>::st(p + i, pp);
    m[i] = mm;
    v[i] = vv;
    if (ams) vmax[i] = xx;
  }
}

__global__ __launch_bounds__(256) void adam_advance_kernel(float* __restrict__ steps, const int* __restrict__ active, int n_active) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_active) steps[active[i]] += 1.0f;  // (active holds every index once)
}

extern "C" int gm_adam_step(const long long* table, long long n_entries, const float* steps, const double* hyper, int dtype, void* stream) {
  GM_REQUIRE(table && steps && hyper, "null table");
  GM_REQUIRE(n_entries >= 1 && n_entries <= 0x7fffffffll, "1 <= entries < 2^31 (one work-group per entry)");
  GM_REQUIRE(gm_aligned16(table) && gm_aligned16(hyper), "tables must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == GM_F32) hipLaunchKernelGGL((adam_kernel<float, 4>), dim3((unsigned)n_entries), dim3(256), 0, s, table, steps, hyper);
  else if (dtype == GM_BF16) hipLaunchKernelGGL((adam_kernel<bf16_raw, 8>), dim3((unsigned)n_entries), dim3(256), 0, s, table, steps, hyper);
  else GM_FAIL(-2, "unsupported dtype");
  GM_LAUNCH_CHECK();
}

extern "C" int gm_adam_advance(float* steps, const int* active, int n_active, void* stream) {
  GM_REQUIRE(steps && active && n_active >= 1, "null / empty counter list");
  hipLaunchKernelGGL(adam_advance_kernel, dim3(gm_cdiv(n_active, 256)), dim3(256), 0, (hipStream_t)stream, steps, active, n_active);
  GM_LAUNCH_CHECK();
}

extern "C" int gm_optim_upload(void* dst, const void* src_pinned, long long bytes, void* stream) {
  GM_REQUIRE(dst && src_pinned && bytes > 0, "null / empty upload");
  hipError_t e = hipMemcpyAsync(dst, src_pinned, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) GM_FAIL((int)e, hipGetErrorString(e));
  return 0;
}
