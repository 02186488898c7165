// Softmax attention for wide heads, 256 < head dim <= GM_ATTN_WIDE_MAX_DH (1024): the 512- and 768-channel heads of the reference's wide networks
// (DiffusionModelUNet with num_head_channels 512 / 768, an AutoencoderKL whose non-local attention spans a 512-channel level).
//
// The register-staged attn_kernel (attention.hip) keeps a lane's Q fragments and its whole O^T accumulator in registers; at head dim 256 it is
// already at one wave per SIMD, and its K + V^T tiles would outgrow the LDS beyond that.  Here a work-group owns 64 queries x ONE OUTPUT SLICE of
// W = 256 channels (blockIdx.z), so its accumulator is exactly the head-dim-256 kernel's:
//   S^T = sum_c K_c Q_c^T      over the head dim in W-channel chunks c = 0, 1, ... (K_c staged per key tile, Q_c fragments read from global memory
//                              one stage ahead -- 64 queries x W channels, L2-resident: every slice of the same queries reads them)
//   online softmax on S^T      as attn_kernel, lane-local (a lane owns one query)
//   O^T_slice += V_slice^T P^T as attn_kernel (bf16: V transposed in 8x8 register blocks at the commit)
// Every slice sums the chunks in the same fixed order, so all slices see bit-identical scores, maxima and normalisers.  The cost: QK^T is
// recomputed once per slice -- (n_slices + 1) / 2 x the arithmetic of one pass.
//
// Staging is one pipeline of STAGES: per key tile, n_chunks K chunks then the V slice ([KT][W] each).
// Stage s + 1 is requested into registers right after stage s has been committed to LDS, so its memory latency runs under stage s's MFMAs.
#include "gm_common.h"

#include "attn_common.h"

namespace {

constexpr int WIDE_W = 256;  // channels per score chunk and per output slice

// 16 bytes of row `row` at element offset c0 (zero outside [0, climit) / invalid rows); scalar loads when the row is not 16-byte friendly
template <typename T>
__device__ __forceinline__ uint4 wide_load16(const T* base, long long ld, long long row, bool row_ok, int c0, int climit, bool vec_ok) {
  constexpr int VECW = 16 / sizeof(T);
  uint4 r = make_uint4(0, 0, 0, 0);
  if (!row_ok || c0 >= climit) return r;
  const T* p = base + row * ld + c0;
  if (vec_ok) return *reinterpret_cast<const uint4*>(p);
  uint32_t w[4];  // (assembled in registers: no private array)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (sizeof(T) == 2) {
      const uint32_t lo = c0 + 2 * i < climit ? (uint32_t)p[2 * i] : 0u, hi = c0 + 2 * i + 1 < climit ? (uint32_t)p[2 * i + 1] : 0u;
      w[i] = lo | (hi << 16);
    } else {
      w[i] = c0 + i < climit ? __float_as_uint(p[i]) : 0u;
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// word i (a compile-time constant after unrolling) of a 16-byte register vector, without taking its address
__device__ __forceinline__ uint32_t u4_word(const uint4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

template <typename T> struct WideTraits;
template <> struct WideTraits<bf16_raw> { static constexpr int KT = 64; };
template <> struct WideTraits<float> { static constexpr int KT = 32; };

template <typename T>
constexpr size_t wide_lds_bytes() {
  constexpr int KT = WideTraits<T>::KT;
  return (size_t)KT * (WIDE_W * sizeof(T) + 16) + (sizeof(T) == 2 ? (size_t)WIDE_W * (KT * 2 + 16) : (size_t)KT * (WIDE_W * 4 + 16));
}

template <typename T>
__global__ __launch_bounds__(256) void attn_wide_kernel(const GmAttnDesc p) {
  constexpr int VECW = 16 / (int)sizeof(T);
  constexpr int KT = WideTraits<T>::KT;
  constexpr int W = WIDE_W;
  constexpr int KF = KT / 16;                      // key fragments per tile
  constexpr int ROWB_K = W * (int)sizeof(T) + 16;  // K chunk row pitch (bytes)
  constexpr int STEPS = W * (int)sizeof(T) / 64;   // 64-byte k-steps over a chunk
  constexpr int DF = W / 16;                       // output channel fragments of the slice
  constexpr bool IS_BF16 = sizeof(T) == 2;
  constexpr int ROWB_V = IS_BF16 ? (KT * 2 + 16) : (W * 4 + 16);  // bf16: V^T rows of KT keys; fp32: V rows of W channels
  constexpr int CHK = W * (int)sizeof(T) / 16;     // 16-byte chunks per K row (fp32: and per V row)
  constexpr int NKI = KT * CHK / 256;              // K items per thread
  constexpr int PB = KT / 8, DB = W / 8;           // bf16 V: 8-key x 8-channel blocks
  constexpr int NSR = 8;                           // staging registers per thread (16 bytes each) of either kind of stage
  static_assert(KT * CHK % 256 == 0 && NKI == NSR, "K stage: 8 vectors per thread");
  static_assert(!IS_BF16 || PB * DB == 256, "bf16 V stage: one 8x8 block per thread");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsK = smem;                          // [KT][ROWB_K]
  char* ldsV = ldsK + (size_t)KT * ROWB_K;    // bf16: [W][ROWB_V] (transposed), fp32: [KT][ROWB_V]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, qg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int c_out = blockIdx.z * W;  // first head channel of this work-group's output slice
  const int q0 = blockIdx.x * 64 + wave * 16;
  const int my_q = q0 + l15;
  const bool q_ok = my_q < p.Lq;

  const T* Qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.Lq * p.q_ld + (long long)h * p.dh;
  const T* Kb = reinterpret_cast<const T*>(p.k) + (long long)b * (p.k_bs ? p.k_bs : p.Lk * p.k_ld) + (long long)h * p.dh;
  const T* Vb = reinterpret_cast<const T*>(p.v) + (long long)b * (p.v_bs ? p.v_bs : p.Lk * p.v_ld) + (long long)h * p.dh;
  const bool qvec = (p.dh % VECW == 0) && (p.q_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(Qb) & 15) == 0);
  const bool kvec = (p.dh % VECW == 0) && (p.k_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(Kb) & 15) == 0);
  const bool vvec = (p.dh % VECW == 0) && (p.v_ld % VECW == 0) && ((reinterpret_cast<uintptr_t>(Vb) & 15) == 0);

  const int nchunks = (p.dh + W - 1) / W;

  // causal: this lane's query sees keys <= my_q + (Lk - Lq); the work-group stops after the tile holding its last visible key
  const int kmax = p.causal ? my_q + (p.Lk - p.Lq) : p.Lk;
  int ntiles = (p.Lk + KT - 1) / KT;
  if (p.causal) {
    const int last = min(p.Lk - 1, (int)blockIdx.x * 64 + 63 + (p.Lk - p.Lq));
    ntiles = max(1, min(ntiles, last / KT + 1));
  }

  uint4 kreg[NSR];     // the next stage's K chunk ...
  uint4 vreg[NSR];     // ... or V slice (bf16: 8 keys x 8 channels, transposed at the commit)
  uint4 qreg[STEPS];   // the next K stage's Q fragments ...
  uint4 qf[STEPS];     // ... and the current one's: lane (query l15, slot qg) holds chunk channels s*4*VECW + qg*VECW .. + VECW-1
  f32x4_t sacc[KF];
  f32x4_t oacc[DF];
#pragma unroll
  for (int d = 0; d < DF; ++d) oacc[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kf = 0; kf < KF; ++kf) sacc[kf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  // ---- staging: a K stage is one chunk of K (plus the queries' Q fragments of that chunk), a V stage this work-group's V slice; both [KT][W] -------
  auto fetch_k = [&](int tile, int c) __attribute__((always_inline)) {
    const int key0 = tile * KT, ch0 = c * W;
#pragma unroll
    for (int it = 0; it < NKI; ++it) {
      const int item = tid + it * 256;
      const int row = item / CHK, ch = item % CHK;
      kreg[it] = wide_load16<T>(Kb, p.k_ld, key0 + row, key0 + row < p.Lk, ch0 + ch * VECW, p.dh, kvec);
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) qreg[s] = wide_load16<T>(Qb, p.q_ld, my_q, q_ok, ch0 + (s * 4 + qg) * VECW, p.dh, qvec);
  };
  auto fetch_v = [&](int tile) __attribute__((always_inline)) {
    const int key0 = tile * KT;
    if constexpr (IS_BF16) {
      // 8 keys x 8 channels per thread, transposed at the commit; key order inside a V^T row as in attn_kernel: the 8 keys lane-group qq feeds
      // into k-step s of the PV MFMA are contiguous (one ds_read_b128)
      const int pb = tid % PB, db = tid / PB;
      const int sq = pb >> 2, qq = pb & 3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = key0 + (2 * sq + (j >> 2)) * 16 + qq * 4 + (j & 3);
        vreg[j] = wide_load16<T>(Vb, p.v_ld, key, key < p.Lk, c_out + db * 8, p.dh, vvec);
      }
    } else {
#pragma unroll
      for (int it = 0; it < NKI; ++it) {
        const int item = tid + it * 256;
        const int row = item / CHK, ch = item % CHK;
        vreg[it] = wide_load16<T>(Vb, p.v_ld, key0 + row, key0 + row < p.Lk, c_out + ch * VECW, p.dh, vvec);
      }
    }
  };
  auto commit_k = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < NKI; ++it) {
      const int item = tid + it * 256;
      *reinterpret_cast<uint4*>(ldsK + (size_t)(item / CHK) * ROWB_K + (item % CHK) * 16) = kreg[it];
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) qf[s] = qreg[s];
  };
  auto commit_v = [&]() __attribute__((always_inline)) {
    if constexpr (IS_BF16) {
      const int pb = tid % PB, db = tid / PB;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        uint32_t w[4];
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) {
          const uint32_t a = u4_word(vreg[2 * c2], d >> 1), bq = u4_word(vreg[2 * c2 + 1], d >> 1);
          w[c2] = (d & 1) ? ((a >> 16) | (bq & 0xffff0000u)) : ((a & 0xffffu) | (bq << 16));
        }
        *reinterpret_cast<uint4*>(ldsV + (size_t)(db * 8 + d) * ROWB_V + pb * 16) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    } else {
#pragma unroll
      for (int it = 0; it < NKI; ++it) {
        const int item = tid + it * 256;
        *reinterpret_cast<uint4*>(ldsV + (size_t)(item / CHK) * ROWB_V + (item % CHK) * 16) = vreg[it];
      }
    }
  };
  // ---- S^T += K_c Q_c^T over the chunk in LDS / the Q fragments in qf --------------------------------------------------------------------
  auto scores = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
      for (int kf = 0; kf < KF; ++kf) {
        const uint4 kfrag = *reinterpret_cast<const uint4*>(ldsK + (size_t)(kf * 16 + l15) * ROWB_K + s * 64 + qg * 16);
        if constexpr (IS_BF16) {
          sacc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kfrag), __builtin_bit_cast(bf16x8_t, qf[s]), sacc[kf], 0, 0, 0);
        } else {
          sacc[kf] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(kfrag.x), __uint_as_float(qf[s].x), sacc[kf], 0, 0, 0);
          sacc[kf] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(kfrag.y), __uint_as_float(qf[s].y), sacc[kf], 0, 0, 0);
          sacc[kf] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(kfrag.z), __uint_as_float(qf[s].z), sacc[kf], 0, 0, 0);
          sacc[kf] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(kfrag.w), __uint_as_float(qf[s].w), sacc[kf], 0, 0, 0);
        }
      }
    }
  };

  // Per key tile: K chunks 0 .. n-2 (each prefetching the next chunk), the last chunk (prefetching the V slice), the V slice (prefetching the
  // next tile's chunk 0).  Two barriers per stage: the previous stage's LDS reads are complete / this stage's data is visible.
  fetch_k(0, 0);
  for (int tile = 0; tile < ntiles; ++tile) {
    const int key0 = tile * KT;
#pragma unroll
    for (int kf = 0; kf < KF; ++kf) sacc[kf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nchunks - 1; ++c) {
      __syncthreads();
      commit_k();
      __syncthreads();
      fetch_k(tile, c + 1);  // in flight under this chunk's MFMAs
      scores();
    }
    __syncthreads();
    commit_k();
    __syncthreads();
    fetch_v(tile);
    scores();

    // ---- online softmax: this lane's query, keys key0 + kf*16 + qg*4 + r -------------------------------------------------------------------
    float tmax = -INFINITY;
#pragma unroll
    for (int kf = 0; kf < KF; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + kf * 16 + qg * 4 + r;
        const float sv = ((key < p.Lk) & (key <= kmax)) ? sacc[kf][r] * p.scale : -INFINITY;
        sacc[kf][r] = sv;
        tmax = fmaxf(tmax, sv);
      }
    tmax = attn_quad_max(tmax);
    const float m_new = fmaxf(m_run, tmax);
    const float m_ref = m_new == -INFINITY ? 0.f : m_new;  // (a query with no visible key yet: every weight e^(-inf) = 0)
    const float alpha = IS_BF16 ? __expf(m_run - m_ref) : expf(m_run - m_ref);
    float psum = 0.f;
#pragma unroll
    for (int kf = 0; kf < KF; ++kf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = IS_BF16 ? __expf(sacc[kf][r] - m_ref) : expf(sacc[kf][r] - m_ref);
        sacc[kf][r] = pv;
        psum += pv;
      }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int d = 0; d < DF; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[d][r] *= alpha;

    // ---- O^T_slice += V_slice^T P^T ------------------------------------------------------------------------------------------------------
    __syncthreads();
    commit_v();
    __syncthreads();
    if (tile + 1 < ntiles) fetch_k(tile + 1, 0);
    if constexpr (IS_BF16) {
      uint4 pf[KF / 2];
#pragma unroll
      for (int s = 0; s < KF / 2; ++s) {
        uint32_t w[4];
        w[0] = (uint32_t)f32_to_bf16(sacc[2 * s][0]) | ((uint32_t)f32_to_bf16(sacc[2 * s][1]) << 16);
        w[1] = (uint32_t)f32_to_bf16(sacc[2 * s][2]) | ((uint32_t)f32_to_bf16(sacc[2 * s][3]) << 16);
        w[2] = (uint32_t)f32_to_bf16(sacc[2 * s + 1][0]) | ((uint32_t)f32_to_bf16(sacc[2 * s + 1][1]) << 16);
        w[3] = (uint32_t)f32_to_bf16(sacc[2 * s + 1][2]) | ((uint32_t)f32_to_bf16(sacc[2 * s + 1][3]) << 16);
        pf[s] = make_uint4(w[0], w[1], w[2], w[3]);
      }
#pragma unroll
      for (int d = 0; d < DF; ++d)
#pragma unroll
        for (int s = 0; s < KF / 2; ++s) {
          const uint4 vfrag = *reinterpret_cast<const uint4*>(ldsV + (size_t)(d * 16 + l15) * ROWB_V + s * 64 + qg * 16);
          oacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vfrag), __builtin_bit_cast(bf16x8_t, pf[s]), oacc[d], 0, 0, 0);
        }
    } else {
#pragma unroll
      for (int d = 0; d < DF; ++d)
#pragma unroll
        for (int kf = 0; kf < KF; ++kf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float vv = *reinterpret_cast<const float*>(ldsV + (size_t)(kf * 16 + qg * 4 + i) * ROWB_V + (d * 16 + l15) * 4);
            oacc[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, sacc[kf][i], oacc[d], 0, 0, 0);
          }
    }
  }
  // ---- finish: 1/l, residual, store this slice's channels ------------------------------------------------------------
  const float inv = 1.0f / attn_quad_sum(l_run);
  if (!q_ok) return;
  T* orow = reinterpret_cast<T*>(p.o) + ((long long)b * p.Lq + my_q) * p.o_ld + (long long)h * p.dh;
  const T* rrow = p.res ? reinterpret_cast<const T*>(p.res) + ((long long)b * p.Lq + my_q) * p.res_ld + (long long)h * p.dh : nullptr;
#pragma unroll
  for (int d = 0; d < DF; ++d) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c_out + d * 16 + qg * 4 + r;
      if (c < p.dh) {
        float v = oacc[d][r] * inv;
        if (rrow) v += ElemIO<T>::ld(rrow + c);
        ElemIO<T>::st(orow + c, v);
      }
    }
  }
}

template <typename T>
int launch_attn_wide(const GmAttnDesc& d, hipStream_t st) {
  constexpr size_t smem = wide_lds_bytes<T>();
  static_assert(smem <= 160 * 1024, "LDS budget");
  static bool attr_set = false;
  auto kern = attn_wide_kernel<T>;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) (void)hipGetLastError();
    attr_set = true;
  }
  dim3 grid((d.Lq + 63) / 64, d.B * d.H, (d.dh + WIDE_W - 1) / WIDE_W);
  kern<<<grid, 256, smem, st>>>(d);
  return 0;
}

}  // namespace

// attention.hip: gm_attention_forward routes 256 < dh <= GM_ATTN_WIDE_MAX_DH here after its descriptor checks
int gm_attn_wide_dispatch(const GmAttnDesc& d, hipStream_t st) {
  if (d.dh <= 256 || d.dh > GM_ATTN_WIDE_MAX_DH) return -1;
  if (d.dtype == GM_F32) return launch_attn_wide<float>(d, st);
  if (d.dtype == GM_BF16) return launch_attn_wide<bf16_raw>(d, st);
  return -2;
}

extern "C" int gm_attention_max_wide_head_dim(void) { return GM_ATTN_WIDE_MAX_DH; }
