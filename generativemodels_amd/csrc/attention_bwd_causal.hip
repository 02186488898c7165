// Causal flash-attention backward: dQ, dK, dV of O = softmax(mask(scale Q K^T)) V per (batch, head), where query i sees keys j <= i + off,
// off = Lk - Lq >= 0 (the forward's GmAttnDesc.causal; reference: torch autograd through blocks/selfattention.py:117-147 with its lower-triangular
// mask).  This is what a training step of the DecoderOnlyTransformer differentiates.
//
// The three kernels are the fp32-MFMA flash kernels of attention_bwd.hip -- 64 own rows per work-group as MFMA columns, 32-row streamed tiles
// in fp32 LDS, v_mfma_f32_16x16x4_f32, fp32 / bf16 storage, head dims 16 .. 256 (256 in two channel slices), no atomics -- with two changes:
//   * the mask: a masked probability is EXACTLY 0, by a select (`ok ? expf(...) : 0.f`), never by -inf arithmetic on the score;
//   * the walk: a work-group streams only the tiles that hold a visible (query, key) pair for its own rows (attn_bwd_causal_walk.h; bounds
//     from blockIdx alone, because the loop body synchronises the work-group).  About half the tiles of a square problem.
//   attn_bwd_causal_pre   own rows = queries: LSE[q] over the VISIBLE keys, and Dsum[q] = dO[q] . O[q]  (the forward keeps no log-sum-exp for
//                         causal launches -- attention_dma.hip declines them -- so this sweep always runs)
//   attn_bwd_causal_dq    own rows = queries: key tiles [0, key_end)
//   attn_bwd_causal_dkv   own rows = keys:    query tiles [query_begin, Lq)
#include "attn_bwd_tiles.h"
#include "attn_bwd_causal_walk.h"

static_assert(ABC_TILE == AB_ROWS, "the walk's tile is the streamed tile of attn_bwd_tiles.h");

// ---- LSE over the visible keys and Dsum ---------------------------------------------------------------------------------------------
template <typename T, int DH>
__global__ __launch_bounds__(256) void attn_bwd_causal_pre_kernel(const GmAttnBwdDesc p, float* __restrict__ lse, float* __restrict__ dsum) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ldsK = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, qg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int off = p.Lk - p.Lq;
  const int my_q = blockIdx.x * ABC_OWN + wave * 16 + l15;
  const bool q_ok = my_q < p.Lq;
  const T* Qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.Lq * p.q_ld + h * p.dh;
  const T* Kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.Lk * p.k_ld + h * p.dh;
  float4 qf[DH / 16];
  ab_load_own<T, DH>(Qb + (long long)(q_ok ? my_q : 0) * p.q_ld, q_ok, qf, qg);
  // Key 0 is visible to every query (off >= 0) and lies in the first tile, and the tile maximum below is taken over the four lanes of a query:
  // m_run is finite after the first tile, so exp(m_run - m_new) never sees inf - inf.  (Before it, l_run = 0 and exp(-inf - finite) = 0.)
  float m_run = -INFINITY, l_run = 0.f;
  const int key_end = abc_key_end(p.Lq, p.Lk, blockIdx.x);  // uniform over the work-group
  for (int key0 = 0; key0 < key_end; key0 += AB_ROWS) {
    __syncthreads();
    ab_stage<T, DH>(Kb, p.k_ld, key0, p.Lk, ldsK, tid);
    __syncthreads();
    f32x4_t s[2] = {(f32x4_t){0.f, 0.f, 0.f, 0.f}, (f32x4_t){0.f, 0.f, 0.f, 0.f}};
    ab_rows_dot<DH>(ldsK, qf, s, l15, qg);
    float tmax = -INFINITY;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + f * 16 + qg * 4 + r;
        s[f][r] *= p.scale;
        if (key < p.Lk && key <= my_q + off) tmax = fmaxf(tmax, s[f][r]);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    float psum = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + f * 16 + qg * 4 + r;
        psum += (key < p.Lk && key <= my_q + off) ? expf(s[f][r] - m_new) : 0.f;
      }
    l_run = l_run * expf(m_run - m_new) + psum;
    m_run = m_new;
  }
  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  // Dsum: this lane's channels of dO . O, then over the four lanes of the query
  const T* Ob = reinterpret_cast<const T*>(p.o) + ((long long)b * p.Lq + (q_ok ? my_q : 0)) * p.o_ld + h * p.dh;
  const T* Gb = reinterpret_cast<const T*>(p.go) + ((long long)b * p.Lq + (q_ok ? my_q : 0)) * p.go_ld + h * p.dh;
  float dot = 0.f;
  if (q_ok) {
#pragma unroll
    for (int s = 0; s < DH / 16; ++s) {
      const float4 a = ab_load4<T>(Ob + s * 16 + qg * 4), g = ab_load4<T>(Gb + s * 16 + qg * 4);
      dot += a.x * g.x + a.y * g.y + a.z * g.z + a.w * g.w;
    }
  }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
  if (q_ok && qg == 0) {
    lse[(long long)bh * p.Lq + my_q] = m_run + logf(l_tot);
    dsum[(long long)bh * p.Lq + my_q] = dot;
  }
}

// ---- dQ ---------------------------------------------------------------------------------------------------------------------------
// CS: the head dim is covered in CS channel slices (blockIdx.z) of DH / CS accumulated channels each (register budget at d = 256)
template <typename T, int DH, int CS>
__global__ __launch_bounds__(256) void attn_bwd_causal_dq_kernel(const GmAttnBwdDesc p, const float* __restrict__ lse, const float* __restrict__ dsum) {
  constexpr int DF = DH / CS / 16, PITCH = DH + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ldsK = reinterpret_cast<float*>(smem);
  float* ldsV = ldsK + AB_ROWS * PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, qg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int c0 = blockIdx.z * (DH / CS);
  const int off = p.Lk - p.Lq;
  const int my_q = blockIdx.x * ABC_OWN + wave * 16 + l15;
  const bool q_ok = my_q < p.Lq;
  const long long qrow = (long long)b * p.Lq + (q_ok ? my_q : 0);
  const T* Kb = reinterpret_cast<const T*>(p.k) + (long long)b * p.Lk * p.k_ld + h * p.dh;
  const T* Vb = reinterpret_cast<const T*>(p.v) + (long long)b * p.Lk * p.v_ld + h * p.dh;
  float4 qf[DH / 16], gf[DH / 16];
  ab_load_own<T, DH>(reinterpret_cast<const T*>(p.q) + qrow * p.q_ld + h * p.dh, q_ok, qf, qg);
  ab_load_own<T, DH>(reinterpret_cast<const T*>(p.go) + qrow * p.go_ld + h * p.dh, q_ok, gf, qg);
  const float my_lse = q_ok ? lse[(long long)bh * p.Lq + my_q] : 0.f;
  const float my_d = q_ok ? dsum[(long long)bh * p.Lq + my_q] : 0.f;
  f32x4_t acc[DF];
#pragma unroll
  for (int d = 0; d < DF; ++d) acc[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  const int key_end = abc_key_end(p.Lq, p.Lk, blockIdx.x);  // uniform over the work-group
  for (int key0 = 0; key0 < key_end; key0 += AB_ROWS) {
    __syncthreads();
    ab_stage<T, DH>(Kb, p.k_ld, key0, p.Lk, ldsK, tid);
    ab_stage<T, DH>(Vb, p.v_ld, key0, p.Lk, ldsV, tid);
    __syncthreads();
    f32x4_t s[2] = {(f32x4_t){0.f, 0.f, 0.f, 0.f}, (f32x4_t){0.f, 0.f, 0.f, 0.f}}, dp[2] = {s[0], s[0]};
    ab_rows_dot<DH>(ldsK, qf, s, l15, qg);   // S^T  = K Q^T
    ab_rows_dot<DH>(ldsV, gf, dp, l15, qg);  // dP^T = V dO^T
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + f * 16 + qg * 4 + r;
        const bool ok = q_ok && key < p.Lk && key <= my_q + off;
        const float pr = ok ? expf(s[f][r] * p.scale - my_lse) : 0.f;
        s[f][r] = pr * (dp[f][r] - my_d) * p.scale;  // dS^T
      }
    ab_cols_acc<DH, DF>(ldsK, s, acc, c0, l15, qg);  // dQ^T += K^T dS^T
  }
  if (!q_ok) return;
  T* out = reinterpret_cast<T*>(p.dq) + qrow * p.dq_ld + h * p.dh + c0;
#pragma unroll
  for (int d = 0; d < DF; ++d) ab_store4<T>(out + d * 16 + qg * 4, acc[d][0], acc[d][1], acc[d][2], acc[d][3]);
}

// ---- dK, dV ---------------------------------------------------------------------------------------------------------------------
template <typename T, int DH, int CS>
__global__ __launch_bounds__(256) void attn_bwd_causal_dkv_kernel(const GmAttnBwdDesc p, const float* __restrict__ lse, const float* __restrict__ dsum) {
  constexpr int DF = DH / CS / 16, PITCH = DH + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ldsQ = reinterpret_cast<float*>(smem);
  float* ldsG = ldsQ + AB_ROWS * PITCH;
  float* ldsL = ldsG + AB_ROWS * PITCH;  // [AB_ROWS] lse, then [AB_ROWS] dsum
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, qg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int c0 = blockIdx.z * (DH / CS);
  const int off = p.Lk - p.Lq;
  const int my_k = blockIdx.x * ABC_OWN + wave * 16 + l15;
  const bool k_ok = my_k < p.Lk;
  const long long krow = (long long)b * p.Lk + (k_ok ? my_k : 0);
  const T* Qb = reinterpret_cast<const T*>(p.q) + (long long)b * p.Lq * p.q_ld + h * p.dh;
  const T* Gb = reinterpret_cast<const T*>(p.go) + (long long)b * p.Lq * p.go_ld + h * p.dh;
  float4 kf[DH / 16], vf[DH / 16];
  ab_load_own<T, DH>(reinterpret_cast<const T*>(p.k) + krow * p.k_ld + h * p.dh, k_ok, kf, qg);
  ab_load_own<T, DH>(reinterpret_cast<const T*>(p.v) + krow * p.v_ld + h * p.dh, k_ok, vf, qg);
  f32x4_t dka[DF], dva[DF];
#pragma unroll
  for (int d = 0; d < DF; ++d) { dka[d] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; dva[d] = dka[d]; }
  const int q_begin = abc_query_begin(p.Lq, p.Lk, blockIdx.x);  // uniform over the work-group
  for (int q0 = q_begin; q0 < p.Lq; q0 += AB_ROWS) {
    __syncthreads();
    ab_stage<T, DH>(Qb, p.q_ld, q0, p.Lq, ldsQ, tid);
    ab_stage<T, DH>(Gb, p.go_ld, q0, p.Lq, ldsG, tid);
    if (tid < AB_ROWS) {
      const bool ok = q0 + tid < p.Lq;  // rows past the sequence are masked below: their entries only have to be finite
      ldsL[tid] = ok ? lse[(long long)bh * p.Lq + q0 + tid] : 0.f;
      ldsL[AB_ROWS + tid] = ok ? dsum[(long long)bh * p.Lq + q0 + tid] : 0.f;
    }
    __syncthreads();
    f32x4_t s[2] = {(f32x4_t){0.f, 0.f, 0.f, 0.f}, (f32x4_t){0.f, 0.f, 0.f, 0.f}}, dp[2] = {s[0], s[0]};
    ab_rows_dot<DH>(ldsQ, kf, s, l15, qg);   // S  = Q K^T   (rows: queries of the tile, column: this lane's key)
    ab_rows_dot<DH>(ldsG, vf, dp, l15, qg);  // dP = dO V^T
    f32x4_t pm[2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = f * 16 + qg * 4 + r, qi = q0 + row;
        const bool ok = k_ok && qi < p.Lq && my_k <= qi + off;
        const float pr = ok ? expf(s[f][r] * p.scale - ldsL[row]) : 0.f;
        pm[f][r] = pr;
        s[f][r] = pr * (dp[f][r] - ldsL[AB_ROWS + row]) * p.scale;  // dS
      }
    ab_cols_acc<DH, DF>(ldsG, pm, dva, c0, l15, qg);  // dV^T += dO^T P
    ab_cols_acc<DH, DF>(ldsQ, s, dka, c0, l15, qg);   // dK^T += Q^T dS
  }
  if (!k_ok) return;
  T* ok_ = reinterpret_cast<T*>(p.dk) + krow * p.dk_ld + h * p.dh + c0;
  T* ov_ = reinterpret_cast<T*>(p.dv) + krow * p.dv_ld + h * p.dh + c0;
#pragma unroll
  for (int d = 0; d < DF; ++d) {
    ab_store4<T>(ok_ + d * 16 + qg * 4, dka[d][0], dka[d][1], dka[d][2], dka[d][3]);
    ab_store4<T>(ov_ + d * 16 + qg * 4, dva[d][0], dva[d][1], dva[d][2], dva[d][3]);
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// block: index of a 64-row work-group on either side.  key_end: the key tiles [0, key_end) the work-group owning queries [64 block, ...) streams
// (0 when it owns no query); query_begin: the query tiles [query_begin, Lq) the work-group owning keys [64 block, ...) streams (Lq when it owns
// no key).  Pure host arithmetic over attn_bwd_causal_walk.h, the functions the kernels call; -1 (and no error text, like the other planners) for
// arguments outside 0 < Lq <= Lk, 0 <= block.
extern "C" int gm_attention_backward_causal_walk(int Lq, int Lk, int block, int* key_end, int* query_begin) {
  if (!key_end || !query_begin || Lq <= 0 || Lk < Lq || block < 0 || block > (1 << 24)) return -1;
  *key_end = (long long)ABC_OWN * block < Lq ? abc_key_end(Lq, Lk, block) : 0;
  *query_begin = (long long)ABC_OWN * block < Lk ? abc_query_begin(Lq, Lk, block) : Lq;
  return 0;
}

extern "C" long long gm_attention_backward_causal_workspace_bytes(const GmAttnBwdDesc* d) {
  if (!d) return -1;
  return 2LL * d->B * d->H * d->Lq * (long long)sizeof(float);  // LSE and dO.O per query
}

template <typename KernT>
static void abc_set_lds(KernT kern) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) (void)hipGetLastError();
}

template <typename T, int DH, int CS>
static void launch_attn_bwd_causal(const GmAttnBwdDesc& d, hipStream_t st) {
  float* lse = reinterpret_cast<float*>(d.workspace);
  float* dsum = lse + (long long)d.B * d.H * d.Lq;
  constexpr size_t tile = (size_t)AB_ROWS * (DH + 4) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    abc_set_lds(attn_bwd_causal_pre_kernel<T, DH>);
    abc_set_lds(attn_bwd_causal_dq_kernel<T, DH, CS>);
    abc_set_lds(attn_bwd_causal_dkv_kernel<T, DH, CS>);
    attr_set = true;
  }
  const int qblocks = (d.Lq + ABC_OWN - 1) / ABC_OWN, kblocks = (d.Lk + ABC_OWN - 1) / ABC_OWN;
  attn_bwd_causal_pre_kernel<T, DH><<<dim3(qblocks, d.B * d.H), 256, tile, st>>>(d, lse, dsum);
  attn_bwd_causal_dq_kernel<T, DH, CS><<<dim3(qblocks, d.B * d.H, CS), 256, 2 * tile, st>>>(d, lse, dsum);
  attn_bwd_causal_dkv_kernel<T, DH, CS><<<dim3(kblocks, d.B * d.H, CS), 256, 2 * tile + 2 * AB_ROWS * sizeof(float), st>>>(d, lse, dsum);
}

template <typename T>
static int dispatch_attn_bwd_causal(const GmAttnBwdDesc& d, hipStream_t st) {
  switch (d.dh) {
    case 16: launch_attn_bwd_causal<T, 16, 1>(d, st); return 0;
    case 32: launch_attn_bwd_causal<T, 32, 1>(d, st); return 0;
    case 64: launch_attn_bwd_causal<T, 64, 1>(d, st); return 0;
    case 128: launch_attn_bwd_causal<T, 128, 1>(d, st); return 0;
    case 256: launch_attn_bwd_causal<T, 256, 2>(d, st); return 0;
    default: return -1;
  }
}

extern "C" int gm_attention_backward_causal(const GmAttnBwdDesc* dp, void* stream) {
  GM_REQUIRE(dp, "null descriptor");
  const GmAttnBwdDesc& d = *dp;
  GM_REQUIRE(d.q && d.k && d.v && d.o && d.go && d.dq && d.dk && d.dv, "null tensor pointer");
  GM_REQUIRE(d.B >= 0 && d.H > 0 && d.Lk > 0 && d.Lq >= 0, "bad batch / head geometry");
  GM_REQUIRE(d.Lk >= d.Lq, "causal attention needs at least as many keys as queries");
  GM_REQUIRE((long long)d.B * d.H <= 65535, "too many (batch, head) pairs for one launch");
  GM_REQUIRE(d.workspace && d.workspace_bytes >= gm_attention_backward_causal_workspace_bytes(dp), "workspace too small");
  const int al = d.dtype == GM_F32 ? 16 : 8;  // rows are read and written as 4-element vectors (16 / 8 bytes)
  auto ok = [&](const void* p, long long ld) { return ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & (al - 1)) == 0; };
  GM_REQUIRE(ok(d.q, d.q_ld) && ok(d.k, d.k_ld) && ok(d.v, d.v_ld) && ok(d.o, d.o_ld) && ok(d.go, d.go_ld) && ok(d.dq, d.dq_ld) &&
                 ok(d.dk, d.dk_ld) && ok(d.dv, d.dv_ld), "operands must be 4-element aligned rows");
  if (d.B == 0 || d.Lq == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if (d.dtype == GM_F32) rc = dispatch_attn_bwd_causal<float>(d, st);
  else if (d.dtype == GM_BF16) rc = dispatch_attn_bwd_causal<bf16_raw>(d, st);
  else GM_FAIL(-2, "unsupported dtype");
  GM_REQUIRE(rc == 0, "head dim must be 16, 32, 64, 128 or 256");
  GM_LAUNCH_CHECK();
}
