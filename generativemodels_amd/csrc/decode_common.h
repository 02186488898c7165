// The one device helper the decode step's two kernel files share: the merge of the split-KV single-query attention partials, run by
// attn_decode_combine_kernel (decode_attention.hip) and by the out-projection's prologue (rows_gemm.hip: linear_rows_ksplit_kernel STAGE 1).
#pragma once
#include "attn_common.h"

// One channel of the split-KV single-query attention, merged from its GM_DECODE_KV_SPLITS partials in range order.  Workspace =
// o[BH][NS][dh], then m[BH][NS], l[BH][NS].  The split count is a compile-time constant so that all 3 NS loads are in flight at once (a
// run-time loop waits for every load in turn: 16 dependent L2 round trips, measured +22 us per call).
__device__ __forceinline__ float kv_merge_one(const float* __restrict__ ws, int BH, int dh, int bh, int c) {
  constexpr int NS = GM_DECODE_KV_SPLITS;
  const float* o = ws + (long long)bh * NS * dh + c;
  const float* m = ws + (long long)BH * NS * dh + (long long)bh * NS;
  const float* l = m + (long long)BH * NS;
  float ms[NS], ls[NS], os[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) { ms[s] = m[s]; ls[s] = l[s]; os[s] = o[(long long)s * dh]; }
  float M = -INFINITY;
#pragma unroll
  for (int s = 0; s < NS; ++s) M = fmaxf(M, ms[s]);
  float L = 0.f, acc = 0.f;
#pragma unroll
  for (int s = 0; s < NS; ++s) {  // range order
    const float e = ms[s] == -INFINITY ? 0.f : expf(ms[s] - M);
    L += ls[s] * e;
    acc += os[s] * e;
  }
  return acc * (1.0f / L);
}
