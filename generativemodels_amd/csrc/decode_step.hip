// One autoregressive decoding step of the decoder-only transformer, issued from native code.
//
// A token step was 62 tiny launches in round 2 (per block: LayerNorm + stacked q|k|v GEMM writing k, v into the KV caches, 1 x t attention, out_proj +
// residual, LayerNorm + MLP up + GELU, MLP down + residual).  Issued one by one through the Python binding it cost 2.7 ms per token
// (20 us of interpreter + descriptor work per launch) -- no faster than the reference's recompute-the-prefix loop on this model
// size.  This entry point walks the block table in C++ and enqueues the kernels back to back.  Round 3: 38 launches where the fused kernels of
// rows_gemm.hip and decode_attention.hip take the geometry -- per block [LayerNorm + q|k|v + split-KV attention ranges, its prologue assembling the residual stream from
// the previous block's MLP partials] -> [out_proj + residual, its prologue merging the attention ranges] -> [LayerNorm + MLP up + GELU + MLP down
// as K-slice partials] -- and the round-2 sequence (or a partly fused one) otherwise
// (reference semantics: networks/nets/transformer.py:98-106, blocks/transformerblock.py:86-91, blocks/selfattention.py:98-147).
// Cross attention (GmDecodeDesc.ctx_len > 0; until then such models were decoded op by op from Python, re-projecting the whole context through to_k / to_v
// for every token): between the out-projection and the MLP every block adds out_proj(softmax(scale q Kc^T) Vc), q = to_q(LayerNorm2(x)), over context keys /
// values the caller projected ONCE per cache.  Two added launches per block where the fused kernel of decode_attention.hip takes the geometry
// ([LayerNorm2 + q + 1 x Lc attention] -> [out_proj + residual]), three otherwise ([LayerNorm2 + q GEMM] -> [gm_attention_forward, one query] ->
// [out_proj + residual]): gm_decode_cross_route.  The stage reads the stream from x1 and leaves it in x0, after which the two buffers swap roles.
#include <cstdlib>
#include <utility>
#include "attn_common.h"
#include "conv_common.h"

static long long elt(int dtype) { return dtype == GM_F32 ? 4 : 2; }
// Context windows longer than DECODE_SPLIT_MIN_LEN keys run the single-query attention split over DECODE_KV_SPLITS key ranges (decode_attention.hip).
// The choice depends on the window (max_len), not on the position, so a step issued with a host position and its graph replay agree bit for bit.
#define DECODE_KV_SPLITS GM_DECODE_KV_SPLITS
#define DECODE_SPLIT_MIN_LEN 256

extern "C" long long gm_decode_scratch_bytes(int B, int C, int M, int dtype) {
  // x0, x1, h, y: B*C each; qkv: 3*B*C; a: B*M; split-KV attention partials: B * heads * DECODE_KV_SPLITS * (dh + 2) floats, bounded
  // without the head count by B * DECODE_KV_SPLITS * 3 * C (heads <= C); every buffer rounded up to 256 bytes
  auto r = [](long long v) { return (v + 255) / 256 * 256; };
  return 4 * r((long long)B * C * elt(dtype)) + r(3LL * B * C * elt(dtype)) + r((long long)B * M * elt(dtype)) +
         r((long long)B * DECODE_KV_SPLITS * 3 * C * 4) + r((long long)((M + 63) / 64) * B * C * 4);  // + the MLP's K-slice partials
}

// y[rows][cout] = act(x[rows][cin] W^T + b) (+ res) through the row GEMM (rows_gemm.hip), with the fused prologue / epilogue `f` describes (null: none)
static int linear_rows(const void* x, long long x_ld, const void* w, const float* b, const void* res, long long res_ld, void* y, long long y_ld,
                       int rows, int cin, int cout, int post_act, int dtype, const GmRowsFused* f, void* stream) {
  GmRowsDesc r = {};
  r.x = x; r.x_ld = x_ld; r.w = w; r.bias = b; r.res = res; r.res_ld = res_ld; r.y = y; r.y_ld = y_ld;
  r.rows = rows; r.cin = cin; r.cout = cout; r.post_act = post_act; r.dtype = dtype;
  return gm_rows_gemm_fused(&r, f, stream);
}

// ---- the route plan ---------------------------------------------------------------------------------------------------------------------
// Every route decision of the step, taken in ONE place: block `blk`'s routes (and the step-wide ones) as GM_DECODE_PLAN_COUNT ints, indexed
// by the GM_DECODE_PLAN_* names of include/gm_amd.h.  gm_transformer_decode_step consults it per block; gm_transformer_decode_plan exports it.
// The decisions depend on the geometry, the dtype, null-ness of pointers and host-or-device position only -- never on the position itself.
static bool decode_mlp_fused(const GmDecodeDesc& d) {
  // the MLP as one launch leaving M / 64 K-slice partials that the next launch's prologue sums with the residual row (rows_gemm.hip)
  bool mlp_fuse = gm_mlp_rows_fusable(d.B, d.C, d.M, d.dtype) == 1;
  for (int i = 0; i < d.depth; ++i) mlp_fuse = mlp_fuse && d.blocks[i].ln3_g;  // (its staging pass is the LayerNorm)
  return mlp_fuse;
}

// the fused q|k|v + attention kernel's arguments for block `blk` (everything but the position), as the step passes them
static QkvAttnArgs decode_qkv_args(const GmDecodeDesc& d, int blk, bool mlp_fuse, char* x0, char* x1, float* mlp_p, float* kv_ws) {
  const GmDecodeBlock& b = d.blocks[blk];
  QkvAttnArgs qa = {};
  if (mlp_fuse && blk > 0) { qa.mlp_p = mlp_p; qa.mlp_nj = d.M / 64; qa.mlp_x1 = x1; qa.mlp_b2 = d.blocks[blk - 1].b_2; qa.x0_out = x0; }
  else qa.x0 = x0;
  qa.ln_g = b.ln1_g; qa.ln_b = b.ln1_b; qa.ln_eps = d.ln_eps;
  qa.w = b.w_qkv; qa.bias = b.b_qkv;
  qa.kcache = b.k_cache; qa.vcache = b.v_cache;
  qa.B = d.B; qa.H = d.heads; qa.C = d.C; qa.dh = d.C / d.heads; qa.cap = d.max_len; qa.pos_dev = d.pos_dev;
  qa.scale = 1.0f / sqrtf((float)(d.C / d.heads)); qa.ws = kv_ws;
  return qa;
}

static void decode_plan(const GmDecodeDesc& d, int blk, const QkvAttnArgs& qa, bool mlp_fuse, int* f) {
  static const bool kv_split = !(getenv("GM_DECODE_KV_SPLIT") && getenv("GM_DECODE_KV_SPLIT")[0] == '0');  // bench switches (tools/diag_c5.py)
  static const bool kv_fuse = !(getenv("GM_DECODE_KV_FUSE") && getenv("GM_DECODE_KV_FUSE")[0] == '0');
  for (int i = 0; i < GM_DECODE_PLAN_COUNT; ++i) f[i] = 0;
  const int dh = d.C / d.heads;
  const bool split = kv_split && d.max_len > DECODE_SPLIT_MIN_LEN;
  const bool ks_c = gm_linear_rows_takes_ksplit(d.B, d.C, d.dtype) == 1, ks_m = gm_linear_rows_takes_ksplit(d.B, d.M, d.dtype) == 1;
  f[GM_DECODE_PLAN_SPLIT_KV] = split;
  // LayerNorm + q | k | v + the attention ranges as one launch where that kernel takes the geometry (split windows only)
  int ng = 0, um = 0;
  const bool qkv_fused = split && gm_qkv_attn_rows_plan(&qa, d.dtype, &ng, &um) == 1;
  f[GM_DECODE_PLAN_QKV_NG] = qkv_fused ? ng : 0;
  f[GM_DECODE_PLAN_QKV_UM] = qkv_fused ? um : 0;
  // behind a fused MLP the q|k|v launch (fused or GEMM) assembles its input from the previous block's partials
  f[GM_DECODE_PLAN_QKV_INPUT] = mlp_fuse && blk > 0 ? GM_DECODE_INPUT_MLP_MERGE : GM_DECODE_INPUT_ROW;
  // the partials are merged by the out-projection's prologue where its K-split kernel applies, by a combine launch otherwise: the two
  // forms give the same bits, and which one runs depends on the geometry only
  f[GM_DECODE_PLAN_OUT_MERGE] = !split ? GM_DECODE_MERGE_NONE
                                : kv_fuse && dh % (d.dtype == GM_F32 ? 4 : 8) == 0 && d.C % dh == 0 && ks_c ? GM_DECODE_MERGE_OUT_PROJ : GM_DECODE_MERGE_COMBINE;
  f[GM_DECODE_PLAN_ATTN_ENTRY] = split ? GM_DECODE_ENTRY_NONE : d.pos_dev ? GM_DECODE_ENTRY_DEVICE_POS : GM_DECODE_ENTRY_HOST_POS;
  f[GM_DECODE_PLAN_MLP_FUSED] = mlp_fuse;
  f[GM_DECODE_PLAN_KSPLIT_QKV] = !qkv_fused && ks_c;  // (the fused kernel replaces the GEMM)
  f[GM_DECODE_PLAN_KSPLIT_OUT] = ks_c;
  f[GM_DECODE_PLAN_KSPLIT_MLP_UP] = !mlp_fuse && ks_c;  // (the fused MLP kernel replaces both GEMMs)
  f[GM_DECODE_PLAN_KSPLIT_MLP_DOWN] = !mlp_fuse && ks_m;
  f[GM_DECODE_PLAN_KSPLIT_LOGITS] = ks_c;
}

// ---- the cross-attention stage -------------------------------------------------------------------------------------------------------------
// the fused kernel's arguments for block `blk`: the stream row `x` in, the attention output `o` (before the out-projection) out
static CrossAttnArgs decode_cross_args(const GmDecodeDesc& d, int blk, const void* x, void* o) {
  const GmDecodeBlock& b = d.blocks[blk];
  CrossAttnArgs ca = {};
  ca.x = x; ca.ln_g = b.ln2_g; ca.ln_b = b.ln2_b; ca.ln_eps = d.ln_eps;
  ca.w = b.w_cq; ca.bias = b.b_cq; ca.ck = b.ck; ca.cv = b.cv; ca.o = o;
  ca.B = d.B; ca.H = d.heads; ca.C = d.C; ca.dh = d.C / d.heads; ca.Lc = d.ctx_len;
  ca.scale = 1.0f / sqrtf((float)(d.C / d.heads));
  return ca;
}

// Host only: GM_DECODE_CROSS_* for `dp`, from the geometry and the dtype alone (the same for every block), or a negative error.
extern "C" int gm_decode_cross_route(const GmDecodeDesc* dp) {
  GM_REQUIRE(dp, "null descriptor");
  const GmDecodeDesc& d = *dp;
  GM_REQUIRE(d.ctx_len >= 0, "negative context length");
  if (d.ctx_len == 0) return GM_DECODE_CROSS_NONE;
  GM_REQUIRE(d.B > 0 && d.C > 0 && d.heads > 0 && d.C % d.heads == 0 && d.depth > 0 && d.blocks, "bad geometry");
  for (int i = 0; i < d.depth; ++i) {
    const GmDecodeBlock& b = d.blocks[i];
    GM_REQUIRE(b.ln2_g && b.w_cq && b.w_co && b.ck && b.cv, "null cross-attention pointer in a block (ctx_len > 0)");
  }
  const CrossAttnArgs ca = decode_cross_args(d, 0, nullptr, nullptr);
  int ng = 0, um = 0;
  // (more than 16 rows: the out-projection behind the kernel leaves the K-split GEMM, and B * heads work-groups stop being a handful)
  return d.B <= 16 && gm_cross_attn_rows_plan(&ca, d.dtype, &ng, &um) == 1 ? GM_DECODE_CROSS_FUSED : GM_DECODE_CROSS_COMPOSED;
}

// the descriptor checks shared by the step and its plan (a macro: a failure names the entry point that was called)
#define GM_DECODE_CHECK(dp)                                                                                                               \
  do {                                                                                                                                    \
    GM_REQUIRE(dp, "null descriptor");                                                                                                    \
    GM_REQUIRE(dp->tokens && dp->tok_emb && dp->pos_emb && dp->blocks && dp->w_logits && dp->logits && dp->scratch, "null pointer");      \
    GM_REQUIRE(dp->B > 0 && dp->C > 0 && dp->M > 0 && dp->heads > 0 && dp->C % dp->heads == 0 && dp->depth > 0, "bad geometry");           \
    GM_REQUIRE(dp->pos_dev || (dp->pos >= 0 && dp->pos < dp->max_len), "position outside the context window");                            \
    GM_REQUIRE(dp->scratch_bytes >= gm_decode_scratch_bytes(dp->B, dp->C, dp->M, dp->dtype), "scratch too small");                        \
  } while (0)

struct DecodeScratch { char *x0, *x1, *h, *y, *qkv, *a; float *kv_ws, *mlp_p; };
static DecodeScratch decode_scratch(const GmDecodeDesc& d) {
  const long long es = elt(d.dtype);
  auto r = [](long long v) { return (v + 255) / 256 * 256; };
  DecodeScratch w;
  char* s = reinterpret_cast<char*>(d.scratch);
  w.x0 = s;  s += r((long long)d.B * d.C * es);
  w.x1 = s;  s += r((long long)d.B * d.C * es);
  w.h = s;   s += r((long long)d.B * d.C * es);
  w.y = s;   s += r((long long)d.B * d.C * es);
  w.qkv = s; s += r(3LL * d.B * d.C * es);
  w.a = s;   s += r((long long)d.B * d.M * es);
  w.kv_ws = reinterpret_cast<float*>(s); s += r((long long)d.B * DECODE_KV_SPLITS * 3 * d.C * 4);
  w.mlp_p = reinterpret_cast<float*>(s);
  return w;
}

// The plan of the step `dp` describes, launching nothing: flags[GM_DECODE_PLAN_COUNT].  The per-block entries are those of the last block
// (with depth >= 2 that is the steady state: block 0 alone has no MLP partials in front of it and always takes the plain row).
extern "C" int gm_transformer_decode_plan(const GmDecodeDesc* dp, int* flags) {
  GM_REQUIRE(flags, "null pointer");
  GM_DECODE_CHECK(dp);
  const GmDecodeDesc& d = *dp;
  const DecodeScratch w = decode_scratch(d);
  const bool mlp_fuse = decode_mlp_fused(d);
  const int blk = d.depth - 1;
  const QkvAttnArgs qa = decode_qkv_args(d, blk, mlp_fuse, w.x0, w.x1, w.mlp_p, w.kv_ws);
  decode_plan(d, blk, qa, mlp_fuse, flags);
  return 0;
}

extern "C" int gm_transformer_decode_step(const GmDecodeDesc* dp, void* stream) {
  GM_DECODE_CHECK(dp);
  const int cross = gm_decode_cross_route(dp);  // (validates the cross fields of ALL blocks before the first launch)
  if (cross < 0) return cross;
  const GmDecodeDesc& d = *dp;
  const int hpos = d.pos_dev ? 0 : d.pos;  // host-side position (0 when the device supplies it)
  const long long es = elt(d.dtype);
  const DecodeScratch w = decode_scratch(d);
  char *x0 = w.x0, *x1 = w.x1, *y = w.y, *qkv = w.qkv, *a = w.a;
  float *kv_ws = w.kv_ws, *mlp_p = w.mlp_p;
  const bool mlp_fuse = decode_mlp_fused(d);
  const int mlp_nj = d.M / 64;
  const int C = d.C;
  int rc = gm_embed_tokens_dev(d.tokens, d.tok_emb, d.pos_emb, x0, d.B, 1, C, hpos, d.num_tokens, d.max_len, d.dtype, d.pos_dev, stream);
  if (rc) return rc;
  const float scale = 1.0f / sqrtf((float)(C / d.heads));
  for (int i = 0; i < d.depth; ++i) {
    const GmDecodeBlock& b = d.blocks[i];
    GM_REQUIRE(b.w_qkv && b.w_o && b.w_1 && b.w_2 && b.k_cache && b.v_cache, "null block parameter");
    QkvAttnArgs qa = decode_qkv_args(d, i, mlp_fuse, x0, x1, mlp_p, kv_ws);
    int plan[GM_DECODE_PLAN_COUNT];
    decode_plan(d, i, qa, mlp_fuse, plan);
    const bool split = plan[GM_DECODE_PLAN_SPLIT_KV] != 0;
    // LayerNorm + q | k | v + the attention ranges as ONE launch where that kernel takes the geometry (decode_attention.hip: qkv_attn_rows_kernel) ...
    bool qkv_done = false;
    if (plan[GM_DECODE_PLAN_QKV_NG]) {
      qa.pos = hpos;
      rc = gm_qkv_attn_rows(&qa, d.dtype, stream);
      if (rc < 0) return rc;
      GM_REQUIRE(rc == 1, "the fused q|k|v + attention launch disagrees with the plan");
      qkv_done = true;
    }
    // ... otherwise LayerNorm + stacked q | k | v projection in one launch; the key / value rows land directly in cache row `pos` of every sequence.
    // Behind a fused MLP the launch first assembles its input x0 = x1 + b2 + sum_j P[j] (and stores it: the out-projection below adds it as the residual)
    char* kdst = reinterpret_cast<char*>(b.k_cache) + (long long)hpos * C * es;
    char* vdst = reinterpret_cast<char*>(b.v_cache) + (long long)hpos * C * es;
    if (!qkv_done) {
      const bool merge_in = plan[GM_DECODE_PLAN_QKV_INPUT] == GM_DECODE_INPUT_MLP_MERGE;
      GmRowsFused fz = {};
      fz.ln_g = b.ln1_g; fz.ln_b = b.ln1_b; fz.ln_eps = d.ln_eps;
      fz.y1 = kdst; fz.y2 = vdst; fz.y12_ld = (long long)d.max_len * C; fz.split = C;
      fz.off_dev = d.pos_dev; fz.off_mul = C;
      if (merge_in) { fz.mlp_p = mlp_p; fz.mlp_nj = mlp_nj; fz.mlp_x1 = x1; fz.mlp_b2 = d.blocks[i - 1].b_2; fz.mlp_x0 = x0; }
      if ((rc = linear_rows(merge_in ? nullptr : x0, merge_in ? 0 : C, b.w_qkv, b.b_qkv, nullptr, 0, qkv, 3 * C, d.B, C, 3 * C, 0, d.dtype, &fz, stream))) return rc;
    }
    GmAttnDesc at = {};
    at.q = qkv; at.q_ld = 3 * C;
    at.k = b.k_cache; at.k_ld = C; at.k_bs = (long long)d.max_len * C;
    at.v = b.v_cache; at.v_ld = C; at.v_bs = (long long)d.max_len * C;
    at.o = y; at.o_ld = C;
    at.B = d.B; at.H = d.heads; at.Lq = 1; at.Lk = d.pos_dev ? d.max_len : d.pos + 1; at.dh = C / d.heads;
    at.scale = scale; at.dtype = d.dtype;
    bool out_done = false;
    if (split) {
      // the partials are merged by the out-projection's prologue where its K-split kernel applies (the plan's decision: the launcher refuses a
      // geometry outside that kernel), by a combine launch otherwise: the two forms give the same bits, and which one runs depends on the geometry only
      if (!qkv_done)
        GM_REQUIRE(gm_attention_decode_split(&at, d.pos_dev, kv_ws, DECODE_KV_SPLITS, 0, d.max_len, stream) == 1, "head size beyond the single-query attention kernels");
      if (plan[GM_DECODE_PLAN_OUT_MERGE] == GM_DECODE_MERGE_OUT_PROJ) {
        GmRowsFused fz = {};
        fz.kv_ws = kv_ws; fz.kv_ns = DECODE_KV_SPLITS; fz.kv_dh = at.dh;
        if ((rc = linear_rows(nullptr, 0, b.w_o, b.b_o, x0, C, x1, C, d.B, C, C, 0, d.dtype, &fz, stream))) return rc;
        out_done = true;
      } else {
        GM_REQUIRE(gm_attention_decode_split(&at, d.pos_dev, kv_ws, DECODE_KV_SPLITS, 2, d.max_len, stream) == 1, "merge of the attention partials");
      }
    } else if (plan[GM_DECODE_PLAN_ATTN_ENTRY] == GM_DECODE_ENTRY_DEVICE_POS) {
      GM_REQUIRE(gm_attention_decode_dev(&at, d.pos_dev, stream) == 1, "context window too long for the single-query attention kernel");
    } else if ((rc = gm_attention_forward(&at, stream))) {
      return rc;
    }
    if (!out_done && (rc = linear_rows(y, C, b.w_o, b.b_o, x0, C, x1, C, d.B, C, C, 0, d.dtype, nullptr, stream))) return rc;
    if (cross != GM_DECODE_CROSS_NONE) {
      // the stream is in x1; x0 is dead since the out-projection above read it as its residual: the stage leaves x1 + out_proj(attention) there and
      // the two buffers swap roles, so the MLP below, the next block's prologue and to_logits find the stream where they expect it (x1)
      if (cross == GM_DECODE_CROSS_FUSED) {
        const CrossAttnArgs ca = decode_cross_args(d, i, x1, y);
        rc = gm_cross_attn_rows(&ca, d.dtype, stream);
        if (rc < 0) GM_FAIL(rc, "launch of the fused cross-attention kernel");
        GM_REQUIRE(rc == 1, "the fused cross-attention launch disagrees with the route");
      } else {
        GmRowsFused ln2 = {};
        ln2.ln_g = b.ln2_g; ln2.ln_b = b.ln2_b; ln2.ln_eps = d.ln_eps;
        if ((rc = linear_rows(x1, C, b.w_cq, b.b_cq, nullptr, 0, w.h, C, d.B, C, C, 0, d.dtype, &ln2, stream))) return rc;
        GmAttnDesc ct = {};
        ct.q = w.h; ct.q_ld = C;
        ct.k = b.ck; ct.k_ld = C; ct.k_bs = (long long)d.ctx_len * C;
        ct.v = b.cv; ct.v_ld = C; ct.v_bs = (long long)d.ctx_len * C;
        ct.o = y; ct.o_ld = C;
        ct.B = d.B; ct.H = d.heads; ct.Lq = 1; ct.Lk = d.ctx_len; ct.dh = C / d.heads;
        ct.scale = scale; ct.dtype = d.dtype;
        if ((rc = gm_attention_forward(&ct, stream))) return rc;
      }
      if ((rc = linear_rows(y, C, b.w_co, b.b_co, x1, C, x0, C, d.B, C, C, 0, d.dtype, nullptr, stream))) return rc;
      std::swap(x0, x1);
    }
    if (mlp_fuse) {
      if ((rc = gm_mlp_rows(x1, b.ln3_g, b.ln3_b, d.ln_eps, b.w_1, b.b_1, b.w_2, mlp_p, d.B, C, d.M, 6, d.dtype, stream))) return rc;
      continue;
    }
    GmRowsFused ln3 = {};
    ln3.ln_g = b.ln3_g; ln3.ln_b = b.ln3_b; ln3.ln_eps = d.ln_eps;
    if ((rc = linear_rows(x1, C, b.w_1, b.b_1, nullptr, 0, a, d.M, d.B, C, d.M, 6, d.dtype, &ln3, stream))) return rc;
    if ((rc = linear_rows(a, d.M, b.w_2, b.b_2, x1, C, x0, C, d.B, d.M, C, 0, d.dtype, nullptr, stream))) return rc;
  }
  if (mlp_fuse) {  // to_logits assembles its input from the last block's MLP partials
    GmRowsFused fz = {};
    fz.mlp_p = mlp_p; fz.mlp_nj = mlp_nj; fz.mlp_x1 = x1; fz.mlp_b2 = d.blocks[d.depth - 1].b_2;
    return linear_rows(nullptr, 0, d.w_logits, d.b_logits, nullptr, 0, d.logits, d.num_tokens, d.B, C, d.num_tokens, 0, d.dtype, &fz, stream);
  }
  return linear_rows(x0, C, d.w_logits, d.b_logits, nullptr, 0, d.logits, d.num_tokens, d.B, C, d.num_tokens, 0, d.dtype, nullptr, stream);
}
