// Tile walk of the causal flash backward (attention_bwd.hip, CAUSAL).  Query i sees keys j <= i + off, off = Lk - Lq >= 0 (attn_common.h,
// GmAttnDesc.causal).  A work-group owns ABC_OWN consecutive rows and streams the other side in tiles of ABC_TILE rows with a
// __syncthreads() per tile, so both bounds are functions of the work-group's block index alone -- never of a lane's own row.  The kernels and
// the host entry point gm_attention_backward_causal_walk read the SAME two functions, so a host test checks the walk the kernels run.
#pragma once

#define ABC_OWN 64   // own rows of a work-group (4 waves x 16 MFMA columns)
#define ABC_TILE 32  // rows of a streamed tile (= AB_ROWS of attn_bwd_tiles.h)

#ifdef __HIPCC__
#define ABC_FN __host__ __device__ inline
#else
#define ABC_FN inline
#endif

// The work-group owning queries [ABC_OWN * block, ...) streams the key tiles that start in [0, key_end): the last of them holds the last key
// its last query sees.  (last_q + off + 1 <= Lq + off = Lk; the min() only states it.)
ABC_FN int abc_key_end(int Lq, int Lk, int block) {
  const int off = Lk - Lq;
  const int last_q = ABC_OWN * block + ABC_OWN - 1 < Lq - 1 ? ABC_OWN * block + ABC_OWN - 1 : Lq - 1;
  const int end = last_q + off + 1;
  return end < Lk ? end : Lk;
}

// The work-group owning keys [ABC_OWN * block, ...) streams the query tiles that start in [query_begin, Lq): the first of them holds the first
// query that sees its first key, query ABC_OWN * block - off.
ABC_FN int abc_query_begin(int Lq, int Lk, int block) {
  const int off = Lk - Lq;
  const int first = ABC_OWN * block - off > 0 ? ABC_OWN * block - off : 0;
  return first / ABC_TILE * ABC_TILE;
}
