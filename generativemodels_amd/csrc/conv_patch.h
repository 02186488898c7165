// Patch staging of the small-grid LDS-DMA convolutions (conv_sk.hip: the K slices of a split cfg 11 launch; conv_sn.hip: cfg 24 / 25): the work item of a
// work-group, the placement of a lane's patch rows, the requests of a K chunk, the GroupNorm-apply + activation prologue in LDS and the operand read addresses
// of a tap.  conv_dma.hip shares the layouts but not this code: its tile loop is hand-balanced against the register budget (OPAQUE_LANE, cold_desc, PVOX_LDS).
#pragma once
#include "conv_dma_shared.h"

// The patch of a tile: PROWS rows of 64 bytes (one K chunk of one voxel each), planes of PH x PW rows at a pitch of PLANE rows (padded so that depth offsets keep
// row mod 16); NW waves move it in PPIECES pieces of 16 rows, piece i by wave i % NW.
template <int NW_, int PLANE_, int PW_, int PH_, int PROWS_> struct PatchGeom {
  static constexpr int NW = NW_, PLANE = PLANE_, PW = PW_, PH = PH_, PROWS = PROWS_;
  static constexpr int PPIECES = PROWS / 16, PPW = (PPIECES + NW - 1) / NW;
};

// The work item of work-group `wg` out of `nwork`: XCD x (= wg & 7: consecutive work-groups go to consecutive XCDs) owns a contiguous range of items, so that
// neighbouring items -- the channel blocks of a tile, the K slices of a channel block -- meet in one L2.  PATCH_NO_ITEM: the XCD's range is shorter than wg >> 3.
constexpr unsigned PATCH_NO_ITEM = ~0u;
__device__ __forceinline__ unsigned patch_work_item(unsigned nwork, unsigned wg) {
  const unsigned xcd = wg & 7, pos = wg >> 3;
  const unsigned q8 = nwork >> 3, r8 = nwork & 7, cx = q8 + (xcd < r8 ? 1u : 0u), sx = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  return pos < cx ? sx + pos : PATCH_NO_ITEM;
}

// The patch rows of this lane: row 16 (wave + NW j) + lane / 4 of piece j -> its source voxel in pvox[j] (-1: padding, or a pad row of the plane pitch) and the
// bank-swizzle key of its column within the W line in bits 2j, 2j + 1 of psw.  The swizzle is applied on the SOURCE side (lane l of a row fetches 16-byte slot
// (l & 3) ^ key): an LDS-DMA piece lands as 64 lanes x 16 consecutive bytes, so the destination cannot be permuted.
// in_mode 1: the input is the nearest-neighbour up-sampling by (fd, fh, fw) of the stored tensor, never materialised (reference Upsample,
// diffusion_model_unet.py:572-585): bounds on the virtual grid, source voxel = virtual / factor.  in_mode 0 (a literal at conv_sk.hip's call): the factors are 1.
template <typename PG>
__device__ __forceinline__ void patch_place(const GmConvDesc& p, int in_mode, int n, int od0, int oh0, int ow0, int wave, int lane, int& psw, int (&pvox)[PG::PPW]) {
  psw = 0;
#pragma unroll
  for (int j = 0; j < PG::PPW; ++j) {
    const int row = 16 * (wave + PG::NW * j) + (lane >> 2);
    const int pa = row / PG::PLANE, rr = row - pa * PG::PLANE;
    const int pb = rr / PG::PW, lc = rr - pb * PG::PW;
    psw |= dma_swz(lc) << (2 * j);
    int ud = od0 - p.pd + pa, uh = oh0 - p.ph + pb, uw = ow0 - p.pw + lc;
    const int Dv = in_mode == 1 ? p.Ds * p.fd : p.Ds, Hv = in_mode == 1 ? p.Hs * p.fh : p.Hs, Wv = in_mode == 1 ? p.Ws * p.fw : p.Ws;
    const bool ok = (row < PG::PROWS) & (rr < PG::PH * PG::PW) & (ud >= 0) & (ud < Dv) & (uh >= 0) & (uh < Hv) & (uw >= 0) & (uw < Wv);
    if (in_mode == 1) { ud /= p.fd; uh /= p.fh; uw /= p.fw; }
    pvox[j] = ok ? ((n * p.Ds + ud) * p.Hs + uh) * p.Ws + uw : -1;
  }
}

// The requests of K chunk `chunk`, per wave: (arrays: the prologue's scale / shift come as GmConvDesc.pre_scale / pre_shift) the chunk's [scale | shift] into
// this wave's own LDS copy -- lanes 0 .. BK/4 - 1 fetch the scale, the next BK/4 the shift, 16 bytes each; requested AHEAD of the patch pieces, so that it
// has landed when they have (an ordinary global load would make hipcc wait for vmcnt(0) at its first use) -- then the wave's patch pieces.  Chunks from
// cin_split on come from x2 (virtual channel concatenation); padding rows come from the 64 zero bytes at `zero`.  aff_off: LDS offset of wave 0's copy.
// (The kernel's scalars come by reference and the copy's address is formed next to its use, as in the per-kernel lambdas this replaces: with by-value
// arguments hipcc allocated 2 more VGPRs or SGPR spills in some instantiations -- tools/kernel_resources.py.)
constexpr int PATCH_AFF_WAVE = 256;  // bytes of a wave's [scale | shift] copy
template <typename T, typename PG>
__device__ __forceinline__ void patch_issue(const GmConvDesc& p, const bool& arrays, int chunk, const int& n, const int (&pvox)[PG::PPW], const int& psw,
                                            const char* const& zero, const unsigned& lds0, unsigned aff_off, const int& wave, const int& lane) {
  constexpr int BK = ConvTraits<T>::BK;
  if (arrays) {
    const int nl = BK / 4;
    if (lane < 2 * nl) {
      const float* src = (lane < nl ? p.pre_scale : p.pre_shift) + (long long)n * p.Cin + chunk * BK + 4 * (lane < nl ? lane : lane - nl);
      dma16(src, lds0 + aff_off + (unsigned)wave * PATCH_AFF_WAVE);
    }
  }
  const int nchunks0 = p.x2 ? p.cin_split / BK : p.Cin / BK;
  const bool second = chunk >= nchunks0;  // wave-uniform
  const char* cbase = second ? reinterpret_cast<const char*>(p.x2) + (long long)(chunk - nchunks0) * (BK * (int)sizeof(T))
                             : reinterpret_cast<const char*>(p.x) + (long long)chunk * (BK * (int)sizeof(T));
  const long long rowb = second ? p.x2_ld * (long long)sizeof(T) : p.x_ld * (long long)sizeof(T);
#pragma unroll
  for (int j = 0; j < PG::PPW; ++j) {
    if (wave + PG::NW * j < PG::PPIECES) {  // wave-uniform
      // (both addresses computed, then selected: a conditional 64-bit multiply compiles to a branch per piece)
      const char* in_src = cbase + (long long)(pvox[j] & ~(pvox[j] >> 31)) * rowb + (((lane & 3) ^ ((psw >> (2 * j)) & 3)) << 4);
      const char* pad_src = zero + ((lane & 3) << 4);
      dma16(pvox[j] >= 0 ? in_src : pad_src, lds0 + (unsigned)(16 * (wave + PG::NW * j)) * DMA_ROWB);
    }
  }
}

// GroupNorm-apply + activation IN LDS on this wave's own landed pieces: v * scale + shift, the activation, rounded to T -- the arithmetic and rounding of
// gm_gn_apply, so the fused form equals the two-pass form bit for bit.  aff[i] / aff[shoff + i] = scale / shift of channel i of the chunk (the wave's own
// per-chunk copy, or the kernel's table built from the statistics).  Rows that came from the zero row stay zero: the reference pads the ACTIVATED tensor.
template <typename T, typename PG>
__device__ __forceinline__ void patch_transform(char* smem, const float* aff, int shoff, int pre_act, const int (&pvox)[PG::PPW], int psw, int wave, int lane) {
  constexpr int VECW = ConvTraits<T>::VECW;
  float sc[VECW], sh[VECW];
#pragma unroll
  for (int i = 0; i < VECW; i += 4) {
    const float4 a = *reinterpret_cast<const float4*>(aff + (lane & 3) * VECW + i), c = *reinterpret_cast<const float4*>(aff + shoff + (lane & 3) * VECW + i);
    sc[i] = a.x; sc[i + 1] = a.y; sc[i + 2] = a.z; sc[i + 3] = a.w;
    sh[i] = c.x; sh[i + 1] = c.y; sh[i + 2] = c.z; sh[i + 3] = c.w;
  }
#pragma unroll
  for (int j = 0; j < PG::PPW; ++j) {
    if (wave + PG::NW * j < PG::PPIECES && pvox[j] >= 0) {
      char* a = smem + (16 * (wave + PG::NW * j) + (lane >> 2)) * DMA_ROWB + (((lane & 3) ^ ((psw >> (2 * j)) & 3)) << 4);
      float v[VECW];
      Vec16<T>::unpack(*reinterpret_cast<const uint4*>(a), v);
#pragma unroll
      for (int i = 0; i < VECW; ++i) v[i] = v[i] * sc[i] + sh[i];
      conv_act_vec(v, pre_act, sizeof(T) == 4);
      *reinterpret_cast<uint4*>(a) = Vec16<T>::pack(v);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// Operand read addresses of a lane (byte offsets into the LDS block): xa[kw] = the patch row of tap column kw for the lane's voxel l15 of the W line at
// (plane, line) of the patch -- tap (kd, kh) adds kd planes and kh lines --, wa0 = row l15 of the first weight panel behind the patch; 16-byte slot q of
// either row, through the row's swizzle key.
template <int KS, typename PG>
__device__ __forceinline__ void patch_operand_addresses(int plane, int line, int l15, int q, int patch_bytes, int (&xa)[KS], int& wa0) {
#pragma unroll
  for (int kw = 0; kw < KS; ++kw) xa[kw] = (plane * PG::PLANE + line * PG::PW + l15 + kw) * DMA_ROWB + ((q ^ dma_swz(l15 + kw)) << 4);
  wa0 = patch_bytes + l15 * DMA_ROWB + ((q ^ dma_swz(l15)) << 4);
}
