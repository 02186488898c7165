// 3x3x3 stride-1 convolution with BOTH operands streamed global -> LDS by the LDS-DMA engine (global_load_lds_dwordx4): the
// prologue-free ResnetBlock / Upsample convolutions of the 3-D UNet and auto-encoders (conv_fast.hip keeps the fused-prologue,
// 1^d and 2-D cases).  What rocprof / the ISA of conv_fast showed on MI355X and what this kernel changes:
//   * register-staged prefetch does not survive hipcc: every ds_read after a prefetch `global_load` is guarded by
//     `s_waitcnt vmcnt(0)` (register re-use hazard), so the weight panel's L2 latency was exposed once per tap group and the
//     halo patch was fetched in serialised batches of two.  LDS-DMA has no destination register: all pieces of a patch are in
//     flight at once, weight panels are issued two tap groups ahead into a 3-deep ring, and the only waits are the counted
//     `s_waitcnt vmcnt(N)` written here (hipcc does not see inline-asm memory operations);
//   * 4.4 VALU + 4.4 SALU instructions per MFMA (swizzle address arithmetic, tap counters): the tile geometry is a template
//     constant, the 27 taps are fully unrolled, the patch plane pitch is padded to a multiple of 16 rows so the XOR swizzle is
//     invariant under the depth offset -- a tap's operand reads are `ds_read_b128 v, vaddr offset:imm` from 9 precomputed
//     per-lane addresses per voxel fragment: zero address arithmetic in the loop.
// LDS-DMA writes lane-linear (M0 base + lane*16), so the swizzle is applied on the SOURCE side: LDS (row, slot s) receives the
// 16-byte channel slot s ^ swz(row) of that row; out-of-volume rows (zero padding) read a zero page.
// Tile: 4x4x16 = 256 voxels x 64 channels, 8 waves (32 voxels x 64 channels each), 78 KiB LDS -> two work-groups per CU, one
// staging its patch while the other computes.
#include "conv_dma_shared.h"
#include <type_traits>

// bench-only build (-DGM_CONV_TIMELINE, tools/conv_timeline.py): thread 0 of every work-group stamps the shader clock at phase boundaries
// into GmConvDesc.kpartial (64 slots per work-group) when debug_flags bit 12 is set; compiled out of the shipped library
#ifdef GM_CONV_TIMELINE
#define TL_STAMP(k)                                                                                                              \
  do {                                                                                                                           \
    if ((p.debug_flags & 4096) && threadIdx.x == 0 && tl_on)                                                                            \
      reinterpret_cast<unsigned long long*>(p.kpartial)[(long long)blockIdx.x * 64 + (k)] = __builtin_readcyclecounter();        \
  } while (0)
#else
#define TL_STAMP(k)
#endif
// This file is compiled once per PART (-DGM_DMA_PART=k, _build.py: one object per part, in parallel -- the seven tile configurations x two dtypes x
// the prologue forms took 4.5 minutes as one translation unit): part 0 = the host entry points + cfg 11, 1 = cfg 14, 2 = cfg 15 + 17,
// 3 = cfg 16 + 18, 4 = cfg 19.  Without the define everything lands in one translation unit.
#ifndef GM_DMA_PART
#define GM_DMA_PART (-1)
#endif
#define DMA_PART(k) (GM_DMA_PART == -1 || GM_DMA_PART == (k))
static __device__ __attribute__((aligned(64))) unsigned int gm_zero_row[16] = {0};  // the source of every padding row (one per part)

// NW waves per work-group, each owning MF voxel fragments (16 voxels) x 64 channels of the 256-voxel tile: <8, 2> = 16 waves / CU,
// 0.75 LDS operand reads per MFMA; <4, 4> = 8 waves / CU with 256 VGPRs each, 0.5 reads per MFMA (the LDS port is the next limit
// after latency: 16 waves x 6 KiB per tap = 768 LDS clocks against 512 MFMA clocks per SIMD)
// S = 1: stride 1 (optionally over a 2x nearest-upsampled input), 4x4x16 output tile.  S = 2: stride 2 (the Downsample convolutions),
// 2x4x16 output tile whose 5 x 9 x 33 input patch is stored with even and odd W columns in separate row runs, so that the 16 voxels of
// a fragment still read 16 consecutive LDS rows for every tap (the DMA source address is free per lane: any layout costs nothing).
// KS = 3: the 3x3x3 kernel.  KS = 2 (in_mode 3): a nearest-2x up-sampling followed by a 3x3x3 convolution, evaluated as 8 sub-pixel
// 2x2x2 convolutions on the LOW-resolution input -- of the 27 taps of an output voxel only 8 distinct input voxels exist, so the weights
// are pre-summed per output parity (ops.py) and the launch does 8/27 of the multiply-adds (reference: Upsample = interpolate + conv,
// diffusion_model_unet.py:572-585, autoencoderkl.py:76-93).  The parity is a grid dimension: it selects the weight image, the low-side
// padding (1 - parity per axis) and the output sub-lattice the tile is written to.
// NFR_ = 16-channel output fragments per wave: 4 (BN = 64 output channels per work-group) or 8 (BN = 128: one staged patch feeds
// twice the output channels -- half the patch traffic per multiply-add, 0.375 instead of 0.5 LDS operand reads per MFMA at MF = 4).
// PRE: the instantiation that applies the fused GroupNorm-apply + activation prologue in LDS (a separate instantiation so that the plain
// kernel's register allocation -- 128 VGPRs = four waves per SIMD for cfg 11 -- is not disturbed by code it never runs).
// phase_wgs / phase_sleeps: the ONE-TIME phase offset between the work-groups that share a CU (round 5).  The dispatcher starts the co-resident
// work-groups of a CU together, their tiles take equal time, and every replacement starts when its predecessor ends: the work-groups of a CU
// run in LOCK STEP for the whole launch -- both in the tap loop (each gets half the MFMA pipe), then both in the epilogue (the pipe idles):
// tile life = non-loop time + 2 x MFMA time, which is what the cycle stamps show (64 -> 64: 18 k + 2 x 13.8 k = 45.6 k modelled, 44.3 k
// measured; 192 -> 64: 119 k modelled, 117.9 k measured).  Delaying the work-groups of the FIRST residency round that sit in an odd
// work-group slot of their CU (HW_ID.TG_ID) by about half a tile puts one work-group's epilogue / chunk boundary under the other's tap
// loop; every later work-group inherits the phase of the slot it is dispatched into.  (The round-2 skew experiment delayed EVERY tile of the
// odd slot by <= 3 k cycles -- a permanent handicap of one slot, not a phase.)  Results do not depend on it.
template <typename T, int NW, int MF, int S, int MINW, int KS = 3, int NFR_ = 4, bool PRE = false>
__global__ __launch_bounds__(64 * NW, MINW) void conv_dma_kernel(const GmConvDesc p, const unsigned phase_wgs, const unsigned phase_sleeps) {
  constexpr int BK = ConvTraits<T>::BK;
  constexpr int VECW = ConvTraits<T>::VECW;
  constexpr int NT = 64 * NW;
  constexpr int NFR = NFR_, G = KS == 3 ? 3 : 2, RING = KS == 3 ? 3 : 4;  // taps per weight panel; panels in the LDS ring
  static_assert(KS == 3 || (KS == 2 && S == 1 && (NW == 8 || NW == 4)), "the sub-pixel variant is stride 1, 8 waves x 32 or 4 waves x 64 voxels");
  static_assert(NW * MF * 16 == 512 || NW * MF * 16 == (S == 1 ? 256 : 128), "waves x fragments cover the tile");
  constexpr int TH = 4, TW = 16, BM = NW * MF * 16, TD = BM / (TH * TW);  // 4x4x16 (8x4x16 for the 16-wave variant); S = 2: 2x4x16
  // NPW (round 5): a sub-pixel work item covers BOTH W parities of its (d, h) parity: parity 0 reads input columns (i - 1, i), parity 1 (i, i + 1) --
  // the union i - 1 .. i + 1 is one column more of the same staged patch (5 x 18 = 90 rows of a 96-row plane: no more LDS), so one patch request per
  // chunk feeds 16 taps instead of 8: half the patch traffic, half the chunk boundaries, placements and first-patch waits per output voxel (the
  // launch was 0.84 ms at 983 TFLOP/s executed with 707 MB of HBM traffic against 377 algorithmic: VERDICT r4 weak 5).  Two accumulator sets.
  constexpr int NPW = KS == 2 ? 2 : 1;
  constexpr int PD = S * (TD - 1) + KS, PH = S * (TH - 1) + KS, PW = S * (TW - 1) + KS + (NPW - 1);  // LDS rows per W line (33 for S = 2: 17 even + 16 odd)
  constexpr int EW = TW + 1;                                                            // S = 2: rows of the even-column run
  constexpr int PLANE = ((PH * PW + 15) / 16) * 16;        // 112 rows: depth offsets keep (row mod 16)
  constexpr int PROWS = PD * PLANE;                        // 672 rows = 42 DMA pieces
  constexpr int PPIECES = PROWS / 16;
  constexpr int PPW = (PPIECES + NW - 1) / NW;             // patch pieces per wave (6; the last round is partial)
  constexpr int BN = 16 * NFR;
  constexpr int WROWS = G * BN;                            // 192 rows per weight panel = 12 KiB = 1.5 pieces per wave (BN = 64)
  constexpr bool WGEN = NFR != 4 || (KS == 2 && NW == 4);  // general panel distribution: piece wave + NW * h, whole pieces only
  constexpr int PATCH_BYTES = PROWS * DMA_ROWB;
  constexpr int WBUF_BYTES = WROWS * DMA_ROWB;
  constexpr int PVT_OFF = PATCH_BYTES + (KS == 2 ? 36864 : RING * WBUF_BYTES) + 512;  // the placement table of the sub-pixel form (behind the addend vector)
  constexpr int NGROUPS = KS * KS * KS / G * NPW;          // 27 taps / 3, or 2 parities x 8 taps / 2: group g of a chunk = (W parity g / 4, taps 2 (g % 4) ..)
  // DMA instructions per wave per weight panel (12 pieces): 8 waves x (1 full + 1 half piece), 4 waves x 3 full, or -- 16 waves --
  // one full piece on waves 0..11 and none on waves 12..15 (the end-of-group wait count is then wave dependent)
  constexpr int WPW = WGEN ? WROWS / 16 / NW : (KS == 2 ? 1 : (NW == 8 ? 2 : (NW == 4 ? 3 : 1)));  // KS = 2: 128 rows = 8 pieces, one per wave
  static_assert(!WGEN || (S == 1 && (WROWS / 16) % NW == 0), "general panel distribution: whole pieces per wave");
  static_assert(WROWS == (KS == 3 ? 3 : 2) * BN, "G taps per weight panel");
  static_assert(NGROUPS % RING == 0, "the ring slot of a group is a compile-time constant");
  // weight rows in direct_chan() order (the register-direct epilogue below).  Not for the sub-pixel form: its output voxels are every other
  // voxel of a row, a store instruction would write sixteen isolated 64-byte halves of 128-byte lines (measured: cfg 17 0.84 -> 1.04 ms)
  constexpr bool DIRECT_W = NFR == 4 && KS == 3;

  extern __shared__ __attribute__((aligned(1024))) char smem[];  // [patch 42 KiB][3 weight panels x 12 KiB][addend vector 512 B]
  const unsigned lds0 = (unsigned)(uintptr_t)smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, q = lane >> 4;
  if (blockIdx.x < phase_wgs) {  // (first residency round only; work-group uniform)
    const unsigned tg = __builtin_amdgcn_s_getreg((3 << 11) | (16 << 6) | 4);  // HW_REG_HW_ID[19:16] = TG_ID: the work-group's slot on its CU
    if (tg & 1) {
      for (unsigned k = phase_sleeps; k > 0; --k) __builtin_amdgcn_s_sleep(16);  // 16 x 64 = 1 024 cycles per iteration
    }
  }

  // ---- launch constants -------------------------------------------------------------------------------------------------------------------
  // KS = 2: the tiles walk the low-resolution grid (= the input grid); p.Do/Ho/Wo are the full-resolution output extents
  const int Dt = KS == 2 ? p.Ds : p.Do, Ht = KS == 2 ? p.Hs : p.Ho, Wt = KS == 2 ? p.Ws : p.Wo;
  const int ntd = (Dt + TD - 1) / TD, nth = (Ht + TH - 1) / TH, ntw = (Wt + TW - 1) / TW;
  const int ncb = (p.Cout + BN - 1) / BN;
  // split-K (small grids): the work list holds ksplit copies of the tile list; copy ks computes K chunks [c_begin, c_end) only
  const int ksplit = (KS == 3 && S == 1 && p.kpartial && p.ksplit > 1) ? p.ksplit : 1;
  int Dv = p.Ds, Hv = p.Hs, Wv = p.Ws;
  if (p.in_mode == 1) { Dv *= p.fd; Hv *= p.fh; Wv *= p.fw; }
  const int nchunks = p.Cin / BK;                          // host-checked: Cin % BK == 0
  const int cout_pad = (p.Cout + 15) & ~15;
  const int cps = ksplit > 1 ? (nchunks + ksplit - 1) / ksplit : nchunks;  // chunks per K slice (host-checked: (ksplit - 1) * cps < nchunks, no slice is empty)

  // ---- the work list of this work-group ---------------------------------------------------------------------------------------------------
  // nwork = tiles x channel blocks (x 8 parities) (x K slices) work items.  The dispatcher deals consecutive work-groups round-robin to the 8
  // XCDs (each with a private L2): XCD x owns the contiguous item range [sx, sx + cx) -- neighbouring halo patches meet in one L2 -- and its
  // gx work-groups walk it with stride gx.  A grid of nwork work-groups (gx == cx) is the one-tile-per-work-group launch; the host caps the
  // grid at the number of co-resident work-groups (gm_conv_dma_launch), and a work-group then runs several tiles back to back: the tile-
  // independent address tables are built once and the first patch of the next tile is requested BEFORE the epilogue of the current one.
  const unsigned nwork = (unsigned)p.N * ntd * nth * ntw * ncb * (KS == 2 ? 4u : 1u) * (unsigned)ksplit;  // KS = 2: x the four (d, h) parities
  const unsigned xcd = blockIdx.x & 7, gx = (gridDim.x >> 3) + (xcd < (gridDim.x & 7) ? 1u : 0u);
  const unsigned q8 = nwork >> 3, r8 = nwork & 7, cx = q8 + (xcd < r8 ? 1u : 0u), sx = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
  unsigned pos = blockIdx.x >> 3;
  if (pos >= cx) return;  // (never for gridDim.x <= nwork)
#ifdef GM_CONV_TIMELINE
  const unsigned tl_pos = pos + gx < cx ? pos + gx : pos;  // stamp the second tile of a persistent work-group (steady state), else its only one
#endif

  struct Tile { int cb, par, n, td_i, th_i, tw_i, ks; };
  auto decode = [&](unsigned wi) __attribute__((always_inline)) {
    Tile t;
    unsigned b = wi;
    t.ks = 0;
    if (ksplit > 1) {  // (the divisions stay off the common path)
      const unsigned tiles_all = nwork / (unsigned)ksplit;
      t.ks = (int)(b / tiles_all);
      b -= (unsigned)t.ks * tiles_all;
    }
    t.cb = b % ncb; b /= ncb;
    t.par = 0;
    if (KS == 2) { t.par = b & 3; b >>= 2; }  // (d parity, h parity); the W parity is a loop inside the work item
    t.tw_i = b % ntw; b /= ntw;
    t.th_i = b % nth; b /= nth;
    t.td_i = b % ntd; b /= ntd;
    t.n = b;
    return t;
  };

  // ---- per-lane DMA sources ---------------------------------------------------------------------------------------------
  // patch piece j of this wave covers LDS rows 16*(wave + NW*j) .. +15; lane -> (row, LDS slot lane&3) <- channel slot swizzled
  const char* zero = reinterpret_cast<const char*>(gm_zero_row);
  const char* xbase = reinterpret_cast<const char*>(p.x);
  // The bank swizzle of a patch row is keyed on the row's COLUMN within its W line (lc), not on the row index: a tap's operand address is
  // then (lane base for kw) + (line, plane) * constant -- KS address registers per lane instead of KS x (S (MF - 1) + KS) -- and conflict-free
  // for the same reason (the 16 lanes of a fragment read 16 consecutive columns).  psw: the 2-bit swizzle of this lane's row, per piece.
  int psw = 0;
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int row = 16 * (wave + NW * j) + (lane >> 2);
    const int rr = row % PLANE;
    psw |= dma_swz(rr % PW) << (2 * j);
  }
  int pvox[PPW];  // source voxel of this lane's patch row per piece, or -1 for a padding row (32-bit: host checks N*V < 2^31)
  // PVOX_LDS: the sub-pixel form carries two accumulator sets (128 registers) and two operand sets through its tap loop; its eight placements per
  // lane did not fit next to them and went to scratch -- reloaded in front of every patch request, i.e. behind the previous piece's LDS-DMA
  // (vector memory returns in order).  They live in LDS instead (8 KiB behind the addend vector; a lane reads back only what it wrote).
  constexpr bool PVOX_LDS = KS == 2 && NW == 4;
  int* pvt = reinterpret_cast<int*>(smem + PVT_OFF) + threadIdx.x;  // entry j of this thread: pvt[j * NT]; entry PPW: the slot keys psw
  if (PVOX_LDS) pvt[PPW * NT] = psw;
  auto place_patch = [&](const Tile& t) __attribute__((always_inline)) {
    KDesc& pk = cold_desc();
    // KS = 2: output parity 0 reads inputs (i - 1, i), parity 1 reads (i, i + 1): low-side padding 1 - parity
    const int ud0 = t.td_i * TD * S - (KS == 2 ? 1 - ((t.par >> 1) & 1) : pk.pd), uh0 = t.th_i * TH * S - (KS == 2 ? 1 - (t.par & 1) : pk.ph),
              uw0 = t.tw_i * TW * S - (KS == 2 ? 1 : pk.pw);  // KS = 2: the union of both W parities starts at column i - 1
    OPAQUE_LANE(lane_p);
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int row = 16 * (wave + NW * j) + (lane_p >> 2);  // (the row's place in the patch is recomputed per tile: two constant divisions
      const int pa = row / PLANE, rr = row - pa * PLANE;   //  are cheaper than six more live registers across the tap loop)
      const int pb = rr / PW, lc = rr - pb * PW;
      const int pc = S == 1 ? lc : (lc < EW ? 2 * lc : 2 * (lc - EW) + 1);  // S = 2: even columns first, then the odd ones
      int ud = ud0 + pa, uh = uh0 + pb, uw = uw0 + pc;
      const bool ok = (row < PROWS) & (rr < PH * PW) & (ud >= 0) & (ud < Dv) & (uh >= 0) & (uh < Hv) & (uw >= 0) & (uw < Wv);
      if (pk.in_mode == 1) { ud /= pk.fd; uh /= pk.fh; uw /= pk.fw; }
      const int pvj = ok ? ((t.n * pk.Ds + ud) * pk.Hs + uh) * pk.Ws + uw : -1;
      if (PVOX_LDS) pvt[j * NT] = pvj; else pvox[j] = pvj;
    }
  };
  const long long xrowb = p.x_ld * (long long)sizeof(T);
  // optional second source: input channels [cin_split, Cin) come from x2 (the never-materialised torch.cat([h, skip]) of the decoder)
  const char* x2base = reinterpret_cast<const char*>(p.x2);
  const long long x2rowb = p.x2_ld * (long long)sizeof(T);
  const int nchunks0 = p.x2 ? p.cin_split / BK : nchunks;
  // (Staging the patch through registers instead -- all loads of a lane in flight, then ds_write_b128 -- was measured 5-7 % slower.)
  auto issue_patch = [&](int chunk) __attribute__((always_inline)) {
#ifdef GM_CONV_ABLATE
    if (p.debug_flags & 1024) return;  // bench-only: no patch traffic (results are garbage)
#endif
    const bool second = chunk >= nchunks0;  // wave-uniform
    const char* cbase = second ? x2base + (long long)(chunk - nchunks0) * (BK * (int)sizeof(T)) : xbase + (long long)chunk * (BK * (int)sizeof(T));
    const long long rowb = second ? x2rowb : xrowb;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      if (wave + NW * j < PPIECES) {  // wave-uniform
        int pv = PVOX_LDS ? pvt[j * NT] : pvox[j];
        asm volatile("" : "+v"(pv));  // opaque: keeps the 64-bit row offsets pvox[j] * rowb (x and x2: 24 registers) out of the chunk loop's live set
        int ps = PVOX_LDS ? pvt[PPW * NT] : psw;  // (likewise the slot keys: hoisted per piece they went to scratch in the sub-pixel form, and so did the one register they come from)
        if (PVOX_LDS) asm volatile("" : "+v"(ps));
        const char* src = pv >= 0 ? cbase + pv * rowb + (((lane & 3) ^ ((ps >> (2 * j)) & 3)) << 4) : zero + ((lane & 3) << 4);
        dma16(src, lds0 + (unsigned)(16 * (wave + NW * j)) * DMA_ROWB);
      }
    }
  };

  Tile cur = decode(sx + pos);
  const Tile stride = decode(gx);  // the digits of the walk's stride (gx <= cx <= nwork / 8 + 1: a valid work item index, K slice 0)
  place_patch(cur);
  if (min(nchunks, cur.ks * cps) < nchunks) issue_patch(min(nchunks, cur.ks * cps));  // the first patch of the first tile

  // ---- fused GroupNorm-apply + activation prologue (pre_scale / pre_shift / pre_act), applied IN LDS to the landed patch ---------------
  // Each lane transforms 16-byte pieces of its own wave's DMA instructions (piece j, row 16 * (wave + NW * j) + lane / 4, the LDS slot that holds
  // channel slot lane & 3 of the chunk): act(x * scale[n][c] + shift[n][c]) in fp32, rounded back to T -- the same arithmetic and rounding as
  // gm_gn_apply, so the fused and the two-pass forms are bit-identical.  Rows that came from the zero page stay zero: the reference pads
  // the ACTIVATED tensor (conv(silu(gn(x))), diffusion_model_unet.py:671-684).  Needs no barrier of its own: a wave's own DMA pieces are
  // complete after its vmcnt(0), and the barrier that follows publishes the transformed rows.  Each halo row is transformed once per
  // work-group that stages it (2.1x redundant at the 512-voxel tile) on the VALU -- against a whole extra read + write pass over HBM.
  constexpr bool pre = PRE;
  float sc[VECW], sh[VECW];  // this lane's scale / shift for the chunk being staged: loaded next to the patch DMA, consumed after its wait
  auto load_affine = [&](int chunk) __attribute__((always_inline)) {
    const int c0 = chunk * BK + (lane & 3) * VECW;   // this lane's channels within cat(x, x2): channel slot lane & 3 of every row it transforms
    const float* ps = p.pre_scale + (long long)cur.n * p.Cin + c0;
    const float* ph = p.pre_shift + (long long)cur.n * p.Cin + c0;
#pragma unroll
    for (int i = 0; i < VECW; i += 4) {
      const float4 a = *reinterpret_cast<const float4*>(ps + i), b = *reinterpret_cast<const float4*>(ph + i);
      sc[i] = a.x; sc[i + 1] = a.y; sc[i + 2] = a.z; sc[i + 3] = a.w;
      sh[i] = b.x; sh[i + 1] = b.y; sh[i + 2] = b.z; sh[i + 3] = b.w;
    }
  };
  auto transform_patch = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      if (wave + NW * j < PPIECES && pvox[j] >= 0) {
        char* a = smem + (16 * (wave + NW * j) + (lane >> 2)) * DMA_ROWB + (((lane & 3) ^ ((psw >> (2 * j)) & 3)) << 4);  // (a piece of this wave's own DMA instruction)
        float v[VECW];
        Vec16<T>::unpack(*reinterpret_cast<const uint4*>(a), v);
#pragma unroll
        for (int i = 0; i < VECW; ++i) v[i] = v[i] * sc[i] + sh[i];
        // the activation kind is tested once per vector (conv_act_vec): a per-element ternary on p.pre_act compiled to one basic block per
        // element with the v_exp -> v_rcp chain of each SiLU fully exposed -- what made this prologue cost as much as a pass over HBM in round 2
        conv_act_vec(v, p.pre_act, sizeof(T) == 4);
        *reinterpret_cast<uint4*>(a) = Vec16<T>::pack(v);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the stores are in LDS before the barrier that follows
  };


  // weight panel of global tap group t (chunk = t / 9, taps 3*(t%9) ..): rows r = u*64 + co_local.  Wave w moves rows
  // 16w .. 16w+15 (full piece) and rows 128 + 8w .. +7 (half piece, lanes 0..31).
  const char* wbase = nullptr;  // parity image of the current tile
  int wsrc[WPW];                // byte offset within a (chunk, group) panel image, or -1 (channel beyond cout_pad)
  auto place_weights = [&](const Tile& t) __attribute__((always_inline)) {
    KDesc& pk = cold_desc();
    wbase = reinterpret_cast<const char*>(pk.w) + (long long)(t.par * NPW) * nchunks * (KS * KS * KS) * cout_pad * DMA_ROWB;  // image of W parity 0; parity 1 follows it
    OPAQUE_LANE(lane_w);
#pragma unroll
    for (int h = 0; h < WPW; ++h) {
      const int row = WGEN ? 16 * (wave + NW * h) + (lane_w >> 2)
                    : KS == 2 ? 16 * wave + (lane_w >> 2)
                              : NW == 8 ? (h == 0 ? 16 * wave + (lane_w >> 2) : 128 + 8 * wave + ((lane_w & 31) >> 2))
                                        : (NW == 4 ? 16 * (wave + NW * h) + (lane_w >> 2) : 16 * (wave < 12 ? wave : 0) + (lane_w >> 2));
      const int u = row / BN, col = row % BN;
      const int co = t.cb * BN + (DIRECT_W ? direct_col_chan<T>(col) : col);  // (the LDS row keeps its place and swizzle: only its SOURCE changes)
      wsrc[h] = co < cout_pad ? ((u * cout_pad + co) * DMA_ROWB + (((lane_w & 3) ^ dma_swz(row)) << 4)) : -1;
    }
  };
  auto issue_w_pieces = [&](int t, int buf, int h0, int h1) __attribute__((always_inline)) {  // pieces [h0, h1) of the WPW instructions per wave
#ifdef GM_CONV_ABLATE
    if (p.debug_flags & 512) return;  // bench-only: no weight traffic (results are garbage)
#endif
    // KS = 3: (chunk * 27 + 3 * grp) * cout_pad rows.  KS = 2: t = chunk * 8 + g, W parity g / 4 -> its image, rows (chunk * 8 + 2 (g % 4)) * cout_pad
    const char* panel = KS == 2 ? wbase + ((long long)((t & 7) >> 2) * nchunks * 8 + (long long)(t >> 3) * 8 + 2 * (t & 3)) * cout_pad * DMA_ROWB
                                : wbase + (long long)t * G * cout_pad * DMA_ROWB;
    const unsigned dst = lds0 + PATCH_BYTES + (unsigned)buf * WBUF_BYTES;
#pragma unroll
    for (int h = h0; h < h1; ++h) {
      const char* src = wsrc[h] >= 0 ? panel + wsrc[h] : zero + ((lane & 3) << 4);
      if (WGEN) {
        dma16(src, dst + (unsigned)(16 * (wave + NW * h)) * DMA_ROWB);
      } else if (KS == 2) {
        dma16(src, dst + (unsigned)(16 * wave) * DMA_ROWB);
      } else if (NW == 8) {
        if (h == 0) dma16(src, dst + (unsigned)(16 * wave) * DMA_ROWB);
        else if (lane < 32) dma16(src, dst + (unsigned)(128 + 8 * wave) * DMA_ROWB);
      } else if (NW == 16) {
        if (wave < 12) dma16(src, dst + (unsigned)(16 * wave) * DMA_ROWB);
      } else {
        dma16(src, dst + (unsigned)(16 * (wave + NW * h)) * DMA_ROWB);
      }
    }
  };
  auto issue_w = [&](int t, int buf) __attribute__((always_inline)) { issue_w_pieces(t, buf, 0, WPW); };  // WPW instructions per wave, every wave


  // ---- LDS regions of the epilogue ---------------------------------------------------------------------------------------------------------
  // Transpose scratch: NW wave-private blocks of MF*16 rows x 144 B.  When they fit into the weight ring (EARLY: cfg 11 / 14 / 15 / 17 / 19) the
  // patch buffer is free from the last tap on, and the next tile's first patch is requested before the epilogue; otherwise (the 512-voxel x
  // 64-channel tiles) the scratch overlays the patch buffer and the request follows the epilogue.
  constexpr int SCRATCH_WAVE = MF * 16 * 144, SCRATCH_BYTES = NW * SCRATCH_WAVE;
  constexpr int RING_BYTES = KS == 2 ? (RING * WBUF_BYTES > 36864 ? RING * WBUF_BYTES : 36864) : RING * WBUF_BYTES;  // KS = 2: padded to hold the scratch
  constexpr bool EARLY = SCRATCH_BYTES <= RING_BYTES;
  constexpr int SCRATCH_OFF = EARLY ? PATCH_BYTES : 0;
  static_assert(EARLY || SCRATCH_BYTES <= PATCH_BYTES + RING_BYTES, "the transpose scratch fits under the addend vector");
  static_assert(BN * 8 <= SCRATCH_WAVE, "a wave's statistic partials fit into its scratch block");
  static_assert(PVT_OFF == PATCH_BYTES + RING_BYTES + 512, "the placement table follows the addend vector");
  float* addv = reinterpret_cast<float*>(smem + PATCH_BYTES + RING_BYTES);  // per-channel epilogue addend of this work-group's BN output channels
  // DIRECT: the register-direct epilogue (conv_dma_shared.h): the weight rows of a panel are DMA'd in direct_chan() order, so that a lane's
  // accumulators are 16-byte runs of the output row and no LDS transpose is needed (64-channel tiles; the other tiles, and the rare output-activation
  // form, keep the transposed one.  Round 5 A/B against the transposed form everywhere: profiles/r05_phase_skew_sweep.txt)
  constexpr bool DIRECT = NFR == 4 && KS == 3;
  constexpr int EPASSES = (NFR * 16 * (int)sizeof(T) + 127) / 128;
  constexpr int CH_PER_PASS = 128 / (int)sizeof(T);
  static_assert(EPASSES <= 4, "at most 4 epilogue passes (128 output channels in fp32)");

  for (;;) {
#ifdef GM_CONV_TIMELINE
    const bool tl_on = pos == tl_pos;
#endif
    TL_STAMP(0);
    const int c_begin = min(nchunks, cur.ks * cps), c_end = min(nchunks, c_begin + cps);
    const int total = (c_end - c_begin) * NGROUPS;            // an empty slice (never launched by the host) would touch nothing: total == 0
    const int od0 = cur.td_i * TD, oh0 = cur.th_i * TH, ow0 = cur.tw_i * TW;
    // ---- the first panels go out behind the patch already in flight; everything below that does not feed them runs under the DMA ------------
    TL_STAMP(1);
    place_weights(cur);
    if (total > 0) {
      issue_w(c_begin * NGROUPS, 0);
      if (total > 1) issue_w(c_begin * NGROUPS + 1, 1);
      if (pre) load_affine(c_begin);
    }
    // bias + shortcut bias + timestep row (this order), fp32
    float addend = 0.f;
    KDesc& pa = cold_desc();
    OPAQUE_LANE(lane_a);
    const int tid_a = wave * 64 + lane_a;  // (= threadIdx.x, from the phase's own lane id)
    if (tid_a < BN) {
      const int co = cur.cb * BN + tid_a;
      if (co < pa.Cout) {
        if (pa.bias) addend += pa.bias[co];
        if (pa.skip_bias) addend += pa.skip_bias[co];
        if (pa.rowvec) addend += pa.rowvec[(long long)cur.n * pa.rowvec_bstride + co];
      }
    }
    TL_STAMP(55);
    // ---- per-lane operand read addresses (bytes from smem): rebuilt per tile under the DMA flight -- 16 registers that are NOT live across the
    // epilogue, where they would push the allocation into scratch (a scratch reload behind the next tile's patch request waits for the patch)
    // A wave's MF fragments are MF consecutive H rows of one tile plane ((wave * MF + mf) * 16 + l15 with TH = 4, TW = 16), so fragment mf
    // at tap row kh reads patch row S * (bb0 + mf) + kh: the addresses depend on hk = S * mf + kh only -- HK x KS registers, not MF x KS x KS.
    constexpr int HK = S * (MF - 1) + KS;
    static_assert(MF <= 4 && (4 % MF) == 0, "a wave's fragments stay inside one 4-row tile plane");
    OPAQUE_LANE(lane_t);  // keeps the two tables out of loop-invariant code motion (= out of the epilogue's live set)
    const int l15t = lane_t & 15, qt = lane_t >> 4;
    constexpr int NXA = KS + NPW - 1;  // tap columns of the staged patch (KS = 2: tap kw of W parity pw reads union column kw + pw)
    int xa[NXA];  // patch row of this lane's voxel column for tap column kw (line 0 of the wave's fragments); lines / planes are immediates
    {
      const int m0 = wave * MF * 16 + l15t;
      const int a = m0 >> 6, bb0 = (m0 >> 4) & 3, c = m0 & 15;
#pragma unroll
      for (int kw = 0; kw < NXA; ++kw) {
        const int col = S == 1 ? c + kw : (kw == 1 ? EW + c : c + (kw >> 1));  // patch column S*c + kw in the split layout
        xa[kw] = (S * a * PLANE + S * bb0 * PW + col) * DMA_ROWB + ((qt ^ dma_swz(col)) << 4);
      }
    }
    // weight rows nf * 16 + l15: the swizzle has period 8 rows, so every further fragment is fragment 0 plus 16 rows -- an immediate
    const int wa0 = PATCH_BYTES + l15t * DMA_ROWB + ((qt ^ dma_swz(l15t)) << 4);
#define XADDR(hk, kw) (xa[kw] + (hk) * (PW * DMA_ROWB))
#define WADDR(nf) (wa0 + (nf) * (16 * DMA_ROWB))
    f32x4_t accs[NPW][NFR][MF];
#pragma unroll
    for (int pw = 0; pw < NPW; ++pw)
#pragma unroll
      for (int nf = 0; nf < NFR; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) accs[pw][nf][mf] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    f32x4_t (&acc)[NFR][MF] = accs[0];  // (the 3x3x3 forms have one set)
    if (tid_a < BN) addv[tid_a] = addend;
    TL_STAMP(56);
    if (total > 0) {
      dma_wait<0>();
      if (pre) transform_patch();
    }
    __builtin_amdgcn_s_barrier();
#ifdef GM_CONV_TIMELINE
    // bench-only experiment (debug_flags bit 11): the work-groups of a CU start in pairs and stay in lock step (equal lifetimes), every wave
    // wanting the LDS port and then the MFMA pipe at the same moment; skew the odd work-group slot (HW_ID.TG_ID) by bits 16..23 x 64 cycles
    if (p.debug_flags & 2048) {
      const unsigned tg = __builtin_amdgcn_s_getreg((3 << 11) | (16 << 6) | 4);  // HW_REG_HW_ID[19:16]
      if (tg & 1) {
        for (int k = (p.debug_flags >> 16) & 255; k > 0; --k) __builtin_amdgcn_s_sleep(1);
      }
    }
#endif
    TL_STAMP(2);

    // ---- main loop ----------------------------------------------------------------------------------------------------------
    for (int chunk = c_begin; chunk < c_end; ++chunk) {
      const bool last_chunk = chunk + 1 == c_end;
      constexpr int NH = NFR / 4;
      // two operand sets where they fit without scratch (hipcc 7.2: the sub-pixel, stride-2 and the 256-register tiles without a fused prologue; the
      // 128-register tiles -- cfg 11 / 16 -- and the prologue forms would spill 70-350 registers)
      constexpr bool PIPE2 = NH == 1 && !PRE && (KS == 2 || S == 2 || MINW == 2);
      if constexpr (PIPE2) {
        // Two operand register sets, software-pipelined over the taps AND over the group barrier (ISA of the single-set form: the last tap's
        // four weight fragments went through ONE register quad -- read, wait, 2 MFMAs, four times -- and every group began with ~45 address
        // instructions of the panel request in front of its first LDS read: a wave alone on its SIMD pair ran a group in 1 370 cycles against
        // 384 cycles of MFMA issue).  Group g: tap 0 is already in set X (read right after the barrier that ended group g - 1, whose wait made
        // panel g visible); tap 1 -> set Y under tap 0's MFMAs, the panel request's address arithmetic in the shadow of those MFMAs, tap 2 -> X
        // under tap 1's MFMAs, end-of-group wait + barrier, next group's tap 0 -> Y under tap 2's MFMAs.  A chunk's first group reads its own tap 0
        // (the patch has just been replaced).
        uint4 xf[2][MF], wf[2][4];
        auto read_tap = [&](int g, int u, int set) __attribute__((always_inline)) {
          const int tap = (KS == 2 ? g % 4 : g) * G + u;  // KS = 2: groups 4 .. 7 are the taps of W parity 1 ...
          const int kd = tap / (KS * KS), kh = (tap / KS) % KS, kw = tap % KS + (KS == 2 ? g / 4 : 0);  // ... one patch column further
#pragma unroll
          for (int nf = 0; nf < 4; ++nf)
            wf[set][nf] = *reinterpret_cast<const uint4*>(smem + WADDR(nf) + (g % RING) * WBUF_BYTES + u * (BN * DMA_ROWB));
#pragma unroll
          for (int mf = 0; mf < MF; ++mf)
            xf[set][mf] = *reinterpret_cast<const uint4*>(smem + XADDR(S * mf + kh, kw) + kd * (PLANE * DMA_ROWB));
        };
        auto mma_tap_pw = [&](int set, int pw) __attribute__((always_inline)) {
#pragma unroll
          for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) Mma<T>::run(wf[set][nf], xf[set][mf], accs[pw][nf][mf]);
        };
#define mma_tap(set) mma_tap_pw(set, KS == 2 ? g / 4 : 0)  /* every tap multiplied inside iteration g belongs to group g */
        constexpr int NMMA = MF * 4 * (sizeof(T) == 2 ? 1 : 4), NRD = MF + 4;
        static_assert(G == 3 || G == 2, "taps per panel");
#pragma unroll
        for (int g = 0; g < NGROUPS; ++g) {
          const int t = chunk * NGROUPS + g;
          const int X = (g * G) & 1, Y = X ^ 1;                              // operand set of a tap = (tap index) & 1
          const int LASTSET = (g * G + G - 1) & 1, NEXTSET = ((g + 1) * G) & 1;  // ... of the group's last tap / the next group's first
          if (g == 0) read_tap(0, 0, X);
          read_tap(g, 1, Y);
          mma_tap(X);
          if (g == 0) __builtin_amdgcn_sched_group_barrier(0x100, 2 * NRD, 0);  // the operand reads first, then the tap's MFMAs
          else __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NMMA, 0);
          // panel t+2 goes into the ring slot group t-1 read from (every wave is past the barrier that ended it)
          if (g < NGROUPS - 2 || !last_chunk) issue_w(t + 2, (g + 2) % RING);
          if (G == 3) {
            read_tap(g, 2, X);
            mma_tap(Y);
            __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NMMA, 0);
          }
          if (g == NGROUPS - 1) {
            if (!last_chunk) {
              asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
              __builtin_amdgcn_s_barrier();  // every wave is done with this chunk's patch
              issue_patch(chunk + 1);
              if (pre) load_affine(chunk + 1);
              dma_wait<0>();                 // patch + the two panels in flight
              if (pre) transform_patch();
              __builtin_amdgcn_s_barrier();
            }
          } else {
            // panel t+1 (issued a group ago) must have landed; panel t+2 (WPW instructions, just issued) may stay in flight.  The wait also
            // retires every LDS read of the group: the barrier releases other waves to DMA into the ring slot this group read.
            if ((g < NGROUPS - 2 || !last_chunk) && (NW != 16 || wave < 12)) dma_wait<WPW>(); else dma_wait<0>();
            __builtin_amdgcn_s_barrier();
            read_tap(g + 1, 0, NEXTSET);
          }
          mma_tap(LASTSET);
          if (g < NGROUPS - 1) {
            __builtin_amdgcn_sched_group_barrier(0x100, NRD, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, NMMA, 0);
          }
          if (chunk - c_begin < 5) TL_STAMP(3 + (chunk - c_begin) * 10 + g);  // after the barrier that ends group g (g = 8: incl. the chunk boundary)
        }
      } else {
#pragma unroll
      for (int g = 0; g < NGROUPS; ++g) {
        const int t = chunk * NGROUPS + g;
        // panel t+2 goes into the ring slot group t-1 read from (every wave is past the barrier that ended it)
        if (g < NGROUPS - 2 || !last_chunk) issue_w(t + 2, (g + 2) % RING);
        // The last tap's operand reads are issued before the end-of-group wait and its MFMAs after the barrier.  The wait retires
        // every LDS read of the group (lgkmcnt(0)): the barrier releases other waves to DMA into the ring slot this group read.
        // BN = 128 splits a tap into NH = 2 half-steps of four channel fragments each (16 + 16 operand registers instead of 48).
        constexpr int NSTEPS = G * NH;
        uint4 xf[MF], wf[4];
        auto read_step = [&](int st) __attribute__((always_inline)) {
          const int u = st / NH, hf = st % NH;
          const int tap = g * G + u;
          const int kd = tap / (KS * KS), kh = (tap / KS) % KS, kw = tap % KS;
#pragma unroll
          for (int nf = 0; nf < 4; ++nf)
            wf[nf] = *reinterpret_cast<const uint4*>(smem + WADDR(nf) + hf * (64 * DMA_ROWB) + (g % RING) * WBUF_BYTES + u * (BN * DMA_ROWB));
          if (hf == 0) {
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
              xf[mf] = *reinterpret_cast<const uint4*>(smem + XADDR(S * mf + kh, kw) + kd * (PLANE * DMA_ROWB));
          }
        };
        auto mma_step = [&](int st) __attribute__((always_inline)) {
          const int hf = st % NH;
#pragma unroll
          for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) Mma<T>::run(wf[nf], xf[mf], acc[hf * 4 + nf][mf]);
        };
        constexpr int NMMA = MF * 4 * (sizeof(T) == 2 ? 1 : 4);
#pragma unroll
        for (int st = 0; st < NSTEPS - 1; ++st) {
          read_step(st);
          mma_step(st);
          if (st % NH == 0) __builtin_amdgcn_sched_group_barrier(0x100, MF + 4, 0);  // all operand reads of a step before its MFMAs
          else __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, NMMA, 0);
        }
        read_step(NSTEPS - 1);
        if (g == NGROUPS - 1) {
          if (!last_chunk) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();  // every wave is done with this chunk's patch
            issue_patch(chunk + 1);
            if (pre) load_affine(chunk + 1);
            dma_wait<0>();                 // patch + the two panels in flight
            if (pre) transform_patch();
            __builtin_amdgcn_s_barrier();
          }
        } else {
          // panel t+1 (issued a group ago) must have landed; panel t+2 (WPW instructions, just issued) may stay in flight
          if ((g < NGROUPS - 2 || !last_chunk) && (NW != 16 || wave < 12)) dma_wait<WPW>(); else dma_wait<0>();
          __builtin_amdgcn_s_barrier();
        }
        mma_step(NSTEPS - 1);
        if (chunk - c_begin < 5) TL_STAMP(3 + (chunk - c_begin) * 10 + g);  // after the barrier that ends group g (g = 8: incl. the chunk boundary)
      }
      }
    }
  TL_STAMP(60);

    const EpTile et = {cur.n, od0, oh0, ow0, cur.cb * BN, cur.par * NPW};  // (KS = 2: the full parity of W parity 0; parity 1 = + 1)
    const bool partial = KS == 3 && S == 1 && ksplit > 1;
    EpRows<MF * 2> rowsP[NPW];
    EpRows<MF * 2>& rows0 = rowsP[0];
    OPAQUE_LANE(lane_e);
    // ---- register-direct epilogue, part 1: row placement + residual requests (their latency runs under the shortcut / the barrier) ----------------
    // (Round 5, measured and removed: requesting the tile's residual rows a chunk EARLIER through the LDS-DMA engine into a dump area, so that these
    //  loads hit L2 -- the 64 -> 64 launches with a residual take 0.05 ms longer than those without -- made every C2 shape 0.7-2.1 % slower and the
    //  forward 14.41-14.51 vs 14.16-14.23 ms: profiles/r05_res_prefetch_ab.txt.  The 0.05 ms are not exposed HBM latency.)
    // W line mf of this wave = tile line wave * MF + mf: (depth, height) wave-uniform, the 16 lanes l15 are its 16 voxels.  Address of store st:
    // scalar row base + lane offset (voxel l15, 16-byte run q) + 64 st.
    constexpr int NST = 16 / VECW;  // 16-byte stores per voxel and lane: 2 (bf16) / 4 (fp32)
    // (the residual rows share rows0.rv with the transposed form: a second 32-register array live across the shortcut pushed the patch / shortcut
    //  source offsets into scratch -- and a scratch reload queued behind an LDS-DMA request returns only after it.  fp32 would need 64: it loads
    //  the residual at the use, the parity path's latency is not the benchmark's)
    constexpr bool RES_AHEAD = sizeof(T) == 2;
    bool d_direct = false, d_lane_ok = false;
    int d_yoff = 0, d_roff = 0;
    if constexpr (DIRECT) {
      KDesc& pd = cold_desc();
      d_direct = pd.post_act == 0 && !partial;
      if (d_direct) {
        const int l15e = lane_e & 15, qe = lane_e >> 4;
        const int Wl = KS == 2 ? pd.Ws : pd.Wo;
        const int lw = KS == 2 ? 2 * l15e : l15e;              // this lane's voxel within the OUTPUT's W line
        d_yoff = lw * (int)(pd.y_ld * (long long)sizeof(T)) + 16 * qe;
        d_roff = lw * (int)(pd.res_ld * (long long)sizeof(T)) + 16 * qe;
        d_lane_ok = ow0 + l15e < Wl;
#pragma unroll
        for (int it = 0; it < MF * 2; ++it) rows0.rv[it] = make_uint4(0u, 0u, 0u, 0u);
        if (RES_AHEAD && pd.res) {
          const int Dl = KS == 2 ? pd.Ds : pd.Do, Hl = KS == 2 ? pd.Hs : pd.Ho;
#pragma unroll
          for (int mf = 0; mf < MF; ++mf) {
            const int line = wave * MF + mf;
            const int od = od0 + (line >> 2), oh = oh0 + (line & 3);
            if (od < Dl && oh < Hl) {  // wave-uniform
              const long long vrow = KS == 2 ? (((long long)cur.n * pd.Do + 2 * od + ((cur.par >> 2) & 1)) * pd.Ho + 2 * oh + ((cur.par >> 1) & 1)) * pd.Wo + 2 * ow0 + (cur.par & 1)
                                             : (((long long)cur.n * pd.Do + od) * pd.Ho + oh) * pd.Wo + ow0;
              const char* rrow = reinterpret_cast<const char*>(pd.res) + (vrow * pd.res_ld + cur.cb * BN) * (long long)sizeof(T);
#pragma unroll
              for (int st = 0; st < NST; ++st) {
                const int cfirst = cur.cb * BN + (64 * st + 16 * qe) / (int)sizeof(T);
                if (d_lane_ok && cfirst < pd.Cout) rows0.rv[(mf * NST + st) % (MF * 2)] = *reinterpret_cast<const uint4*>(rrow + (unsigned)(d_roff + 64 * st));
              }
            }
          }
        }
      }
    }
    if (!partial && !d_direct) {  // residual rows of the first pass: requested now, used after the transpose
#pragma unroll
      for (int pw = 0; pw < NPW; ++pw) {
        const EpTile etp = {et.n, et.od0, et.oh0, et.ow0, et.co_base, et.par + pw};
        dma_epilogue_rows<T, MF, KS, 0>(cold_desc(), etp, wave * MF, lane_e, rowsP[pw]);
      }
    }

    // ---- fused 1x1 shortcut convolution: extra K chunks over the (virtually concatenated) skip sources, centre tap only ----------
    // Two chunks per round: each wave DMAs the 64-byte channel chunk of ITS OWN 32 output voxels (4 pieces) into the patch buffer
    // and one piece of the two 4 KiB weight panels into the ring, one wait + barrier, then 2 x 8 MFMAs.
    KDesc& ps = cold_desc();
    if (ps.skip_x[0] && cur.ks == ksplit - 1) {  // (split-K: the shortcut's chunks ride with the last K slice)
      const int nsc0 = ps.skip_cin[0] / BK, nsc = nsc0 + (ps.skip_x[1] ? ps.skip_cin[1] / BK : 0);
      OPAQUE_LANE(lane_k);
      const int pswz = ((lane_k & 3) ^ dma_swz(lane_k >> 2)) << 4;  // (the shortcut's rows are voxels: row-keyed swizzle, one term per lane)
      int svox[MF];  // output voxel of this lane's centre rows (piece h covers rows wave*32 + h*16 + lane/4), -1 outside the volume
  #pragma unroll
      for (int h = 0; h < MF; ++h) {
        const int m = wave * (MF * 16) + h * 16 + (lane_k >> 2);  // (a, bb, c) below assume TH = 4, TW = 16
        const int od = od0 + (m >> 6), oh = oh0 + ((m >> 4) & 3), ow = ow0 + (m & 15);
        svox[h] = (od < ps.Do && oh < ps.Ho && ow < ps.Wo) ? ((cur.n * ps.Do + od) * ps.Ho + oh) * ps.Wo + ow : -1;
      }
      const int wpiece = WGEN ? wave : (wave & 3);        // BN = 64: piece wave&3 of a 4-piece panel; BN = 128 (8 waves): piece wave of 8
      const int wcol = wpiece * 16 + (lane_k >> 2);         // weight row of this lane's panel piece
      const int wco = cur.cb * BN + (DIRECT_W ? direct_col_chan<T>(wcol) : wcol);
      const int wswz = ((lane_k & 3) ^ dma_swz(wcol)) << 4;
      int caddr[MF];
  #pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        const int m = (wave * MF + mf) * 16 + (lane_k & 15);
        caddr[mf] = m * DMA_ROWB + (((lane_k >> 4) ^ dma_swz(m)) << 4);
      }
      const char* wsk = reinterpret_cast<const char*>(ps.skip_w);
      for (int sc0 = 0; sc0 < nsc; sc0 += 2) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // patch buffer and ring are free
  #pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int sc = sc0 + j;
          if (sc < nsc) {  // wave-uniform
            const int part = sc >= nsc0 ? 1 : 0, cip = sc - (part ? nsc0 : 0);
            const char* xb = reinterpret_cast<const char*>(ps.skip_x[part]) + (long long)cip * (BK * (int)sizeof(T)) + pswz;
            const long long rowb = ps.skip_ld[part] * (long long)sizeof(T);
  #pragma unroll
            for (int h = 0; h < MF; ++h) {
              const char* src = svox[h] >= 0 ? xb + svox[h] * rowb : zero + ((lane_k & 3) << 4);
              dma16(src, lds0 + (unsigned)(j * BM + wave * (MF * 16) + h * 16) * DMA_ROWB);
            }
            if (WGEN || NW == 4 || (wave >> 2) == j) {  // 8 waves: waves 0-3 move panel 0, waves 4-7 panel 1; 4 waves / BN = 128: every wave moves both
              const char* src = wco < cout_pad ? wsk + ((long long)sc * cout_pad + wco) * DMA_ROWB + wswz : zero + ((lane_k & 3) << 4);
              dma16(src, lds0 + PATCH_BYTES + (unsigned)(j * BN + wpiece * 16) * DMA_ROWB);
            }
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
  #pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (sc0 + j < nsc) {
            uint4 xf[MF], wf[4];
  #pragma unroll
            for (int mf = 0; mf < MF; ++mf) xf[mf] = *reinterpret_cast<const uint4*>(smem + caddr[mf] + j * (BM * DMA_ROWB));
  #pragma unroll
            for (int hf = 0; hf < NFR / 4; ++hf) {
  #pragma unroll
              for (int nf = 0; nf < 4; ++nf)
                wf[nf] = *reinterpret_cast<const uint4*>(smem + WADDR(nf) + hf * (64 * DMA_ROWB) + j * (BN * DMA_ROWB));
  #pragma unroll
              for (int nf = 0; nf < 4; ++nf)
  #pragma unroll
                for (int mf = 0; mf < MF; ++mf) Mma<T>::run(wf[nf], xf[mf], acc[hf * 4 + nf][mf]);
            }
          }
        }
      }
    }


    TL_STAMP(61);
    const bool has_next = pos + gx < cx;
    // The barrier "every wave is done with the operand buffers (patch + ring) of this tile": needed before the next tile's patch request and before
    // anything is written into the ring.  The register-direct epilogue touches no LDS until its statistic partials: with no next tile the barrier
    // moves behind the output stores (has_next_early = false), where the waves of the work-group have nothing left to lose by waiting.
    const bool has_next_early = !DIRECT || has_next || partial;
    if (has_next_early) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    // ---- next tile: its first patch is on the way while this tile's epilogue runs ------------------------------------------------------------
    Tile nxt = cur;
    if (has_next) {
      if (ksplit > 1) {
        nxt = decode(sx + pos + gx);
      } else {  // work item + gx by mixed-radix addition of the stride's digits: a few scalar compares instead of four integer divisions
        int c;
        nxt.cb = cur.cb + stride.cb; c = nxt.cb >= ncb ? 1 : 0; nxt.cb -= c ? ncb : 0;
        if (KS == 2) { nxt.par = cur.par + stride.par + c; c = nxt.par >> 2; nxt.par &= 3; }
        nxt.tw_i = cur.tw_i + stride.tw_i + c; c = nxt.tw_i >= ntw ? 1 : 0; nxt.tw_i -= c ? ntw : 0;
        nxt.th_i = cur.th_i + stride.th_i + c; c = nxt.th_i >= nth ? 1 : 0; nxt.th_i -= c ? nth : 0;
        nxt.td_i = cur.td_i + stride.td_i + c; c = nxt.td_i >= ntd ? 1 : 0; nxt.td_i -= c ? ntd : 0;
        nxt.n = cur.n + stride.n + c;
      }
      place_patch(nxt);
      if (EARLY && min(nchunks, nxt.ks * cps) < nchunks) issue_patch(min(nchunks, nxt.ks * cps));
    }
    TL_STAMP(57);
    // ---- split-K: this slice's fp32 partial sums -> kpartial[ks][n * V + voxel][Cout]; the combine kernel applies the epilogue ----------
    KDesc& pe = cold_desc();
    if (KS == 3 && S == 1 && ksplit > 1) {
      const long long nv = (long long)pe.N * pe.Do * pe.Ho * pe.Wo;
      float* part = pe.kpartial + (long long)cur.ks * nv * pe.Cout;
  #pragma unroll
      for (int mf = 0; mf < MF; ++mf) {
        const int m = (wave * MF + mf) * 16 + (lane_e & 15);
        const int od = od0 + (m >> 6), oh = oh0 + ((m >> 4) & 3), ow = ow0 + (m & 15);
        if (od < pe.Do && oh < pe.Ho && ow < pe.Wo) {
          float* row = part + ((((long long)cur.n * pe.Do + od) * pe.Ho + oh) * pe.Wo + ow) * pe.Cout;
  #pragma unroll
          for (int nf = 0; nf < NFR; ++nf) {
            const int co = cur.cb * BN + (DIRECT ? direct_chan<T>(nf, lane_e >> 4, 0) : nf * 16 + (lane_e >> 4) * 4);
            if (co < pe.Cout)  // host-checked: Cout % 4 == 0
              *reinterpret_cast<float4*>(row + co) = make_float4(acc[nf][mf][0], acc[nf][mf][1], acc[nf][mf][2], acc[nf][mf][3]);
          }
        }
      }
    } else {

    // ---- epilogue: LDS transpose -> 16-byte row stores, fused GroupNorm statistics ------------------------------------------------------------
#ifdef GM_CONV_ABLATE
    if (!(pe.debug_flags & 256)) {  // bench-only: main loop without the epilogue
#endif
    if (DIRECT && d_direct) {
      // ---- register-direct epilogue, part 2: + addend, round, (+ residual, round), 16-byte stores, statistics of the stored values ----------------
      // Straight-line code per form (residual yes / no x tile fully inside the volume yes / no): no wave-uniform branch between the eight stores
      // of a wave, so their dependent chains interleave; a lane outside the volume (or past C_out) is masked at the store and contributes
      // zeros to the statistics (a select on the packed value -- conditional accumulation costs a copy per accumulator and branch arm).
      const int qe = lane_e >> 4;
      typedef float f32x2_t __attribute__((ext_vector_type(2)));
      f32x2_t ds[NST][VECW / 2], dq[NST][VECW / 2];
#pragma unroll
      for (int st = 0; st < NST; ++st)
#pragma unroll
        for (int i = 0; i < VECW / 2; ++i) { ds[st][i] = (f32x2_t){0.f, 0.f}; dq[st][i] = (f32x2_t){0.f, 0.f}; }
      const int Dl = KS == 2 ? pe.Ds : pe.Do, Hl = KS == 2 ? pe.Hs : pe.Ho, Wl = KS == 2 ? pe.Ws : pe.Wo;
      const bool has_res = pe.res != nullptr, has_stats = pe.stats != nullptr;
      const bool full = od0 + TD <= Dl && oh0 + TH <= Hl && ow0 + TW <= Wl && (cur.cb + 1) * BN <= pe.Cout;  // wave-uniform: the common tile
      bool ok_st[NST];
#pragma unroll
      for (int st = 0; st < NST; ++st) ok_st[st] = d_lane_ok && cur.cb * BN + (64 * st + 16 * qe) / (int)sizeof(T) < pe.Cout;
      f32x2_t addl[NST][VECW / 2];  // this lane's 16 channels of the addend vector
#pragma unroll
      for (int st = 0; st < NST; ++st)
#pragma unroll
        for (int i = 0; i < VECW; i += 4) {
          const float4 a = *reinterpret_cast<const float4*>(addv + (64 * st) / (int)sizeof(T) + qe * VECW + i);
          addl[st][i / 2] = (f32x2_t){a.x, a.y};
          addl[st][i / 2 + 1] = (f32x2_t){a.z, a.w};
        }
      auto direct_stores = [&](auto RESc, auto FULLc) __attribute__((always_inline)) {
        constexpr bool RES = decltype(RESc)::value, FULL = decltype(FULLc)::value;
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
          const int line = wave * MF + mf;
          const int od = od0 + (line >> 2), oh = oh0 + (line & 3);
          const bool row_ok = FULL || (od < Dl && oh < Hl);  // wave-uniform
          const long long vrow = KS == 2 ? (((long long)cur.n * pe.Do + 2 * od + ((cur.par >> 2) & 1)) * pe.Ho + 2 * oh + ((cur.par >> 1) & 1)) * pe.Wo + 2 * ow0 + (cur.par & 1)
                                         : (((long long)cur.n * pe.Do + od) * pe.Ho + oh) * pe.Wo + ow0;
          char* yrow = reinterpret_cast<char*>(pe.y) + (vrow * pe.y_ld + cur.cb * BN) * (long long)sizeof(T);
          const char* rrow = reinterpret_cast<const char*>(pe.res) + (vrow * pe.res_ld + cur.cb * BN) * (long long)sizeof(T);
#pragma unroll
          for (int st = 0; st < NST; ++st) {
            const bool ok = FULL || (row_ok && ok_st[st]);
            f32x2_t o[VECW / 2];
#pragma unroll
            for (int i = 0; i < VECW / 2; ++i) {
              const f32x4_t c = acc[st * (VECW / 4) + (i >> 1)][mf];
              o[i] = (i & 1 ? (f32x2_t){c[2], c[3]} : (f32x2_t){c[0], c[1]}) + addl[st][i];
            }
            uint32_t w[4];
            auto pack4 = [&]() __attribute__((always_inline)) {
              if (sizeof(T) == 2) {
#pragma unroll
                for (int i = 0; i < VECW / 2; ++i) w[i] = pack_bf16x2(o[i][0], o[i][1]);
              } else {
                w[0] = __float_as_uint(o[0][0]); w[1] = __float_as_uint(o[0][1]); w[2] = __float_as_uint(o[1][0]); w[3] = __float_as_uint(o[1][1]);
              }
            };
            auto unpack4 = [&](const uint32_t (&u)[4], f32x2_t (&v)[VECW / 2]) __attribute__((always_inline)) {
              if (sizeof(T) == 2) {
#pragma unroll
                for (int i = 0; i < VECW / 2; ++i) v[i] = (f32x2_t){__uint_as_float(u[i] << 16), __uint_as_float(u[i] & 0xffff0000u)};
              } else {
                v[0] = (f32x2_t){__uint_as_float(u[0]), __uint_as_float(u[1])};
                v[1] = (f32x2_t){__uint_as_float(u[2]), __uint_as_float(u[3])};
              }
            };
            pack4();
            if (RES) {  // the reference adds the residual to the ROUNDED convolution output and rounds again (x + h in the compute dtype)
              uint4 rv = RES_AHEAD ? rows0.rv[(mf * NST + st) % (MF * 2)] : make_uint4(0u, 0u, 0u, 0u);
              if (!RES_AHEAD && ok) rv = *reinterpret_cast<const uint4*>(rrow + (unsigned)(d_roff + 64 * st));
              const uint32_t ru[4] = {rv.x, rv.y, rv.z, rv.w};
              f32x2_t r[VECW / 2];
              unpack4(w, o);
              unpack4(ru, r);
#pragma unroll
              for (int i = 0; i < VECW / 2; ++i) o[i] += r[i];
              pack4();
            }
            if (ok) *reinterpret_cast<uint4*>(yrow + (unsigned)(d_yoff + 64 * st)) = make_uint4(w[0], w[1], w[2], w[3]);
            // statistics of the values as stored (rounded to T), like a separate pass over the tensor would see them
            if (!FULL) {
#pragma unroll
              for (int i = 0; i < 4; ++i) w[i] = ok ? w[i] : 0u;
            }
            unpack4(w, o);
#pragma unroll
            for (int i = 0; i < VECW / 2; ++i) {
              ds[st][i] += o[i];
              dq[st][i] = __builtin_elementwise_fma(o[i], o[i], dq[st][i]);
            }
          }
        }
      };
      if (has_res) {
        if (full) direct_stores(std::true_type{}, std::true_type{}); else direct_stores(std::true_type{}, std::false_type{});
      } else {
        if (full) direct_stores(std::false_type{}, std::true_type{}); else direct_stores(std::false_type{}, std::false_type{});
      }
      TL_STAMP(62);
      if (has_stats) {
        // lane sums over its MF voxels -> sum over the 16 voxel lanes of a row: (NW > 4: one / two DPP rotate-adds first, the ring holds 9 KiB
        // per wave at NW = 4) every lane with l15 < WL stores its 16 (sum, sum of squares) pairs as one 128-byte row of the wave's own scratch
        // block, lane t then adds the WL rows of ITS channel in a fixed order -> one partial per (wave, channel) -> fixed-order fp64 sum over
        // the waves: deterministic, one plain store per (tile, channel)
        constexpr int DSTEPS = NW <= 4 ? 0 : (NW == 8 ? 1 : 2), WL = 16 >> DSTEPS, WSCR = RING_BYTES / NW;
        static_assert(4 * WL * 144 <= WSCR && BN * 8 <= WSCR, "a wave's statistic rows fit into its share of the weight ring");
        OPAQUE_LANE(lane_s);
        if (DSTEPS >= 1) {
#pragma unroll
          for (int st = 0; st < NST; ++st)
#pragma unroll
            for (int i = 0; i < VECW; ++i) { ds[st][i / 2][i & 1] += dpp_row_ror8(ds[st][i / 2][i & 1]); dq[st][i / 2][i & 1] += dpp_row_ror8(dq[st][i / 2][i & 1]); }
        }
        if (DSTEPS >= 2) {
#pragma unroll
          for (int st = 0; st < NST; ++st)
#pragma unroll
            for (int i = 0; i < VECW; ++i) { ds[st][i / 2][i & 1] += dpp_row_ror4(ds[st][i / 2][i & 1]); dq[st][i / 2][i & 1] += dpp_row_ror4(dq[st][i / 2][i & 1]); }
        }
        if (!has_next_early) {  // (one tile per work-group: the barrier that frees the ring was not needed until here)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
        char* wscr = smem + PATCH_BYTES + (size_t)wave * WSCR;
        const int l15s = lane_s & 15, qs = lane_s >> 4;
        if (l15s < WL) {
          char* rowp = wscr + (qs * WL + l15s) * 144;
#pragma unroll
          for (int st = 0; st < NST; ++st)
#pragma unroll
            for (int i = 0; i < VECW; i += 2)
              *reinterpret_cast<float4*>(rowp + (st * VECW + i) * 8) = make_float4(ds[st][i / 2][0], dq[st][i / 2][0], ds[st][i / 2][1], dq[st][i / 2][1]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // lane t = channel t of the block: byte b = t * sizeof(T) of the row -> store st = b / 64, lane quarter (b % 64) / 16, element (b % 16) / sizeof(T)
        const int bch = lane_s * (int)sizeof(T);
        const char* colp = wscr + (((bch & 63) >> 4) * WL) * 144 + ((bch >> 6) * VECW + (bch & 15) / (int)sizeof(T)) * 8;
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int w = 0; w < WL; ++w) {
          const float2 v = *reinterpret_cast<const float2*>(colp + w * 144);
          sa += v.x;
          sb += v.y;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        *reinterpret_cast<float2*>(wscr + lane_s * 8) = make_float2(sa, sb);  // (every lane of the wave has read its rows: the block's head is free)
        __syncthreads();
        const int ch = wave * 64 + lane_s;  // (= threadIdx.x, from the phase's own lane id)
        if (ch < BN) {
          double a = 0.0, b2 = 0.0;
#pragma unroll
          for (int w = 0; w < NW; ++w) {
            const float2 v = *reinterpret_cast<const float2*>(smem + PATCH_BYTES + w * WSCR + ch * 8);
            a += (double)v.x;
            b2 += (double)v.y;
          }
          const int co = cur.cb * BN + ch;
          if (co < pe.Cout) {
            const long long slot = ((long long)(cur.td_i * nth + cur.th_i) * ntw + cur.tw_i) * (KS == 2 ? 8 : 1) + cur.par;  // the tile within its sample
            double* dst = pe.stats + ((slot * pe.N + cur.n) * pe.Cout + co) * 2;  // fixed-order reduction over the slots by the consumers, no atomics
            *reinterpret_cast<double2*>(dst) = make_double2(a, b2);
          }
        }
      }
    } else {
    if (DIRECT && !has_next_early) {  // (the transposed form needs the operand buffers: the barrier the direct form postpones)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
#pragma unroll
    for (int pw = 0; pw < NPW; ++pw) {  // (KS = 2: the two W parities of the work item, one after the other through the same scratch)
    const EpTile etp = {et.n, et.od0, et.oh0, et.ow0, et.co_base, et.par + pw};
    if (pw > 0) {  // the cross-wave statistic partials of parity 0 have been read
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    float st_s[EPASSES][VECW], st_q[EPASSES][VECW];
#pragma unroll
    for (int e = 0; e < EPASSES; ++e)
#pragma unroll
      for (int i = 0; i < VECW; ++i) { st_s[e][i] = 0.f; st_q[e][i] = 0.f; }
    char* scratch = smem + SCRATCH_OFF + (size_t)wave * SCRATCH_WAVE;
    dma_epilogue_pass<T, MF, NFR, KS, 0, DIRECT>(pe, accs[pw], scratch, addv, etp, wave * MF, lane_e, rowsP[pw], st_s, st_q);
    if constexpr (EPASSES > 1) {
      EpRows<MF * 2> rows;
      dma_epilogue_rows<T, MF, KS, 1>(pe, etp, wave * MF, lane_e, rows);
      dma_epilogue_pass<T, MF, NFR, KS, 1, DIRECT>(pe, accs[pw], scratch, addv, etp, wave * MF, lane_e, rows, st_s, st_q);
    }
    if constexpr (EPASSES > 2) {
      EpRows<MF * 2> rows;
      dma_epilogue_rows<T, MF, KS, 2>(pe, etp, wave * MF, lane_e, rows);
      dma_epilogue_pass<T, MF, NFR, KS, 2, DIRECT>(pe, accs[pw], scratch, addv, etp, wave * MF, lane_e, rows, st_s, st_q);
    }
    if constexpr (EPASSES > 3) {
      EpRows<MF * 2> rows;
      dma_epilogue_rows<T, MF, KS, 3>(pe, etp, wave * MF, lane_e, rows);
      dma_epilogue_pass<T, MF, NFR, KS, 3, DIRECT>(pe, accs[pw], scratch, addv, etp, wave * MF, lane_e, rows, st_s, st_q);
    }
    TL_STAMP(62);
    if (pe.stats) {
      // lane sums over its rows -> sum over the 8 row lanes of a segment (registers) -> one partial per (wave, channel) in the wave's own
      // scratch block -> fixed-order fp64 sum over the waves: deterministic, one plain store per (tile, channel)
      OPAQUE_LANE(lane_s);
      float ra[EPASSES][VECW], rb[EPASSES][VECW];
#pragma unroll
      for (int e = 0; e < EPASSES; ++e)
#pragma unroll
        for (int i = 0; i < VECW; ++i) { ra[e][i] = wave_segment_sum(st_s[e][i]); rb[e][i] = wave_segment_sum(st_q[e][i]); }
      if (lane_s < 8) {  // lanes 0..7 hold the wave's sums of VECW consecutive channels each: (sum, sum of squares) pairs, 16 bytes per two channels
        float* part = reinterpret_cast<float*>(scratch);
#pragma unroll
        for (int e = 0; e < EPASSES; ++e)
#pragma unroll
          for (int i = 0; i < VECW; i += 2)
            *reinterpret_cast<float4*>(part + 2 * (e * CH_PER_PASS + lane_s * VECW + i)) = make_float4(ra[e][i], rb[e][i], ra[e][i + 1], rb[e][i + 1]);
      }
      __syncthreads();
      const int ch = wave * 64 + lane_s;  // (= threadIdx.x, from the phase's own lane id)
      if (ch < BN) {
        double a = 0.0, b2 = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          const float2 v = *reinterpret_cast<const float2*>(smem + SCRATCH_OFF + w * SCRATCH_WAVE + ch * 8);
          a += (double)v.x;
          b2 += (double)v.y;
        }
        const int co = cur.cb * BN + ch;
        if (co < pe.Cout) {
          const long long slot = ((long long)(cur.td_i * nth + cur.th_i) * ntw + cur.tw_i) * (KS == 2 ? 8 : 1) + etp.par;  // the tile (and parity) within its sample
          double* dst = pe.stats + ((slot * pe.N + cur.n) * pe.Cout + co) * 2;  // fixed-order reduction over the slots by the consumers, no atomics
          *reinterpret_cast<double2*>(dst) = make_double2(a, b2);
        }
      }
    }
    }  // (W parities)
    }  // (the LDS-transposed form)
#ifdef GM_CONV_ABLATE
    }
#endif
    }  // (not a split-K slice)
    TL_STAMP(63);
    if (!has_next) break;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // scratch, statistic partials and the addend vector of this tile have been read: ring and patch buffer are free
    if (!EARLY && min(nchunks, nxt.ks * cps) < nchunks) issue_patch(min(nchunks, nxt.ks * cps));
    cur = nxt;
    pos += gx;
  }
}

#undef mma_tap
#undef XADDR
#undef WADDR

// variant: 1 = stride 1, 4x4x16 tile; 2 = stride 2, 2x4x16 tile; 3 = stride 1, 8x4x16 tile; 4 = sub-pixel 2x2x2 (5 planes of 5 x 17 -> 96 rows,
// four 128-row weight panels, padded to the 36 KiB of the epilogue's transpose scratch); 5 = 8x4x16 tile x 128 output channels (three 384-row
// weight panels).  Every variant ends with the 512-byte epilogue addend vector.
// tile configuration 24 (conv_sn.hip: small volumes, K-complete on 16-channel output blocks) shares this file's entry points
// the K slices of a split-K launch (cfg 11 geometry) run on conv_sk.hip's kernel: one work-group per CU, patch + all nine panels of a chunk resident

#if DMA_PART(0)
extern "C" long long gm_conv_dma_lds_bytes(int variant) {
  const long long addv = 512;
  if (variant == 4) return 5LL * 96 * DMA_ROWB + 36864 + addv + 256LL * 9 * 4;  // ... + the placement table (256 threads x (8 pieces + the slot keys))
  if (variant == 5) return 10LL * 112 * DMA_ROWB + 3LL * 384 * DMA_ROWB + addv;
  const long long plane = variant == 2 ? 304 : 112, planes = variant == 1 ? 6 : (variant == 2 ? 5 : 10);
  return planes * plane * DMA_ROWB + 3LL * 192 * DMA_ROWB + addv;
}

#endif
// Grid policy: 0 (default) = one work-group per tile; -1 = at most as many work-groups as the device holds at once (CUs x work-groups per CU
// by LDS and wave count): a work-group then walks several tiles (see the kernel's work list); n > 0 = at most n work-groups (tests).
// Measured on MI355X (profiles/r02_conv_timeline_grid_policy_ab.txt, C2 bench): the walk hides the first patch's latency (wait 340 vs 1 350-2 450
// cycles) and drops the per-tile address setup, but its next-tile placement + patch request sit on the tile's critical path (5 700 cycles)
// and the epilogue's stores queue behind the six patch requests of the wave (LDS-DMA requests are consumed at ~16 B/clk per CU): 1.238 vs
// 1.252 volumes/s -- the hardware dispatcher's own overlap of a finishing and a starting work-group is as good, so one tile per work-group stays
// the default and the walk is kept as a tested option.
#if DMA_PART(0)
int gm_dma_grid_cap = 0;
extern "C" void gm_conv_dma_set_persistent(int max_work_groups) { gm_dma_grid_cap = max_work_groups; }

// One-time phase offset of the odd work-group slot of every CU (see the kernel): cycles, 0 = off (default), -1 = automatic (half the modelled tile
// life of the launch's shape).  Process-wide; results do not depend on it.  MEASURED (profiles/r05_phase_skew_sweep.txt): tools/hwid_probe.hip
// confirms the lock step (the two work-groups of a CU start 40-620 cycles apart, round after round) and that the offset persists (20.5 k
// cycles, every round) -- and the convolutions do not care: every C2 shape is within +-1.5 % over offsets 0 ... 64 k cycles under both grid
// policies.  A wave alone on its SIMD issues a 16x16x32 MFMA every ~36 cycles, two waves every ~26 (tools/mfma_power.hip: 1 082 / 1 374
// TFLOP/s register-resident at one / two waves per SIMD), so the partner's idle phases were never worth a full-rate tap loop.
int gm_dma_phase_skew = 0;
extern "C" void gm_conv_dma_set_phase_skew(int cycles) { gm_dma_phase_skew = cycles; }
#else
extern int gm_dma_grid_cap, gm_dma_phase_skew;
#endif
#define g_dma_grid_cap gm_dma_grid_cap
#define g_dma_phase_skew gm_dma_phase_skew
static int dma_device_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus = n;
  }
  return cus;
}

static unsigned dma_grid(unsigned nwork, long long lds_bytes, int by_waves, bool splitk) {
  if (splitk || g_dma_grid_cap == 0) return nwork;  // split-K launches are small by construction
  long long cap = g_dma_grid_cap;
  if (cap < 0) {
    const int cus = dma_device_cus();
    long long per_cu = (160LL * 1024) / lds_bytes;  // co-resident work-groups per CU: by LDS and by the waves per SIMD the kernel was built for
    if (per_cu > by_waves) per_cu = by_waves;
    if (per_cu < 1) per_cu = 1;
    cap = per_cu * cus;
  }
  if (cap < 8) cap = 8;  // every XCD's item range needs a work-group (the kernel deals ranges to blockIdx.x & 7)
  return nwork < (unsigned)cap ? nwork : (unsigned)cap;
}

#if DMA_PART(0)
// geometry this kernel covers (cfg 11 / 14: stride 1, tile 4x4x16; cfg 15: stride 2, tile 2x4x16)
extern "C" int gm_conv_dma_variant(int cfg) { return cfg == 17 ? 4 : (cfg == 15 ? 2 : (cfg == 16 || cfg == 18 ? 3 : (cfg == 19 ? 5 : 1))); }

extern "C" int gm_conv_dma_eligible(const GmConvDesc* d) {
  if (d->cfg == 21 || d->cfg == 22) return 0;  // (the 32x32x16 tile structures of rounds 4-5: experiments/conv_mw, conv_w8 -- not in the library)
  if (d->cfg == 24 || d->cfg == 25) return gm_conv_sn_eligible(d);
  const int bk = d->dtype == GM_F32 ? 16 : 32;
  const int vecw = d->dtype == GM_F32 ? 4 : 8;
  const int s = d->cfg == 15 ? 2 : 1;
  if (d->cfg == 17) {  // sub-pixel up-sampling convolution: 8 parity images of a 2x2x2 kernel, output = 2x the input grid
    return d->in_mode == 3 && d->kd == 2 && d->kh == 2 && d->kw == 2 && d->sd == 1 && d->sh == 1 && d->sw == 1 && d->dd == 1 && d->dh == 1 &&
           d->dw == 1 && d->Do == 2 * d->Ds && d->Ho == 2 * d->Hs && d->Wo == 2 * d->Ws && d->Cin % bk == 0 && d->x_ld % vecw == 0 &&
           (reinterpret_cast<uintptr_t>(d->x) & 15) == 0 && d->pre_scale == nullptr && d->pre_act == 0 && d->x2 == nullptr && d->ltd == 2 && d->lth == 2 &&
           d->ltw == 4 && d->Cout % vecw == 0 && d->y_ld % vecw == 0 && (reinterpret_cast<uintptr_t>(d->y) & 15) == 0 &&
           (!d->res || (d->res_ld % vecw == 0 && (reinterpret_cast<uintptr_t>(d->res) & 15) == 0)) && !d->skip_x[0] &&
           (long long)d->N * d->Do * d->Ho * d->Wo < (1LL << 31);
  }
  if (d->in_mode == 3) return 0;
  return d->kd == 3 && d->kh == 3 && d->kw == 3 && d->sd == s && d->sh == s && d->sw == s && d->dd == 1 && d->dh == 1 && d->dw == 1 &&
         (d->in_mode == 0 || (d->in_mode == 1 && s == 1)) && d->Cin % bk == 0 && d->x_ld % vecw == 0 &&
         (reinterpret_cast<uintptr_t>(d->x) & 15) == 0 &&
         // fused GroupNorm-apply + SiLU / ReLU prologue: applied in LDS by the stride-1 variants (scale and shift together, fp32 [N][Cin])
         ((d->pre_stats[0] == nullptr &&
           ((d->pre_scale == nullptr && d->pre_shift == nullptr && d->pre_act == 0) ||
            (s == 1 && d->pre_scale != nullptr && d->pre_shift != nullptr && (reinterpret_cast<uintptr_t>(d->pre_scale) & 15) == 0 &&
             (reinterpret_cast<uintptr_t>(d->pre_shift) & 15) == 0 && (d->Cin % 4) == 0))) ||
          // ... or from the input's statistic tables (GmConvDesc.pre_stats): the K slices of a split launch only (conv_sk.hip finalises the norm in its prologue)
          (d->pre_stats[0] != nullptr && d->cfg == 11 && gm_conv_sk_eligible(d))) &&
         gm_conv_second_source_ok(d, bk, vecw) && gm_conv_shortcut_ok(d, bk, vecw) &&
         d->ltd == (d->cfg == 16 || d->cfg == 18 || d->cfg == 19 ? 3 : (s == 1 ? 2 : 1)) && d->lth == 2 &&
         d->ltw == 4 && d->Cout % vecw == 0 && d->y_ld % vecw == 0 && (reinterpret_cast<uintptr_t>(d->y) & 15) == 0 &&
         (!d->res || (d->res_ld % vecw == 0 && (reinterpret_cast<uintptr_t>(d->res) & 15) == 0)) &&
         (long long)d->N * d->Ds * d->Hs * d->Ws < (1LL << 31) && (long long)d->N * d->Do * d->Ho * d->Wo < (1LL << 31);
}

#endif
template <typename T, int NW, int MF, int S, int MINW, int KS = 3, int NFR = 4, bool PRE = false>
static void launch_dma(const GmConvDesc& d, unsigned nblocks, hipStream_t st) {
  static bool attr_set = false;
  auto kern = conv_dma_kernel<T, NW, MF, S, MINW, KS, NFR, PRE>;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) (void)hipGetLastError();
    attr_set = true;
  }
  const long long lds = gm_conv_dma_lds_bytes(gm_conv_dma_variant(d.cfg));
  const bool splitk = d.ksplit > 1 && d.kpartial != nullptr;
  constexpr int BY_WAVES = MINW * 4 / NW >= 1 ? MINW * 4 / NW : 1;  // __launch_bounds__(64 * NW, MINW): MINW waves per SIMD = MINW * 4 / NW work-groups per CU
  const unsigned grid = dma_grid(nblocks, lds, BY_WAVES, splitk);
  // ---- one-time phase offset between the co-resident work-groups of a CU (see the kernel) -----------------------------------------------------
  long long per_cu = (160LL * 1024) / lds;
  if (per_cu > BY_WAVES) per_cu = BY_WAVES;
  const unsigned resident = (unsigned)(per_cu * dma_device_cus());
  unsigned phase_wgs = 0, phase_sleeps = 0;
  if (per_cu >= 2 && !splitk && g_dma_phase_skew != 0 && nblocks >= 2 * resident) {  // (fewer than two rounds of tiles: the offset would only lengthen the launch)
    long long cycles = g_dma_phase_skew;
    if (cycles < 0) {
      // modelled tile life: MFMA issue cycles of the tile's tap loop for the co-resident waves of a SIMD + the per-tile fixed work (stamps: ~18 k)
      const long long chunks = d.Cin / (d.dtype == GM_F32 ? 16 : 32), taps = KS * KS * KS;
      const long long mfma_cycles = chunks * taps * (MF * NFR) * (d.dtype == GM_F32 ? 4 * 8 : 16);  // per wave
      const long long waves_per_simd = per_cu * NW / 4 > 0 ? per_cu * NW / 4 : 1;
      cycles = (18000 + waves_per_simd * mfma_cycles) / 2;
    }
    phase_wgs = resident;
    phase_sleeps = (unsigned)((cycles + 512) / 1024);
    if (phase_sleeps == 0) phase_wgs = 0;
  }
  kern<<<dim3(grid), 64 * NW, (size_t)lds, st>>>(d, phase_wgs, phase_sleeps);
}

// ---- the parts: each defines the launcher of its tile configurations ----------------------------------------------------------------------------
#define DMA_BY_DTYPE(...)                                                                    \
  do {                                                                                       \
    if (d.dtype == GM_F32) { using T = float; __VA_ARGS__; return 0; }                       \
    if (d.dtype == GM_BF16) { using T = bf16_raw; __VA_ARGS__; return 0; }                   \
    return -2;                                                                               \
  } while (0)
#if DMA_PART(0)
extern "C" int gm_conv_dma_launch_part0(const GmConvDesc* dp, unsigned nblocks, void* stream) {  // cfg 11: 8 waves x 32 voxels, two work-groups per CU
  const GmConvDesc& d = *dp; hipStream_t st = (hipStream_t)stream;
  const bool pre = d.pre_scale != nullptr;  // eligibility (gm_conv_dma_eligible) admits a prologue for the stride-1 3x3x3 variants only
  DMA_BY_DTYPE(if (pre) launch_dma<T, 8, 2, 1, 4, 3, 4, true>(d, nblocks, st); else launch_dma<T, 8, 2, 1, 4>(d, nblocks, st));
}
#endif
#if DMA_PART(1)
extern "C" int gm_conv_dma_launch_part1(const GmConvDesc* dp, unsigned nblocks, void* stream) {  // cfg 14: 4 waves x 64 voxels
  const GmConvDesc& d = *dp; hipStream_t st = (hipStream_t)stream;
  const bool pre = d.pre_scale != nullptr;
  DMA_BY_DTYPE(if (pre) launch_dma<T, 4, 4, 1, 2, 3, 4, true>(d, nblocks, st); else launch_dma<T, 4, 4, 1, 2>(d, nblocks, st));
}
#endif
#if DMA_PART(2)
extern "C" int gm_conv_dma_launch_part2(const GmConvDesc* dp, unsigned nblocks, void* stream) {
  const GmConvDesc& d = *dp; hipStream_t st = (hipStream_t)stream;
  // sub-pixel 2x2x2 kernels of an up-sampling convolution: 4 waves x 64 voxels at 256 registers (round 5: both W parities of a work item = two
  // accumulator sets, 128 registers -- the 8-wave x 32-voxel form at 128 registers spilled 147)
  if (d.cfg == 17) DMA_BY_DTYPE((launch_dma<T, 4, 4, 1, 2, 2>(d, nblocks, st)));
  DMA_BY_DTYPE((launch_dma<T, 8, 1, 2, 2>(d, nblocks, st)));                      // cfg 15, stride 2: 8 waves x 16 voxels, one work-group per CU
}
#endif
#if DMA_PART(3)
extern "C" int gm_conv_dma_launch_part3(const GmConvDesc* dp, unsigned nblocks, void* stream) {
  const GmConvDesc& d = *dp; hipStream_t st = (hipStream_t)stream;
  const bool pre = d.pre_scale != nullptr;
  if (d.cfg == 18) DMA_BY_DTYPE(if (pre) launch_dma<T, 8, 4, 1, 2, 3, 4, true>(d, nblocks, st); else launch_dma<T, 8, 4, 1, 2>(d, nblocks, st));  // 512 voxels x 64 channels, 8 waves x 64 voxels
  DMA_BY_DTYPE(if (pre) launch_dma<T, 16, 2, 1, 4, 3, 4, true>(d, nblocks, st); else launch_dma<T, 16, 2, 1, 4>(d, nblocks, st));                 // cfg 16: 512 voxels (8x4x16), 16 waves
}
#endif
#if DMA_PART(4)
extern "C" int gm_conv_dma_launch_part4(const GmConvDesc* dp, unsigned nblocks, void* stream) {  // cfg 19: 512 voxels x 128 channels
  const GmConvDesc& d = *dp; hipStream_t st = (hipStream_t)stream;
  const bool pre = d.pre_scale != nullptr;
  DMA_BY_DTYPE(if (pre) launch_dma<T, 8, 4, 1, 2, 3, 8, true>(d, nblocks, st); else launch_dma<T, 8, 4, 1, 2, 3, 8>(d, nblocks, st));
}
#endif

#if DMA_PART(0)
extern "C" int gm_conv_dma_launch(const GmConvDesc* dp, unsigned nblocks, void* stream) {
  if (dp->cfg == 24 || dp->cfg == 25) return gm_conv_sn_launch(dp, nblocks, stream);
  if (gm_conv_sk_eligible(dp)) return gm_conv_sk_launch(dp, nblocks, stream);
  switch (dp->cfg) {
    case 14: return gm_conv_dma_launch_part1(dp, nblocks, stream);
    case 15: case 17: return gm_conv_dma_launch_part2(dp, nblocks, stream);
    case 16: case 18: return gm_conv_dma_launch_part3(dp, nblocks, stream);
    case 19: return gm_conv_dma_launch_part4(dp, nblocks, stream);
    default: return gm_conv_dma_launch_part0(dp, nblocks, stream);
  }
}
#endif
