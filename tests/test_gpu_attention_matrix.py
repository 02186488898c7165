"""GPU (-m gpu): the attention forward kernels over their descriptor matrix -- gm_attention_forward called with a GmAttnDesc the test fills itself,
against a plain fp64 reference written here (not oracle/restatement.py), error checked per query row under test_gpu_kernels.py::_check's bars
(2e-5 fp32, 1.5e-2 bf16, times max(1, |want|_inf); measured worst row error / bar on an MI355X: fp32 0.25, bf16 0.25 -- nothing widened).

Which kernel a launch reaches is asserted in `_forward`: `kernel="staged"` (attn_kernel<T, DH, G>, csrc/attention.hip) gives NO workspace -- so a bf16
shape the LDS-DMA kernel would take stays on the register-staged one --, has Lq > 1 (not the decode kernel) and dh <= gm_attention_max_head_dim() (not the
wide kernel); `kernel="dma"` (csrc/attention_dma.hip) asserts gm_attention_workspace_bytes(d) > 0 and gives that workspace.  The wave groups G are forced
through gm_attention_set_wave_groups and reset in a `finally`; `_groups` is launch_attn's mapping (fp32 DH256 always 1; a forced 4 becomes 2 outside fp32
DH <= 64; automatic 1 / 2 / 4 at < 4, 4..7, >= 8 key tiles of KT = 32 fp32 / 64 bf16) and names the owning group in a failure message.

Every output lives in a sentinel-filled buffer with 64 spare rows (and, where the test says so, padding columns): rows past B * Lq and the padding must keep
their bits.  Forced-G launches run twice and must give the same bits (the merge order is fixed).

Operands: `randn`, and for every causal or ragged entry also DIAGONAL-PEAKED ones (`_peaked`): the first 2n channels of a head hold amp * (cos, sin) of
theta_m * position for four incommensurate frequencies, so scale * q.k = (8 / n) sum_m cos theta_m (p_q - p_k) peaks at the query's own position -- the last
keys it may see.  A causal mask off by one key, or a lost key tile, then moves 98 % or more of the rows past the bar in fp32 AND bf16 (with randn operands a
bf16 run hides it on all but a few per cent of long rows).  Head dim 4 holds two frequencies only: kept for fp32, not relied on for bf16.

  test_every_instantiation          every (T, DH) x every G launch_attn can give it, full and causal, head dims 4..256 incl. non-multiples of the vector width,
                                    9 key tiles (every group owns two or more), residual, two heads, batch 2
  test_fewer_tiles_than_groups      1, 2, 3 key tiles under forced G = 2 / 4: a group without a tile merges with weight zero
  test_causal                       Lk == Lq in {63, 64, 65, 129, 300, 1100}, automatic and forced G: the per-work-group tile-walk limit, groups whose first tile
                                    is fully masked; row 0 == v[0] + residual; last causal row == last row of the non-causal call
  test_causal_behind_a_prefix       Lk - Lq in {64, 100, 571, 37} (a multiple of KT and not; 37 < KT: a bf16 group's first tile fully masked) with 129 / 300 queries
  test_causal_needs_enough_keys     ops.attention rejects causal with Lk < Lq
  test_kv_cache_with_several_queries  k_bs / v_bs != 0 with Lq in {2, 65, 200}: first Lk rows of NaN-filled [B][cap][C] caches
  test_slices_and_alignment         q | k | v slices of one stacked buffer with NaN padding columns; bases, leading dimensions and head dims that break 16-byte
                                    alignment (qvec / kvec / vvec false: the scalar load path) at 9 tiles and G = 2; output and residual slices of wider buffers
  test_ragged_query_block           Lq not a multiple of 64
  test_both_bf16_kernels_on_one_shape  the LDS-DMA kernel (workspace) and the register-staged one (none) on the same operands, each against fp64
"""
import ctypes as C
import math
from contextlib import contextmanager

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
NAME = {F32: "fp32", BF16: "bf16"}
TOL = {F32: 2e-5, BF16: 1.5e-2}     # test_gpu_kernels.py::_check
EPS = {F32: 2.0 ** -24, BF16: 2.0 ** -8}  # one round-to-nearest, relative
KT = {F32: 32, BF16: 64}            # keys per tile of attn_kernel (AttnTraits)
VECW = {F32: 4, BF16: 8}            # elements per 16-byte vector
SENTINEL = -768.0                   # (exact in bf16)
SPARE_ROWS = 64


def _lib():
    from generativemodels_amd import _native
    return _native.lib()


def _template(dh):  # dispatch_attn
    return 32 if dh <= 32 else 64 if dh <= 64 else 128 if dh <= 128 else 256


def _groups(dtype, dh, lk, forced):  # launch_attn
    tiles = (lk + KT[dtype] - 1) // KT[dtype]
    g = forced if forced else (4 if tiles >= 8 else 2 if tiles >= 4 else 1)
    if dtype == F32 and _template(dh) == 256:
        return 1
    if dtype == F32 and _template(dh) <= 64:
        return g
    return min(g, 2)


@contextmanager
def _wave_groups(g):
    _lib().gm_attention_set_wave_groups(g)
    try:
        yield
    finally:
        _lib().gm_attention_set_wave_groups(0)


# ---- operands and the reference -------------------------------------------------------------------------------------------------------------------------
def _randn(b, h, lq, lk, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn((b, n, h * dh), generator=g, dtype=torch.float64) for n in (lq, lk, lk))


def _peaked(b, h, lq, lk, dh, seed):
    """Diagonal-peaked scores at scale = 1 / sqrt(dh): see the module docstring.  Query i sits at position i + (Lk - Lq)."""
    g = torch.Generator().manual_seed(seed)
    theta = torch.tensor([0.9, 0.37, 0.153, 0.061], dtype=torch.float64)[:max(1, min(4, dh // 2))]
    n = len(theta)

    def feat(pos):
        a = pos[:, None].double() * theta[None, :]
        return torch.stack([a.cos(), a.sin()], -1).reshape(len(pos), 2 * n)

    amp = math.sqrt(8.0 / n) * dh ** 0.25
    q = torch.randn((b, lq, h, dh), generator=g, dtype=torch.float64) * 0.05
    k = torch.randn((b, lk, h, dh), generator=g, dtype=torch.float64) * 0.05
    q[..., :2 * n] = feat(torch.arange(lq) + (lk - lq))[None, :, None, :] * amp
    k[..., :2 * n] = feat(torch.arange(lk))[None, :, None, :] * amp
    v = torch.randn((b, lk, h * dh), generator=g, dtype=torch.float64)
    return q.reshape(b, lq, h * dh), k.reshape(b, lk, h * dh), v


def _operands(kind, dtype, b, h, lq, lk, dh, seed, res):
    q, k, v = (t.to(dtype) for t in (_randn if kind == "randn" else _peaked)(b, h, lq, lk, dh, seed))
    r = torch.randn((b, lq, h * dh), generator=torch.Generator().manual_seed(seed + 1000)).to(dtype) if res else None
    return q, k, v, r


def _reference(q, k, v, h, scale, causal, res=None):
    """fp64 attention of operands already rounded to the tested dtype: scores, mask j > i + (Lk - Lq), softmax, times V, plus residual."""
    b, lq, c = q.shape
    lk, dh = k.shape[1], c // h
    qh, kh, vh = (t.double().reshape(b, -1, h, dh).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    if causal:
        hidden = torch.arange(lk)[None, :] > torch.arange(lq)[:, None] + (lk - lq)
        s = s.masked_fill(hidden, float("-inf"))
    o = (s.softmax(-1) @ vh).transpose(1, 2).reshape(b, lq, c)
    return o + res.double() if res is not None else o


# ---- the launcher: a GmAttnDesc filled here ------------------------------------------------------------------------------------------------------------
def _forward(dtype, b, h, lq, lk, dh, scale, q, k, v, o, res=None, causal=False, k_bs=0, v_bs=0, kernel="staged"):
    """gm_attention_forward on (pointer, leading dimension) pairs; asserts the kernel the geometry reaches (module docstring)."""
    from generativemodels_amd import _native
    lib = _lib()
    d = _native.GmAttnDesc()
    (d.q, d.q_ld), (d.k, d.k_ld), (d.v, d.v_ld), (d.o, d.o_ld) = q, k, v, o
    d.res, d.res_ld = res if res is not None else (None, 0)
    d.B, d.H, d.Lq, d.Lk, d.dh = b, h, lq, lk, dh
    d.scale, d.dtype = float(scale), 0 if dtype == F32 else 1
    d.causal, d.k_bs, d.v_bs = int(causal), k_bs, v_bs
    d.workspace, d.workspace_bytes = None, 0
    ws_bytes = lib.gm_attention_workspace_bytes(C.byref(d))
    assert lq > 1 and dh <= lib.gm_attention_max_head_dim(), "the decode / wide-head kernels are not what this module launches"
    ws = None
    if kernel == "dma":
        assert ws_bytes > 0, "this geometry is not the LDS-DMA kernel's"
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
    else:
        assert kernel == "staged" and not d.workspace  # no workspace: gm_attention_dma_try declines, attn_kernel<T, DH, G> runs
    rc = lib.gm_attention_forward(C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.gm_last_error()
    torch.cuda.synchronize()
    del ws


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


class _Case:
    """Device layout of one call.  stacked = (first column, trailing columns): q | k | v are slices of ONE [B][L][first + 3c + trailing] buffer (Lq == Lk) whose
    other columns hold NaN; kv_cap: k and v are the first Lk rows of [B][kv_cap][C] buffers (k_bs = v_bs = kv_cap * C), the other rows hold NaN; out_pad /
    res_pad = (first column, trailing columns) of the wider buffers the output / residual are slices of."""

    def __init__(self, dtype, h, q, k, v, res=None, causal=False, stacked=None, kv_cap=None, out_pad=(0, 0), res_pad=(0, 0)):
        self.dtype, self.h, self.causal = dtype, h, causal
        self.b, self.lq, self.c = q.shape
        self.lk, self.dh = k.shape[1], self.c // h
        self.scale = 1 / math.sqrt(self.dh)
        b, lq, lk, c = self.b, self.lq, self.lk, self.c
        nan = float("nan")
        self.k_bs = self.v_bs = 0
        if stacked is not None:
            assert lq == lk and kv_cap is None
            first, trailing = stacked
            self.qkv = torch.full((b, lq, first + 3 * c + trailing), nan, dtype=dtype)
            for i, t in enumerate((q, k, v)):
                self.qkv[..., first + i * c:first + (i + 1) * c] = t
            self.qkv = self.qkv.to(DEV)
            self.qd, self.kd, self.vd = (self.qkv[..., first + i * c:first + (i + 1) * c] for i in range(3))
        else:
            self.qd = q.to(DEV)
            if kv_cap is not None:
                assert kv_cap > lk
                caches = []
                for t in (k, v):
                    cache = torch.full((b, kv_cap, c), nan, dtype=dtype)
                    cache[:, :lk] = t
                    caches.append(cache.to(DEV))
                self.kd, self.vd = (t[:, :lk] for t in caches)
                self.k_bs = self.v_bs = kv_cap * c
            else:
                self.kd, self.vd = k.to(DEV), v.to(DEV)
        self.out_pad = out_pad
        self.rd = None
        if res is not None:
            wide = torch.full((b, lq, res_pad[0] + c + res_pad[1]), nan, dtype=dtype)
            wide[..., res_pad[0]:res_pad[0] + c] = res
            self.rd = wide.to(DEV)[..., res_pad[0]:res_pad[0] + c]

    @staticmethod
    def _pl(t):
        assert t.stride(-1) == 1
        return t.data_ptr(), t.stride(-2)

    def run(self, kernel="staged", causal=None):
        """One launch into a fresh sentinel-filled buffer; returns the (B, Lq, C) result on the host after checking that every element outside it kept its bits."""
        b, lq, c = self.b, self.lq, self.c
        first, trailing = self.out_pad
        buf = torch.full((b * lq + SPARE_ROWS, first + c + trailing), SENTINEL, dtype=self.dtype, device=DEV)
        o = buf[:, first:first + c]
        _forward(self.dtype, b, self.h, lq, self.lk, self.dh, self.scale, self._pl(self.qd), self._pl(self.kd), self._pl(self.vd), self._pl(o),
                 res=self._pl(self.rd) if self.rd is not None else None, causal=self.causal if causal is None else causal,
                 k_bs=self.k_bs, v_bs=self.v_bs, kernel=kernel)
        host = buf.cpu()
        fill = _bits(torch.full((1,), SENTINEL, dtype=self.dtype))[0].item()
        outside = _bits(host).clone()
        outside[:b * lq, first:first + c] = fill
        touched = (outside != fill).nonzero()
        assert touched.numel() == 0, (f"{touched.shape[0]} elements outside the output slice were written, the first at (row, column) {tuple(touched[0].tolist())} of a "
                                      f"[{b * lq} + {SPARE_ROWS} spare rows][{first} + {c} + {trailing}] buffer")
        return host[:b * lq, first:first + c].reshape(b, lq, c)

    def run_twice(self, what):
        got, again = self.run(), self.run()
        assert torch.equal(_bits(got), _bits(again)), f"{what}: two launches of the same call differ in {(_bits(got) != _bits(again)).sum().item()} elements"
        return got


def _check_rows(got, want, dtype, what, h, lk, causal, groups):
    """test_gpu_kernels.py::_check per query row: names the first failing row, its query block, the key tile of its diagonal and the wave group owning it."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    b, lq, c = want.shape
    bar = TOL[dtype] * max(1.0, want.abs().max().item())
    err = (got - want).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    row_err = err.reshape(b, lq, h, c // h).amax(-1)  # (b, row, head)
    print(f"[attention matrix] {what}: worst row error / bar {row_err.max().item() / bar:.3f}")
    bad = row_err > bar
    if bad.any():
        rows = bad.any(0).any(-1).nonzero().flatten()
        row = rows[0].item()
        bi, hi = bad[:, row].nonzero()[0].tolist()
        key = min(lk - 1, row + (lk - lq)) if causal else lk - 1
        tile = key // KT[dtype]
        raise AssertionError(f"{what}: {len(rows)} of {lq} query rows over the bar {bar:.3e}; first: row {row} (batch {bi}, head {hi}, query block {row // 64}) "
                             f"|err| {row_err[bi, row, hi].item():.3e}; its {'diagonal' if causal else 'last'} key {key} is in key tile {tile}, "
                             f"wave group {tile % groups} of {groups}")


def _run_and_check(dtype, b, h, lq, lk, dh, forced, causal, res, what, seed, **layout):
    """Both operand kinds of one matrix entry on the register-staged kernel under `forced` wave groups (0 = automatic), each against fp64, each launched twice."""
    groups = _groups(dtype, dh, lk, forced)
    for kind in ("randn", "peaked"):
        q, k, v, r = _operands(kind, dtype, b, h, lq, lk, dh, seed, res)
        case = _Case(dtype, h, q, k, v, res=r, causal=causal, **layout)
        with _wave_groups(forced):
            got = case.run_twice(f"{what}, {kind}")
        _check_rows(got, _reference(q, k, v, h, case.scale, causal, r), dtype, f"{what}, {kind}", h, lk, causal, groups)


def _gid(dtype, dh, forced, lk=None):
    if not forced:
        return f"{NAME[dtype]}-DH{_template(dh)}-Gauto{_groups(dtype, dh, lk, 0)}"
    eff = _groups(dtype, dh, 1, forced)
    return f"{NAME[dtype]}-DH{_template(dh)}-G{forced}{'' if eff == forced else f'as{eff}'}"


# ---- every instantiation ---------------------------------------------------------------------------------------------------------------------------------
HEAD_DIMS = (4, 24, 32, 40, 64, 72, 128, 200, 256)  # DH 32, 32, 32, 64, 64, 128, 128, 256, 256
# (fp32 DH256 runs one wave group whatever is forced -- two would need 256 registers per wave --: its forced 2 and 4 would repeat the G1 launch and are left out)
INSTANCES = [(dt, dh, g, causal) for dt in DTYPES for dh in HEAD_DIMS for g in (1, 2, 4) for causal in (False, True)
             if not (dt == F32 and _template(dh) == 256 and g != 1)]


@pytest.mark.parametrize("dtype,dh,forced,causal", INSTANCES, ids=[f"{_gid(dt, dh, g)}-d{dh}-{'causal' if c else 'full'}" for dt, dh, g, c in INSTANCES])
def test_every_instantiation(dtype, dh, forced, causal):
    """attn_kernel<T, DH, G> for every (T, DH) and every G launch_attn gives it: 9 key tiles (the last one ragged), so that each of four groups owns two or more;
    150 queries against them (a bf16 DH64/128/256 shape of the LDS-DMA kernel, kept here by giving no workspace), or as many queries as keys when causal."""
    lk = 8 * KT[dtype] + 13
    lq = lk if causal else 150
    _run_and_check(dtype, 2, 2, lq, lk, dh, forced, causal, res=not causal, what=f"{_gid(dtype, dh, forced)} d{dh} {lq}x{lk}", seed=300 + dh)


SHORT = [(dt, dh, g, tiles, causal) for dt in DTYPES for dh in (24, 64, 128, 256) for g in (2, 4) for tiles in (1, 2, 3) for causal in (False, True)
         if not (dt == F32 and _template(dh) == 256)]  # (fp32 DH256: one group always, see INSTANCES)


@pytest.mark.parametrize("dtype,dh,forced,tiles,causal", SHORT,
                         ids=[f"{_gid(dt, dh, g)}-d{dh}-tiles{t}-{'causal' if c else 'full'}" for dt, dh, g, t, c in SHORT])
def test_fewer_tiles_than_groups(dtype, dh, forced, tiles, causal):
    """1, 2 or 3 key tiles under two or four forced wave groups: a group that owns no tile hands over (m, l, o) = (-inf, 0, 0) and must merge with weight zero."""
    lk = tiles * KT[dtype] - 5
    lq = lk if causal else 70
    _run_and_check(dtype, 2, 2, lq, lk, dh, forced, causal, res=False, what=f"{_gid(dtype, dh, forced)} d{dh} {lq}x{lk} ({tiles} tiles)", seed=400 + dh + tiles)


# ---- causal --------------------------------------------------------------------------------------------------------------------------------------------
CAUSAL_DH = {63: 40, 64: 64, 65: 24, 129: 128, 300: 64, 1100: 32}  # tokens -> head dim (1100 x 32: the transformer of test_c5)
CAUSAL = [(dt, n, g) for dt in DTYPES for n in CAUSAL_DH for g in (0, 1, 2, 4)]


@pytest.mark.parametrize("dtype,n,forced", CAUSAL, ids=[f"{_gid(dt, CAUSAL_DH[n], g, n)}-d{CAUSAL_DH[n]}-L{n}" for dt, n, g in CAUSAL])
def test_causal(dtype, n, forced):
    """Causal self-attention (Lk == Lq) at lengths that straddle the 64-query block and the key tile, three heads, batch 2, residual: against fp64 per row; row 0
    sees one key, so it is v[0] + residual to one rounding; the last row sees every key, so it matches the non-causal call of the same operands within the bar."""
    dh, b, h = CAUSAL_DH[n], 2, 3
    groups = _groups(dtype, dh, n, forced)
    for kind in ("randn", "peaked"):
        what = f"{_gid(dtype, dh, forced, n)} d{dh} causal {n}x{n}, {kind}"
        q, k, v, r = _operands(kind, dtype, b, h, n, n, dh, 500 + n, res=True)
        case = _Case(dtype, h, q, k, v, res=r, causal=True)
        with _wave_groups(forced):
            got = case.run_twice(what)
            full = case.run(causal=False)
        want = _reference(q, k, v, h, case.scale, True, r)
        _check_rows(got, want, dtype, what, h, n, True, groups)
        _check_rows(full, _reference(q, k, v, h, case.scale, False, r), dtype, what + " (the non-causal call)", h, n, False, groups)
        first = v[:, 0].double() + r[:, 0].double()
        err0 = (got[:, 0].double() - first).abs()
        assert bool((err0 <= EPS[dtype] * first.abs().clamp(min=1.0)).all()), f"{what}: row 0 differs from v[0] + residual by {err0.max().item():.3e}"
        bar = TOL[dtype] * max(1.0, want.abs().max().item())
        err_last = (got[:, -1].double() - full[:, -1].double()).abs().max().item()
        assert math.isfinite(err_last) and err_last <= bar, \
            f"{what}: the last causal row differs from the non-causal call's by {err_last:.3e} > {bar:.3e} (key tile {(n - 1) // KT[dtype]}, wave group {(n - 1) // KT[dtype] % groups} of {groups})"


# (queries, Lk - Lq, head dim).  129 x 700 x 24: a prefill behind a cache of the odd-geometry transformer.  An offset below the key tile (37) is the only place where a
# bf16 wave group's FIRST tile is fully masked for some query (its tiles and the 64-query blocks coincide otherwise): 300 + 37 keys take two groups automatically
PREFIX_SHAPES = [(129, 64, 64), (129, 100, 40), (129, 571, 24), (129, 37, 128), (300, 37, 32)]
PREFIX = [(dt, shape, g) for dt in DTYPES for shape in PREFIX_SHAPES for g in (0, 1, 2, 4)]


@pytest.mark.parametrize("dtype,shape,forced", PREFIX, ids=[f"{_gid(dt, s[2], g, s[0] + s[1])}-d{s[2]}-q{s[0]}-behind{s[1]}" for dt, s, g in PREFIX])
def test_causal_behind_a_prefix(dtype, shape, forced):
    """Causal attention of queries behind `offset` earlier keys (query i sees keys j <= i + offset): an offset that is a multiple of the key tile (64) and three that
    are not, so the tile that holds a work-group's last visible key and the first fully masked tile of a wave group move against the query blocks."""
    lq, offset, dh = shape
    _run_and_check(dtype, 2, 2, lq, lq + offset, dh, forced, True, res=False, what=f"{_gid(dtype, dh, forced, lq + offset)} d{dh} causal {lq}x{lq + offset}", seed=600 + offset + lq)


def test_causal_needs_enough_keys():
    from generativemodels_amd import ops
    q, k = torch.zeros((1, 5, 32), device=DEV), torch.zeros((1, 4, 32), device=DEV)
    with pytest.raises(ValueError):
        ops.attention(q, k, k, 1, 1.0, causal=True)


# ---- KV cache, slices, alignment, ragged rows ----------------------------------------------------------------------------------------------------------------
CACHE_DH = {2: 32, 65: 64, 200: 128}  # queries -> head dim
CACHE = [(dt, lq, causal) for dt in DTYPES for lq in CACHE_DH for causal in (False, True)]


@pytest.mark.parametrize("dtype,lq,causal", CACHE, ids=[f"{_gid(dt, CACHE_DH[lq], 0, 333)}-d{CACHE_DH[lq]}-q{lq}-{'causal' if c else 'full'}" for dt, lq, c in CACHE])
def test_kv_cache_with_several_queries(dtype, lq, causal):
    """K and V are the first 333 rows of [2][384][C] caches (k_bs = v_bs = 384 * C != Lk * C): sample 1 starts at the batch stride, and the rows from Lk to the
    capacity hold NaN, so a read past the key count shows.  (bf16, head dim 64 / 128, 200 queries: the batch stride alone keeps the call off the LDS-DMA kernel.)"""
    dh = CACHE_DH[lq]
    _run_and_check(dtype, 2, 2, lq, 333, dh, 0, causal, res=False, what=f"{_gid(dtype, dh, 0, 333)} d{dh} cache {lq}x333 of 384", seed=700 + lq, kv_cap=384)


# (fp32 dh 38 / 40, bf16 dh 36 / 100 / 40; what breaks the vector path): "dh" -- the head dim is no multiple of the vector width, so from the second head on the slice
# base is misaligned too; "base" -- the stacked buffer's slices start one element in; "ld" -- the leading dimension is VECW * n + 1
LAYOUTS = [(F32, 64, "aligned"), (F32, 40, "base"), (F32, 40, "ld"), (F32, 38, "dh"),
           (BF16, 64, "aligned"), (BF16, 40, "base"), (BF16, 40, "ld"), (BF16, 36, "dh"), (BF16, 100, "dh")]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("dtype,dh,how", LAYOUTS, ids=[f"{_gid(dt, dh, 2)}-d{dh}-{how}" for dt, dh, how in LAYOUTS])
def test_slices_and_alignment(dtype, dh, how, causal):
    """q | k | v as slices of one stacked buffer wider than 3c with NaN in its other columns, the output and the residual as slices of wider buffers (the output's other
    columns keep their bits: _Case.run), three heads, batch 2, 9 key tiles under two wave groups -- on the 16-byte vector loads ("aligned") and on the scalar path."""
    w = VECW[dtype]
    c = 3 * dh
    first, trailing = {"aligned": (w, 2 * w), "dh": (0, 2 * w), "base": (1, 2 * w - 1), "ld": (0, 1)}[how]
    ld = first + 3 * c + trailing
    es = 4 if dtype == F32 else 2
    vector = dh % w == 0 and ld % w == 0 and (first * es) % 16 == 0 and (c * es) % 16 == 0
    assert vector == (how == "aligned")  # (the kernel's qvec / kvec / vvec for these buffers: torch allocations are 256-byte aligned)
    n = 8 * KT[dtype] + 13
    _run_and_check(dtype, 2, 3, n, n, dh, 2, causal, res=True, what=f"{_gid(dtype, dh, 2)} d{dh} slices ({how}) {n}x{n}{' causal' if causal else ''}", seed=800 + dh,
                   stacked=(first, trailing), out_pad=(3, 5), res_pad=(w, 1))


RAGGED = [(dt, lq) for dt in DTYPES for lq in (2, 65, 100, 191)]


@pytest.mark.parametrize("dtype,lq", RAGGED, ids=[f"{_gid(dt, 72, 0, 200)}-d72-q{lq}" for dt, lq in RAGGED])
def test_ragged_query_block(dtype, lq):
    """A query count that ends inside a 64-query block: the lanes past Lq compute on zero queries and must store nothing (_Case.run: the rows after B * Lq of the output
    buffer keep their bits; sample 1's rows directly follow sample 0's last one)."""
    _run_and_check(dtype, 2, 2, lq, 200, 72, 0, False, res=True, what=f"{_gid(dtype, 72, 0, 200)} d72 ragged {lq}x200", seed=900 + lq, out_pad=(0, 8))


# ---- the two bf16 kernels on one shape ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 333, 200, 64), (1, 1, 700, 520, 256)], ids=lambda s: f"bf16-DH{s[4]}-B{s[0]}H{s[1]}q{s[2]}k{s[3]}")
def test_both_bf16_kernels_on_one_shape(shape):
    """A shape both kernels serve, through the LDS-DMA kernel (the workspace of gm_attention_workspace_bytes given) and through the register-staged one (none):
    each against fp64 under the bar; the two are not held to each other more tightly."""
    b, h, lq, lk, dh = shape
    for kind in ("randn", "peaked"):
        q, k, v, r = _operands(kind, BF16, b, h, lq, lk, dh, 1000 + dh, res=True)
        case = _Case(BF16, h, q, k, v, res=r)
        want = _reference(q, k, v, h, case.scale, False, r)
        _check_rows(case.run(kernel="dma"), want, BF16, f"LDS-DMA kernel d{dh} {lq}x{lk}, {kind}", h, lk, False, 1)
        _check_rows(case.run(kernel="staged"), want, BF16, f"register-staged kernel d{dh} {lq}x{lk}, {kind}", h, lk, False, _groups(BF16, dh, lk, 0))
