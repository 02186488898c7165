"""GPU (-m gpu): the sampling-head kernels and the categorical draw of csrc/transformer_ops.hip over the sizes at which
a one-wave-per-row kernel can go wrong: vocabularies below, at and above one 64-lane pass (1, 63, 64, 65), several passes (257) and many
(4097); rows that are views of a wider poisoned buffer; ties 64 entries apart (the same lane in two passes) and across +0 / -0.

Bars.  sample_probs: the zero pattern exact, values within the suite's existing 1e-6 (tests/test_gpu_models.py).  token_log_prob: torch's own
fp32 CPU evaluation of the reference formula log(softmax(x))[t] differs from fp64 log_softmax by at most 1.75e-7 of max(1, |log p|) on these
rows (measured over both dtypes' rows, every V; log p reaches -73.5); the bar is 4x that, 7.0e-7 of max(1, |log p|).  embed_tokens, decode_advance: exact.  sample_index: a
zero-probability entry is never drawn -- also where rounding leaves the owning lane's running sum below the target (the last test)."""
import math

import pytest
import torch

import restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = [1, 63, 64, 65, 257, 4097]
DTYPES = [torch.float32, torch.bfloat16]
PAD = 100.0  # what the wider buffer holds beyond column V: a logit that would win every row
LOGP_BAR = 7.0e-7


def _ops():
    from generativemodels_amd import ops
    return ops


def _strided(rows, dtype):
    """rows (R, V) -> a [:, :V] view of a device buffer 7 columns wider, the extra columns holding PAD."""
    r, v = rows.shape
    buf = torch.full((r, v + 7), PAD, dtype=dtype)
    buf[:, :v] = rows.to(dtype)
    view = buf.to(DEV)[:, :v]
    assert view.stride(0) == v + 7
    return view


def _prob_rows(v, seed):
    """fp32 rows (R, V): three random rows; ties at the 2nd largest value 64 entries apart; ties at the smallest value 64 apart (the k-th for
    k = V - 1); +0.0 and -0.0 tied as 2nd largest 64 apart; an all-negative row; a row with -inf entries."""
    g = torch.Generator().manual_seed(seed)
    rows = [2.0 * torch.randn(v, generator=g) for _ in range(3)]
    a, b = (v // 3, v // 3 + 64) if v > 64 + v // 3 else (0, v - 1)
    t = 2.0 * torch.randn(v, generator=g).clamp(-3, 3)
    if v >= 3:
        t[a], t[b], t[(a + 1) % v if (a + 1) % v != b else (a + 2) % v] = 6.5, 6.5, 7.0
    rows.append(t)
    t = 2.0 * torch.randn(v, generator=g).clamp(-3, 3)
    t[a], t[b] = -6.5, -6.5
    rows.append(t)
    t = -(2.0 * torch.randn(v, generator=g).abs()) - 0.5
    if v >= 3:
        t[a], t[b], t[(a + 1) % v if (a + 1) % v != b else (a + 2) % v] = 0.0, -0.0, 3.0
    rows.append(t)
    rows.append(-(2.0 * torch.randn(v, generator=g).abs()) - 1.0)
    t = 2.0 * torch.randn(v, generator=g)
    if v >= 2:
        t[::3] = -math.inf
        t[v - 1] = 1.0
    rows.append(t)
    return torch.stack(rows)


@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_sample_probs(v, dtype):
    ops = _ops()
    rows = _prob_rows(v, seed=v).to(dtype)
    view = _strided(rows, dtype)
    up = rows.double()
    for top_k in sorted({k for k in (1, 2, v - 1, v, v + 5) if k >= 1}) + [None]:
        for temp in (0.25, 1.0, 4.0):
            for bos in (0, v - 1, -1):
                # bos = -1 is the "none" that autograd.py passes: nothing is zeroed (an empty index list in the reference's assignment)
                want = R.transformer_sample_probs(up.clone(), temp, top_k, bos if bos >= 0 else [])
                got = ops.sample_probs(view, temp, top_k, bos).cpu()
                what = f"V {v} {str(dtype)[6:]} top_k {top_k} temperature {temp} bos {bos}"
                bad = (got == 0) != (want == 0)
                assert not bool(bad.any()), f"{what}: zero pattern differs at (row, column) {bad.nonzero()[:6].tolist()}"
                err = (got.double() - want).abs().max().item()
                assert err <= 1e-6, f"{what}: max|err| {err:.3e}"


def _logp_rows(v, seed):
    """rows and targets: targets at 0, 63, 64, V - 1 (those inside the row); the target's logit 0 .. 70 below the row maximum."""
    g = torch.Generator().manual_seed(seed)
    targets = sorted({t for t in (0, 63, 64, v - 1) if 0 <= t < v})
    rows, tg = [], []
    for t in targets:
        for depth in (0.0, 20.0, 70.0):
            r = 3.0 * torch.randn(v, generator=g).clamp(-3, 3)
            r[t] = 9.0 - depth
            r[(t + 1) % v] = max(r[(t + 1) % v].item(), 9.0 if v > 1 else r[t].item())
            rows.append(r), tg.append(t)
    return torch.stack(rows), torch.tensor(tg)


@pytest.mark.parametrize("v", VS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_token_log_prob(v, dtype):
    ops = _ops()
    rows, tg = _logp_rows(v, seed=100 + v)
    rows = rows.to(dtype)
    want = torch.log_softmax(rows.double(), -1).gather(1, tg[:, None])[:, 0]
    assert want.min().item() > -80
    got = ops.token_log_prob(_strided(rows, dtype), tg.to(DEV)).cpu().double()
    err = ((got - want).abs() / want.abs().clamp_min(1.0))
    print(f"[sampling] token_log_prob V {v} {str(dtype)[6:]}: max err / max(1, |log p|) {err.max().item():.3e} (bar {LOGP_BAR:.1e})")
    assert err.max().item() <= LOGP_BAR, f"V {v} {dtype}: row {int(err.argmax())} target {int(tg[err.argmax()])}: {err.max().item():.3e}"


@pytest.mark.parametrize("v", [65, 4097])
def test_token_log_prob_underflow_row_gives_the_reference_formulas_minus_infinity(v):
    ops = _ops()
    row = torch.zeros((1, v))
    row[0, 0], row[0, v - 1] = 100.0, -100.0
    tg = torch.tensor([v - 1])
    want = torch.log(torch.softmax(row, -1))[0, v - 1]  # the reference's own fp32 formula
    assert want.item() == -math.inf
    got = ops.token_log_prob(_strided(row, torch.float32), tg.to(DEV)).cpu()
    assert got[0].item() == want.item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("b,t,c,maxpos", [(3, 7, 5, 9), (2, 65, 72, 70), (3, 4, 512, 11), (2, 1100, 512, 1100)])
def test_embed_tokens_bit_exact(b, t, c, maxpos, dtype):
    """pos0 > 0 and pos0 + T == the table's length; (2, 1100, 512) is above 4096 x 256 elements, so the grid-stride loop wraps."""
    ops = _ops()
    g = torch.Generator().manual_seed(b * 1000 + c)
    tok = torch.randn((50, c), generator=g).to(dtype)
    pos = torch.randn((maxpos, c), generator=g).to(dtype)
    idx = torch.randint(0, 50, (b, t), generator=g)
    for pos0 in sorted({0, (maxpos - t) // 2, maxpos - t}):
        want = tok[idx] + pos[pos0:pos0 + t][None]
        assert want.dtype == dtype
        got = ops.embed_tokens(idx.to(DEV), tok.to(DEV), pos.to(DEV), pos0).cpu()
        assert torch.equal(got, want), f"pos0 {pos0}: {(got != want).sum().item()} elements differ"


@pytest.mark.parametrize("b", [1, 64, 65, 200])
def test_decode_advance_exact(b):
    ops = _ops()
    length = 6
    g = torch.Generator().manual_seed(b)
    for p in (0, 3, length - 2, length - 1):  # length - 1: p + 1 is the sequence length -- nothing is written, the position still advances
        flat = torch.randint(0, 1000, (b * length + 8,), generator=g)
        idx = torch.randint(0, 1000, (b, 1), generator=g)
        tokens = torch.full((b, 1), -7, dtype=torch.long)
        fd = flat.to(DEV)
        seq = fd[:b * length].view(b, length)
        pos_dev = torch.tensor([p], dtype=torch.int32, device=DEV)
        td = tokens.to(DEV)
        ops.decode_advance(pos_dev, td, idx.to(DEV), seq)
        want = flat.clone()
        if p + 1 < length:
            want[:b * length].view(b, length)[:, p + 1] = idx[:, 0]
        assert torch.equal(fd.cpu(), want), f"B {b} p {p}: the sequence buffer (or what lies behind it) differs"
        assert torch.equal(td.cpu(), idx) and pos_dev.item() == p + 1


@pytest.mark.parametrize("v", [1, 64, 65, 4097])
def test_sample_index_never_returns_a_zero_probability_entry(v):
    ops = _ops()
    g = torch.Generator().manual_seed(v)
    n = 256  # draws per kind of row (each row gets its own uniform number)
    first, last = torch.zeros((n, v)), torch.zeros((n, v))
    first[:, 0], last[:, v - 1] = 0.7, 1e-3
    gen = torch.Generator(device=DEV).manual_seed(5)
    assert ops.sample_index(first.to(DEV), generator=gen).flatten().tolist() == [0] * n
    assert ops.sample_index(last.to(DEV), generator=gen).flatten().tolist() == [v - 1] * n
    lead = torch.rand((n, v), generator=g)
    lead[:, :v // 2] = 0  # leading zeros: half the row (for V = 1 the row keeps its one entry)
    holes = torch.rand((n, v), generator=g)
    holes[:, 1::2] = 0
    holes[:, v - 1] = 0 if v > 1 else holes[:, v - 1]
    for name, probs in (("leading zeros", lead), ("holes and a zero last entry", holes)):
        got = ops.sample_index(probs.to(DEV), generator=gen).flatten().cpu()
        assert got.min().item() >= 0 and got.max().item() < v
        assert bool((probs[torch.arange(n), got] > 0).all()), f"V {v}, {name}: a zero-probability index was drawn"
    if v >= 64:
        # a row of two equal halves of mass: the draws split between them (the scan crosses every lane)
        two = torch.zeros((4096, v))
        two[:, 0], two[:, v - 1] = 1.0, 1.0
        got = ops.sample_index(two.to(DEV), generator=gen).flatten().cpu()
        assert set(got.tolist()) == {0, v - 1} and abs((got == 0).double().mean().item() - 0.5) < 0.05


def _scan_fp32(pr):
    """The draw kernel's arithmetic in numpy fp32: per-lane sums over ceil(V / 64) consecutive entries, then the 6-step shuffle-up scan."""
    import numpy as np
    f = np.float32
    v = len(pr)
    per = (v + 63) // 64
    loc = np.zeros(64, f)
    for lane in range(64):
        s = f(0)
        for j in range(lane * per, min(v, lane * per + per)):
            s = f(s + pr[j])
        loc[lane] = s
    incl = loc.copy()
    o = 1
    while o < 64:
        prev = incl.copy()
        for lane in range(o, 64):
            incl[lane] = f(incl[lane] + prev[lane - o])
        o *= 2
    return loc, incl


def test_sample_index_when_the_owner_lanes_running_sum_ends_below_the_target():
    """V = 128, two entries per lane, the second of probability zero.  The owning lane restarts its running sum from incl - loc, a rounded
    difference, so the sum can end one ulp below the lane's inclusive sum; a uniform number whose target IS that inclusive sum then finds no
    entry reaching it.  The draw must be the lane's positive entry, not the zero-probability entry behind it.  The rows and uniform numbers
    are found by replaying the kernel's fp32 arithmetic on the host."""
    import numpy as np
    from generativemodels_amd._native import check, lib
    ops = _ops()
    f = np.float32
    rng = np.random.default_rng(1)
    rows, us, lanes = [], [], []
    for _ in range(40):
        pr = np.zeros(128, f)
        pr[0::2] = rng.random(64).astype(f)
        loc, incl = _scan_fp32(pr)
        total = incl[63]
        for lane in range(1, 64):
            excl = f(incl[lane] - loc[lane])
            if not (f(excl + pr[2 * lane]) < incl[lane] and excl <= incl[lane] and incl[lane - 1] < incl[lane]):
                continue
            u = f(incl[lane] / total)
            for _ in range(6):
                t = f(u * total)
                if t == incl[lane]:
                    break
                u = np.nextafter(u, f(2) if t < incl[lane] else f(0))
            if f(u * total) == incl[lane] and u < 1:
                rows.append(pr), us.append(u), lanes.append(lane)
    assert len(rows) >= 8, "the host replay found too few rows whose running sum ends below the target"
    probs = torch.from_numpy(np.stack(rows)).to(DEV)
    u = torch.from_numpy(np.array(us, dtype=f)).to(DEV)
    out = torch.full((len(rows), 1), -1, dtype=torch.long, device=DEV)
    check(lib().gm_sample_index(probs.data_ptr(), len(rows), 128, u.data_ptr(), out.data_ptr(), ops._stream()), "gm_sample_index")
    got = out.flatten().cpu().tolist()
    assert got == [2 * lane for lane in lanes], [(g, 2 * lane) for g, lane in zip(got, lanes) if g != 2 * lane][:8]
